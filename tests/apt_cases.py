"""The shapes and inputs of the all-pass transform tests (tests/test_apt_np_cpu.py, tests/test_gpu_apt.py)."""
import numpy as np

from tests import apt_np as P
from tests import train_np as T

f32 = np.float32
SHAPES = [(2, 1), (13, 3), (16, 2), (17, 1)]             # (subFeatLen, nSubFeat): the smallest, the usual 13 x 3, an even and an odd length
SIZES = [1, 3, 5, 63, 64, 65, 257]                       # Gaussians per leaf: fewer than a slice of k_apt_lhood's bias pass, around a wave, more than a workgroup
TREES = [[1], [2, 3], [4, 5, 3], [2, 7]]
BLT_ALPHAS = [-0.899, -0.3, 0.0, 0.05, 0.6]
SLAPT_PARAMS = [(0.2,), (-0.3, 0.1), (0.05, -0.02, 0.01, 0.005)]
RECOVERY_SHAPES = [(13, 3, 64), (16, 2, 65), (13, 3, 5), (17, 1, 257)]      # (subFeatLen, nSubFeat, Gaussians)
RECOVERY_ALPHAS = [-0.3, -0.1, 0.05, 0.2]


def ref_ns(G, most=50):
    r = [most] * (G // most)
    if G % most:
        r.append(G % most)
    return r


def sizes_for(si, ti):
    """the leaves of tree ti take consecutive sizes, rotated by the shape's index: every size meets every shape over the four trees"""
    first = sum(len(t) for t in TREES[:ti])
    return [SIZES[(first + j + 2 * si) % len(SIZES)] for j in range(len(TREES[ti]))]


def model(L, nSub, leafSizes, leaves, seed, decay=False):
    """a random model (tests.train_np.Model) whose Gaussians carry the classes `leaves`, shuffled; decay: means N(0, 1) / (1 + n)^2 per
    cepstral index n, the envelope of real cepstra"""
    rng = np.random.default_rng(seed); G = int(sum(leafSizes)); D = L * nSub
    m = T.random_model(ref_ns(G), D, seed)
    if decay:
        m.mean = (rng.standard_normal((G, nSub, L)) / (1.0 + np.arange(L))[None, None, :] ** 2).reshape(G, D).astype(f32)
    classes = rng.permutation(np.concatenate([np.full(n, l, np.uint16) for n, l in zip(leafSizes, leaves)]))
    return m, classes


def stats(m, S, seed, mmi=True):
    """per speaker counts with exact zeros (whose sumO is not zero), counts that round to float zero, and negative counts (MMI)"""
    rng = np.random.default_rng(seed); c = rng.uniform(0.5, 30.0, (S, m.G))
    if mmi:
        kind = rng.random((S, m.G))
        c[kind < 0.10] = 0.0; c[(kind >= 0.10) & (kind < 0.13)] = 1.0e-50; c[(kind >= 0.13) & (kind < 0.22)] *= -1.0
    sumO = c[:, :, None] * (m.mean[None].astype(np.float64) + 0.3 * rng.standard_normal((S, m.G, m.D)))
    sumO[c == 0.0] = 1.0
    return c, sumO


def recovery_stats(kind, m, L, nSub, alpha, seed):
    """sumO = c float(A(alpha) mu) with the kind's own matrix and no bias: the statistics of a speaker whose means are the model's under alpha"""
    rng = np.random.default_rng(seed); c = rng.uniform(0.5, 30.0, m.G)
    warped = P.transform(P.matrix(kind, [alpha], L), m.mean, nSub)
    return c, c[:, None] * warped.astype(np.float64)


def recovery_bound(alpha):
    """Brent's method stops when the bracket around x is at most 2 tol2 = 4 tol1 wide, tol1 = Tolerance |x| + ZEpsilon (eA:199-200)"""
    return 4.0 * (0.01 * abs(alpha) + 1.0e-10)
