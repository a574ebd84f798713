"""The inputs of the speaker-adaptive training tests (tests/test_sat_np_cpu.py, tests/test_gpu_sat.py).

The full-rank recipe: mu* ~ N(0, 1), iv ~ U[0.5, 2] as float, A_s = I + 0.1 N(0, 1) / sqrt(bl) per block, b_s = 0.3 N(0, 1), c ~ U[5, 50] as
float, sumO = c (A_s mu* + b_s), the current mean float(mu* + 0.5 N(0, 1)), sumOsq = c (sigma^2 + (A_s mu* + b_s)^2).  On it the smallest kept
sigma_k / sigma_0 is >= 0.2 over D in {1, 3, 13, 16, 39, 40} x S in {1, 3}, LAPACK recovers mu* to <= 3e-14 and auxNew <= auxOld always
(test_sat_np_cpu.py checks all three), so the 1e-7 rule and the accept test are never near a tie.  The rank-deficient case has one speaker
whose A has its last k rows zero: the dropped ratios are <= 1e-16 and the kept ones >= 0.2."""
import numpy as np

from tests import sat_np as N
from tests import train_np as T

f32, f64 = np.float32, np.float64
RECIPE_D = [1, 3, 13, 16, 39, 40]
RECIPE_S = [1, 3]
DEFICIENT = [(3, 1), (13, 4), (39, 13)]                      # (D, zero rows)

# the device cases: dimN, blocks, the tree's leaves, Gaussians per leaf, slots of the first batch, how the transforms reach the handle.
# Gaussians per class: one, fewer than a 16-row tile, around four tiles (63, 64, 65), more (130); S = 17 is more than one wave's k-steps
# at bl = 1 and an odd count; every case runs a second batch of two slots.
GPU_CASES = [
    dict(D=1, nB=1, leaves=[1], sizes=[5], S=1, path="raw"),
    dict(D=3, nB=1, leaves=[2, 3], sizes=[1, 63], S=3, path="tree"),
    dict(D=15, nB=1, leaves=[4, 5, 3], sizes=[64, 65, 5], S=3, path="tree"),
    dict(D=16, nB=1, leaves=[1], sizes=[130], S=17, path="raw"),
    dict(D=39, nB=1, leaves=[2, 3], sizes=[65, 130], S=3, path="tree"),
    dict(D=40, nB=1, leaves=[4, 5, 3], sizes=[1, 64, 63], S=1, path="raw"),
    dict(D=39, nB=3, leaves=[2, 3], sizes=[63, 5], S=3, path="apt"),
    dict(D=32, nB=2, leaves=[4, 5, 3], sizes=[5, 64, 1], S=17, path="apt"),
    dict(D=39, nB=3, leaves=[1], sizes=[65], S=3, path="raw"),
    dict(D=32, nB=2, leaves=[2, 3], sizes=[130, 5], S=1, path="raw"),
    dict(D=81, nB=1, leaves=[1], sizes=[3], S=1, path="raw"),                # the largest block the kernels take: the LDS opt-in of the solve
]
APT_ALPHAS = [-0.3, -0.12, 0.05, 0.2, 0.31]                  # the BLT parameter of a (slot, class), by index


def ref_ns(G, most=50):
    r = [most] * (G // most)
    if G % most:
        r.append(G % most)
    return r


def model(D, sizes, leaves, seed, refN=None):
    """a random model (tests.train_np.Model) whose Gaussians carry the classes `leaves`, shuffled; cv holds inverse variances in [0.5, 2]"""
    rng = np.random.default_rng(seed); G = int(sum(sizes))
    m = T.random_model(refN or ref_ns(G), D, seed)
    classes = rng.permutation(np.concatenate([np.full(n, l, np.uint16) for n, l in zip(sizes, leaves)]))
    return m, classes


def recipe_transform(rng, D, nB, zeroRows=0):
    bl = D // nB
    A_ = np.stack([np.eye(bl) + 0.1 * rng.standard_normal((bl, bl)) / np.sqrt(bl) for _ in range(nB)])
    if zeroRows:
        A_[:, bl - zeroRows:, :] = 0.0
    return A_, 0.3 * rng.standard_normal(D)


def apply_blocks(A_, b, mu):
    """A mu + b in double, block by block: rows [G][D]"""
    nB, bl = A_.shape[0], A_.shape[1]
    y = np.concatenate([mu[:, nb * bl:(nb + 1) * bl] @ A_[nb].T for nb in range(nB)], axis=1)
    return y + b[None, :]


class Problem(object):
    """the recipe for one model: mu*, sigma^2, iv, the current mean, and S speakers each with one (A, b) per class"""

    def __init__(self, D, nB, leaves, sizes, S, seed, deficient=0, kind=N.MLLR, transforms=None, refN=None):
        rng = np.random.default_rng(seed); self.D, self.nB, self.leaves, self.S = D, nB, list(leaves), S
        self.m, self.classes = model(D, sizes, leaves, seed, refN); G = self.m.G; self.G = G
        self.muStar = rng.standard_normal((G, D)).astype(f32).astype(f64)                        # a float, so that a model can hold it
        self.sigma2 = rng.uniform(0.5, 2.0, (G, D))
        self.m.mean = (self.muStar + 0.5 * rng.standard_normal((G, D))).astype(f32)
        self.xf, self.c, self.sumO, self.sumOsq, self.y = [], [], [], [], []
        for s in range(S):
            xf = {}; y = np.zeros((G, D))
            for rc in self.leaves:
                if transforms is not None:
                    x = transforms(s, rc)
                else:
                    A_, b = recipe_transform(rng, D, nB, deficient if s == 0 else 0); x = N.Xform(kind, A_, b)
                xf[rc] = x; sel = self.classes == rc
                y[sel] = apply_blocks(x.A, x.b, self.muStar[sel])
            c = rng.uniform(5.0, 50.0, G).astype(f32).astype(f64)
            self.xf.append(xf); self.c.append(c); self.sumO.append(c[:, None] * y); self.sumOsq.append(c[:, None] * (self.sigma2 + y * y)); self.y.append(y)

    def mean_accus(self, dtype=f64, slots=None):
        a = N.MeanAccus(self.G, self.D, dtype)
        for s in (range(self.S) if slots is None else slots):
            a.accumulate(self.classes, self.m.cv, self.c[s], self.sumO[s], self.xf[s])
        return a
