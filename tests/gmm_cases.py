"""Inputs shared by tests/test_gmm_cases_cpu.py and tests/test_gpu_gmm_shapes.py: model families for mode 2 of dsr_gmm_score (the expanded quadratic on
the matrix cores, csrc/k_gmm_mfma.hip), frames placed where two Gaussians of one codebook are (nearly) equally far, a numpy emulation of the expanded
form's fp32 arithmetic, the rounding bound of the kernel's header, and the lists of shapes the GPU tests run.

Random models with random frames say little about mode 2's trust test: a (frame, codebook) whose two best distances differ by less than the expanded
form's rounding error turns up once in 1e5.  The frames of near_tie_frames sit on such ties by construction, so a kernel that fails to flag or to
re-score one picks the wrong Gaussian on every second frame (test_gmm_cases_cpu.py measures that share on the inputs themselves)."""
import numpy as np

from tests import synth

# name: (mu0, sigma, every (frame, codebook) is re-scored exactly).  Means mu0 + 2 sigma N(0, 1), inverse variances 1 / (sigma U(0.7, 1.4))^2 as in
# test_gmm_mfma_mode_offset_means, det = -sum log ivar as in synth.gmm_model.  What a family is for:
#   unit      distances positive, S = 2 ivMax |x|^2 + termMax a few times the distance
#   offset    the rounding bound is a visible fraction of the distance
#   far       the cancelled terms are ~1e6 times the distance: the trust test sends everything to the exact re-score, scores are mode 0's bits
#             (best_over_S states that as a condition on the frames; test_gmm_cases_cpu.py and the GPU tests assert it of theirs)
#   negative  pi + det = dimN (1.84 + 2 log sigma) is far below zero and the quadratic part of a frame between two means (~2.3 dimN) does not make up
#             for it: the distances the search compares are NEGATIVE floats (an index in the low mantissa bits orders those the other way round)
#   straddle  the same with the two parts about equal: distances of both signs and |d| below the kernel's "bound no longer small against d" test
# (The quadratic part does not depend on sigma -- means and frames scale with it -- so the sign is set by 2 log sigma alone: sigma = 0.3 or 0.6 would
# still give positive distances with means two sigma apart; test_gmm_cases_cpu.py asserts the signs each family is here for.)
FAMILIES = {
    "unit": (0.0, 1.0, False),
    "offset": (5.0, 0.5, False),
    "far": (50.0, 0.1, True),
    "negative": (0.0, 0.003, False),
    "straddle": (0.0, 0.125, False),
}
FAMILY_NAMES = list(FAMILIES)


def model(family, K, R, D, seed=3, refN=None):
    """-> dict(refN, mean, ivar, det, val) of family `family`: K codebooks of R Gaussians, or of refN[k] Gaussians when refN is given"""
    mu0, sigma, _ = FAMILIES[family]
    rng = np.random.default_rng(1000 * seed + 7 * D + R)
    if refN is None:
        m = synth.gmm_model(K, R, D, seed=seed)
    else:
        refN = np.asarray(refN, np.int32)
        w = np.concatenate([rng.dirichlet(np.ones(n)) for n in refN])
        m = dict(refN=refN, val=(-np.log(w)).astype(np.float32))
    G = int(np.sum(m["refN"]))
    m["mean"] = (mu0 + sigma * rng.standard_normal((G, D)) * 2.0).astype(np.float32)
    m["ivar"] = (1.0 / (sigma * rng.uniform(0.7, 1.4, (G, D))) ** 2).astype(np.float32)
    m["det"] = (-np.log(m["ivar"].astype(np.float64)).sum(1)).astype(np.float32)
    return m


def plain_frames(family, N, D, seed):
    mu0, sigma, _ = FAMILIES[family]
    return (mu0 + sigma * 2.0 * np.random.default_rng(seed).standard_normal((N, D))).astype(np.float32)


def _cst(m):
    """float _pi + float det of every Gaussian (codebookBasic.cc:170, :481), as float64"""
    D = m["mean"].shape[1]
    return (np.float32(np.log(2.0 * np.pi) * D) + m["det"].astype(np.float32)).astype(np.float64)


def trust_terms(m):
    """(ivMax, termMax) of gmm_prepare_mfma in float64: S = 2 ivMax |x|^2 + termMax bounds the sum of the magnitudes of the expanded form's terms"""
    mu = m["mean"].astype(np.float64); iv = m["ivar"].astype(np.float64)
    return float(np.abs(iv).max()), float((2.0 * np.abs(mu * mu * iv).sum(1) + np.abs(_cst(m))).max())


def frame_S(m, x):
    """S of every frame, float64 [N]"""
    ivMax, termMax = trust_terms(m)
    x = np.asarray(x, np.float64)
    return 2.0 * ivMax * (x * x).sum(1) + termMax


def score_bound(m, x, scale=None):
    """[N][K] float64: the header's bound on |mode 2 score - mode 0 score| where the two are not the same bits: half (score = 0.5 (d + 2 val)) the
    distance bound (n + 2) 2^-24 S, n = 2 dimN + 1, times the codebook's scale"""
    D = m["mean"].shape[1]; K = len(m["refN"])
    sc = np.ones(K) if scale is None else np.abs(np.asarray(scale, np.float64))
    return 0.5 * (2 * D + 3) * 2.0 ** -24 * frame_S(m, x)[:, None] * sc[None, :]


def dist64(m, x, g):
    """float64 distances of frames x [N][D] to Gaussians g [N] or [N][r] (one row of Gaussians per frame)"""
    mu = m["mean"].astype(np.float64)[g]; iv = m["ivar"].astype(np.float64)[g]
    xx = np.asarray(x, np.float64)
    if mu.ndim == 3:
        xx = xx[:, None, :]
    return _cst(m)[g] + ((mu - xx) ** 2 * iv).sum(-1)


def best_over_S(m, x):
    """max over (frame, codebook) of |the codebook's nearest float64 distance| / S.  The kernels re-score a (frame, codebook) whatever its two
    best are once the bound is no longer small against the distance: r0 S > 1e-3 |d|, r0 >= 1e-5 the untagged trust radius -- so a value below
    1e-2 here (asked with a factor ten to spare: the kernels test their own computed d) means every entry of these frames is re-scored"""
    refN = np.asarray(m["refN"], np.int64); off = np.concatenate([[0], np.cumsum(refN)])
    N, G = len(x), int(off[-1])
    d = np.empty((N, G))
    for g0 in range(0, G, 32):
        g = np.arange(g0, min(G, g0 + 32))
        d[:, g] = dist64(m, x, np.tile(g, (N, 1)))
    return float((np.abs(np.minimum.reduceat(d, off[:-1], axis=1)) / frame_S(m, x)[:, None]).max())


def near_tie_frames(m, N, seed, spread=0.3, max_step=1.0):
    """-> (x float32 [N][D], info dict(k, a, b [N] int: codebook and the two placed Gaussians (indices inside the codebook), g [N]: the float64 gap
    |d_a - d_b| / S the frame was placed at, before its rounding to fp32)).

    Per frame: a codebook k and two of its Gaussians a != b; the line mu_a -> mu_b shifted by `spread` sigma per dimension; the point on it where
    the two float64 distances (pi + det included) are equal, found by bisection; then a step off the bisector that opens the gap to g S, g
    log-uniform in [1e-9, 1e-3] (a fifth of the frames stay on the bisector, g = 0); rounded to fp32.  The step is at most `max_step` times the
    way from mu_a to mu_b, g cut down to what that opens: where the cancelled terms are 1e6 times the distance ('far': S ~ 3e7, the gap grows
    by ~250 per mean-to-mean step) a gap of 1e-3 S lies a hundred such steps out, at a distance of ~2e6 from everything -- no near tie, and no
    longer a frame whose every codebook is re-scored, which is what that family is for.  The other families never reach the limit (their
    frames are the same with and without it), and no g <= 1e-5 does in any.  Candidates whose line does not cross the
    bisector between the two means, or where a third Gaussian of the codebook is nearer than the placed pair (in float64), are drawn again: at
    small dimN and 8+ Gaussians a codebook a random pair's midpoint is often nearer to a third."""
    rng = np.random.default_rng(seed)
    refN = np.asarray(m["refN"], np.int64); off = np.concatenate([[0], np.cumsum(refN)])
    mu = m["mean"].astype(np.float64); iv = m["ivar"].astype(np.float64)
    D = mu.shape[1]
    ok_k = np.nonzero(refN >= 2)[0]
    xs, ks, as_, bs, gs = [], [], [], [], []
    have = 0
    for rnd in range(200):
        if have >= N:
            break
        M = 64 + int((1.3 + 0.5 * rnd) * (N - have))                                  # (more when few were accepted)
        k = ok_k[rng.integers(0, len(ok_k), M)]
        a = rng.integers(0, refN[k]); b = (a + 1 + rng.integers(0, refN[k] - 1)) % refN[k]
        ga, gb = off[k] + a, off[k] + b
        o = spread * rng.standard_normal((M, D)) / np.sqrt(iv[ga])
        p0 = mu[ga] + o; dirv = mu[gb] - mu[ga]
        f = lambda t: dist64(m, p0 + t[:, None] * dirv, ga) - dist64(m, p0 + t[:, None] * dirv, gb)
        lo, hi = np.zeros(M), np.ones(M)
        keep = (f(lo) < 0) & (f(hi) > 0)
        for _ in range(56):
            mid = 0.5 * (lo + hi); neg = f(mid) < 0
            lo = np.where(neg, mid, lo); hi = np.where(neg, hi, mid)
        t0 = 0.5 * (lo + hi)
        x0 = p0 + t0[:, None] * dirv
        # the gap: f is smooth in t, its slope at t0 from a central difference
        h = 1e-6; slope = (f(t0 + h) - f(t0 - h)) / (2 * h)
        g = np.exp(rng.uniform(np.log(1e-9), np.log(1e-3), M)); g[rng.random(M) < 0.2] = 0.0
        sgn = np.where(rng.random(M) < 0.5, -1.0, 1.0)
        keep &= slope > 0
        unit = frame_S(m, x0) / np.where(slope > 0, slope, 1.0)                           # the step in t that opens a gap of S
        g = np.minimum(g, max_step / unit)
        t1 = t0 + sgn * g * unit
        x = (p0 + t1[:, None] * dirv).astype(np.float32)
        # the placed pair must be the codebook's two nearest
        Rmax = int(refN.max())
        idx = off[k][:, None] + np.minimum(np.arange(Rmax)[None, :], refN[k][:, None] - 1)       # (short codebooks repeat their last Gaussian)
        dall = dist64(m, x, idx)
        pair = np.maximum(dist64(m, x, ga), dist64(m, x, gb))
        others = (np.arange(Rmax)[None, :] != a[:, None]) & (np.arange(Rmax)[None, :] != b[:, None]) & (np.arange(Rmax)[None, :] < refN[k][:, None])
        keep &= ~((dall < pair[:, None]) & others).any(1)
        sel = np.nonzero(keep)[0][:N - have]
        xs.append(x[sel]); ks.append(k[sel]); as_.append(a[sel]); bs.append(b[sel]); gs.append(g[sel]); have += len(sel)
    assert have >= N, "near_tie_frames: %d of %d frames placed" % (have, N)
    return np.concatenate(xs), dict(k=np.concatenate(ks), a=np.concatenate(as_), b=np.concatenate(bs), g=np.concatenate(gs))


def frames(family, m, N, seed):
    """-> (x float32 [N][D], tie [N] bool, info of the near-tie frames in their order): half near ties (the larger half), half plain, mixed so that
    every tile of a kernel sees both"""
    D = m["mean"].shape[1]
    nt = (N + 1) // 2
    xt, info = near_tie_frames(m, nt, seed)
    x = np.concatenate([xt, plain_frames(family, N - nt, D, seed + 1)])
    perm = np.random.default_rng(seed + 2).permutation(N)
    tie = np.zeros(N, bool); tie[:nt] = True
    info = dict(info, row=np.argsort(perm)[:nt])                              # where near-tie frame i went
    return np.ascontiguousarray(x[perm]), tie[perm], info


def emulate_expanded(m, x, g):
    """fp32 emulation of the expanded form with gmm_prepare_mfma's operands, for frames x [N][D] and Gaussians g [N][r]: A = (iv, -2 mu iv, c),
    B = (x^2, x, 1), one fused multiply-add per k in k order from 0 (the product exact in float64, the sum rounded to fp32) -> float32 [N][r]"""
    mu = m["mean"].astype(np.float64)[g]; iv = m["ivar"].astype(np.float64)[g]                # [N][r][D]
    D = mu.shape[-1]
    c = _cst(m)[g].copy()
    for d in range(D):
        c += mu[..., d] * mu[..., d] * iv[..., d]
    A = np.concatenate([iv.astype(np.float32), (-2.0 * mu * iv).astype(np.float32), c.astype(np.float32)[..., None]], -1).astype(np.float64)
    x = np.asarray(x, np.float32)
    B = np.concatenate([x * x, x, np.ones((x.shape[0], 1), np.float32)], 1).astype(np.float64)[:, None, :]
    acc = np.zeros(A.shape[:2], np.float32)
    for k in range(2 * D + 1):
        acc = (acc.astype(np.float64) + A[..., k] * B[..., k]).astype(np.float32)
    return acc


# ---- the shapes of tests/test_gpu_gmm_shapes.py (test_gmm_cases_cpu.py checks the near-tie inputs of every (family, D, R) among them)
DEPTH_D = [15, 16, 18, 19, 20, 35, 36, 39, 40, 44, 47, 48, 64]        # both sides of every boundary of the contraction-depth table, and inside
WIDE_R = [(8, 37), (16, 21), (32, 11)]                                  # (R, K): K R <= 600, the last 32-row chunk not filled
WIDE_D_REG = [18, 20, 44, 64]                                           # depths k_gmm_sp.hip has no instantiation for at R >= 8
WIDE_D_SP = [13, 39]                                                    # the two it has


def tie_shapes():
    """every (family, D, R) a GPU test draws near-tie frames for at uniform codebook size"""
    s = [(f, D, 4) for D in DEPTH_D for f in FAMILY_NAMES]
    s += [(f, D, R) for R, _ in WIDE_R for D in WIDE_D_REG + WIDE_D_SP for f in FAMILY_NAMES]
    s += [("far", 5, 4)]                                                # (the large models of the GPU file)
    return s
