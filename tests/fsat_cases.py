"""The inputs of the fast speaker-adaptive training tests (tests/test_fsat_np_cpu.py, tests/test_gpu_fsat.py), built on the recipe of
tests/sat_cases.py.  test_fsat_np_cpu.py checks, for every solve case below, that the restatement's decisions are far from every tie
(tests.fsat_np.conditions): the GPU tests compare decisions only under those conditions."""
import numpy as np

from tests import apt_np as P
from tests import fsat_np as F
from tests import sat_cases as Cs
from tests import sat_np as N

f32, f64 = np.float32, np.float64
APT_RAPT = 1                                                   # dsr._capi.APT_RAPT (include/dsr.h section 13)

# k_fsat_norm: dimN 1, 3, 16, 39 as one MLLR block and 13 x 3 blocks through the APT path; 1, 15, 16, 17 and 130 Gaussians in a class (one
# Gaussian, one short of a 16-row tile, a tile, a tile and one, more than eight tiles); the trees {1}, {2, 3}, {4, 5, 3}; 1, 3 and 17 slots
# in the first batch; every case runs a second batch of two slots into the same accumulators
NORM_CASES = [
    dict(D=1, nB=1, leaves=[1], sizes=[1], S=1, path="raw"),
    dict(D=3, nB=1, leaves=[2, 3], sizes=[15, 16], S=3, path="tree"),
    dict(D=16, nB=1, leaves=[4, 5, 3], sizes=[17, 1, 130], S=17, path="raw"),
    dict(D=39, nB=1, leaves=[2, 3], sizes=[16, 17], S=3, path="tree"),
    dict(D=39, nB=3, leaves=[2, 3], sizes=[15, 17], S=3, path="apt"),
]


def _apt_transforms(ci, D, nB):
    L = D // nB

    def tf(s, rc):
        a = Cs.APT_ALPHAS[(3 * s + rc) % len(Cs.APT_ALPHAS)]; nb = (0, L, D)[(s + ci) % 3]
        bias = (0.3 * np.random.default_rng(1000 * s + rc).standard_normal(nb)).astype(f32)
        return N.apt_xform(P.matrix(APT_RAPT, [a], L), nB, bias)
    return tf


def apt_params(ci, p, s, rc):
    """what _apt_transforms made of (s, rc), as the parameters an Apt handle takes: (alpha, bias)"""
    L = p.D // p.nB; nb = (0, L, p.D)[(s + ci) % 3]
    return Cs.APT_ALPHAS[(3 * s + rc) % len(Cs.APT_ALPHAS)], (0.3 * np.random.default_rng(1000 * s + rc).standard_normal(nb)).astype(f32)


def with_counts(p, seed, special=True):
    """numProb and denProb for every speaker of a sat_cases.Problem: den is zero for most Gaussians and a float in [0, 3] for a third of them,
    num = c + den rounded to float.  special: in speaker 0, Gaussian 0 has no count at all (cfs:348), the last one |ck| < 1e-6 (counts are
    added, nothing else, cfs:368) and the middle one a negative ck"""
    rng = np.random.default_rng(seed); p.num, p.den = [], []
    for s in range(p.S):
        den = np.where(rng.uniform(size=p.G) < 1.0 / 3.0, rng.uniform(0.0, 3.0, p.G), 0.0).astype(f32).astype(f64)
        num = (p.c[s] + den).astype(f32).astype(f64)
        if special and s == 0:
            num[0] = den[0] = 0.0
            if p.G > 1:
                num[-1] = 5.0; den[-1] = 5.0 - 2.0 ** -22
            if p.G > 2:
                num[p.G // 2] = 1.0; den[p.G // 2] = 9.0
        p.num.append(num); p.den.append(den)
    return p


def norm_problem(ci):
    """the recipe for NORM_CASES[ci] with S + 2 speakers: the first batch takes S, the second two"""
    case = NORM_CASES[ci]; D, nB, S = case["D"], case["nB"], case["S"]
    tf = _apt_transforms(ci, D, nB) if case["path"] == "apt" else None
    return with_counts(Cs.Problem(D, nB, case["leaves"], case["sizes"], S + 2, seed=500 + ci, transforms=tf), 600 + ci)


def fold(p, slots=None, fast=None):
    """the restatement's fast accumulators after the speakers `slots` of the problem, in order"""
    fast = F.FastAccus(p.G, p.D, p.nB) if fast is None else fast
    for s in (range(p.S) if slots is None else slots):
        fast.norm(p.classes, p.m.mean, p.m.cv, p.num[s], p.den[s], p.sumO[s], p.sumOsq[s], p.xf[s])
    return fast


def sums(p, fast, dtype=f64, slots=None):
    """the restatement's SAT sums: add_fast, then the matrix-only accumulate of every speaker with c = num - den"""
    a = F.SatSums(p.G, p.D, dtype); a.add_fast(fast)
    for s in (range(p.S) if slots is None else slots):
        a.accumulate(p.classes, p.m.cv, p.num[s] - p.den[s], p.xf[s])
    return a


# the solve: thr 0 keeps every direction of the full-rank recipe; "some" is a threshold in the widest gap of the middle of all contributions
# 0.5 t^2 / l (drops some directions of most blocks, never near one); "all" is ten times the largest contribution.  mean "optimum": the model
# starts at the float of the thr = 0 solution, so that with descLen = 1 every block keeps its old mean and with descLen = bl (what a first
# iteration at thr = 0 leaves) the dropped directions pay for themselves and the block is updated: the descLen penalty changes the decision
SOLVE_CASES = [
    dict(name="full13", D=13, nB=1, leaves=[2, 3], sizes=[5, 4], S=3, thr=0.0, kind=N.MLLR),
    dict(name="full3x13", D=39, nB=3, leaves=[1], sizes=[4], S=3, thr=0.0, kind=N.APT),
    dict(name="full1", D=1, nB=1, leaves=[1], sizes=[3], S=1, thr=0.0, kind=N.MLLR),
    dict(name="some13", D=13, nB=1, leaves=[2, 3], sizes=[5, 4], S=3, thr="some", kind=N.MLLR),
    dict(name="some3x13", D=39, nB=3, leaves=[1], sizes=[4], S=3, thr="some", kind=N.APT),
    dict(name="all13", D=13, nB=1, leaves=[1], sizes=[5], S=3, thr="all", kind=N.MLLR),
    dict(name="second1", D=13, nB=1, leaves=[2, 3], sizes=[5, 4], S=3, thr="some", kind=N.MLLR, mean="optimum", descLen=1),
    dict(name="secondbl", D=13, nB=1, leaves=[2, 3], sizes=[5, 4], S=3, thr="some", kind=N.MLLR, mean="optimum", descLen=13),
]
MASS = 1.0                                                     # the mass threshold of the solve cases: every Gaussian of the recipe passes


def _contribs(a):
    out = []
    for g in range(a.G):
        for nb in range(a.a.nB):
            s = F.mdl_solve(np.asarray(a.a.mat[g, nb], f64), np.asarray(a.a.vec[g, nb], f64), 0.0); out += list(s["contrib"])
    return np.sort(np.asarray(out))


def pick_threshold(contribs, how):
    if how == "all":
        return 10.0 * float(contribs.max())
    c = contribs[int(0.3 * len(contribs)):int(0.7 * len(contribs)) + 1]; k = int(np.argmax(c[1:] / c[:-1]))
    return float(np.sqrt(c[k] * c[k + 1]))


def solve_problem(si):
    """-> dict(p, fast, sums, thr, descLen [G][nB]) for SOLVE_CASES[si]: the restatement's accumulators over all speakers of the problem"""
    case = SOLVE_CASES[si]
    p = with_counts(Cs.Problem(case["D"], case["nB"], case["leaves"], case["sizes"], case["S"], seed=700 + case["D"] + case["nB"], kind=case["kind"]), 800 + si, special=False)
    fast = fold(p); a = sums(p, fast)
    if case.get("mean") == "optimum":
        for g in range(p.G):
            for nb in range(p.nB):
                bl = p.D // p.nB; p.m.mean[g, nb * bl:(nb + 1) * bl] = F.mdl_solve(a.a.mat[g, nb], a.a.vec[g, nb], 0.0)["x"].astype(f32)
        fast = fold(p); a = sums(p, fast)                                                        # fastVar follows the mean the model holds
    thr = case["thr"] if not isinstance(case["thr"], str) else pick_threshold(_contribs(a), case["thr"])
    descLen = np.full((p.G, p.nB), case.get("descLen", 1), np.uint16)
    return dict(p=p, fast=fast, sums=a, thr=thr, descLen=descLen)


def restated_update(q, massThreshold=MASS, meanOnly=False, skip=()):
    """tests.fsat_np.update on the restatement's own sums of a solve_problem / branch_problem"""
    p, a = q["p"], q["sums"]
    return F.update(a.a.mat, a.a.vec, a.a.scalar, a.a.occ, a.a.has, a.varVec, p.m.mean, p.m.cv, q["descLen"], q["thr"], massThreshold, meanOnly, skip=skip)


def branch_problem():
    """D = 3, six Gaussians, two speakers.  0: occ 7, below a mass threshold of 10; 1: counts +5 and -5, occ == 0; 2: never a count (no
    fast statistics either, but add_fast allocates its blocks); 3: counts 30 and -15 under A = 0.1 I and I: an indefinite matrix, the old mean
    is kept; 4: plain here -- the GPU test makes its fastMean infinite through set_fast; 5: plain"""
    D = 3; p = Cs.Problem(D, 1, [1], [6], 2, seed=5)
    p.c[0][:] = [4.0, 5.0, 0.0, 30.0, 20.0, 20.0]; p.c[1][:] = [3.0, -5.0, 0.0, -15.0, 9.0, 9.0]
    p.xf[0][1] = N.Xform(N.MLLR, 0.1 * np.eye(D), np.zeros(D)); p.xf[1][1] = N.Xform(N.MLLR, np.eye(D), np.zeros(D))
    p.num = [np.where(c > 0, c, 0.0) for c in p.c]; p.den = [np.where(c < 0, -c, 0.0) for c in p.c]
    fast = fold(p); a = sums(p, fast)
    return dict(p=p, fast=fast, sums=a, thr=0.0, descLen=np.ones((p.G, 1), np.uint16))
