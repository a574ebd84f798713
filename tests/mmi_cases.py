"""The SubbandMMI cases past one bin per thread (tests/test_gpu_mmi_shapes.py) and the conditions on their inputs (tests/test_mmi_cpu.py).

k_mmi (csrc/k_mmi.hip) is one workgroup of 256 threads per utterance, a thread striding over the bins; the cases of tests/test_gpu_mmi.py have
at most 17 bins.  These have 257, 512 and 1262.  Set-up, inputs and tolerance are those of tests/test_gpu_mmi.py (its _make and TOL); a case
carries its own seed, chosen so that the mask strikes some of the bins from 256 on and spares others (test_mmi_cpu.py asserts it)."""
import functools

import numpy as np

from tests.test_gpu_mmi import TOL, _make  # noqa: F401  (the same set-up calls and tolerance as the small cases)

T_FRAMES = 6

# M, C, hbs, target, nSource, pfType, alpha, NC, mask (avgFactor, fwidth, type), seed, T, U
CASES = [
    (512, 16, False, 0, 2, 0x02, 0.7, 1, (0.6, 3, 0), 701, T_FRAMES, 3),     # 1  F = 257: thread 0 owns bins 0 and 256; wide mask; the last register-resident channel count
    (512, 17, False, 1, 3, 0x02, 0.7, 2, (0.5, 4, 1), 702, T_FRAMES, 3),     # 2  the first taScr channel count; mask type 1 (two density updates of the target a frame); calcWeightsN
    (512, 16, True, 0, 2, 0x04, 0.7, 1, (0.6, 1, 0), 703, T_FRAMES, 3),      # 3  F = 512, two bins a thread; APAB mirrored weights read bin M-1-f across the 256 boundary
    (512, 17, True, 0, 2, 0x02, 0.7, 1, (0.6, 3, 0), 704, T_FRAMES, 3),      # 4  wide mask with f1 = M - 1
    (512, 4, False, 0, 2, 0x04, 0.7, 1, (0.6, 3, 0), 705, T_FRAMES, 3),      # 5  APAB without halfBandShift: Fout = 512 > F, mirror-bin writes M - f from threads on their second bin
    (512, 4, False, 0, 2, 0x0A, 0.8, 1, None, 706, T_FRAMES, 3),             # 6  TYPE_ZELINSKI2, no mask, at F = 257
    (1262, 4, True, 0, 2, 0x02, 0.7, 1, (0.6, 3, 0), 707, 3, 2),             # 7  52 F = 65 624 bytes of LDS, the first size above 64 KiB
]
IDS = ["%d-M%d-C%d%s-pf%02x" % (i + 1, c[0], c[1], "-hbs" if c[2] else "", c[5]) for i, c in enumerate(CASES)]
MASKED = [i for i, c in enumerate(CASES) if c[8] is not None]


def bins(case):
    """(bins a snapshot has, bins an output frame has)"""
    M, hbs, pfType = case[0], case[2], case[5]
    F = M if hbs else M // 2 + 1
    return F, (M if (hbs or (pfType & 0x04)) else F)


def make(kind, case, mask="own"):
    """the product's object ('dsr') or the oracle's ('orc') of a case; mask: the case's own, or another (None: no mask)"""
    M, Cn, hbs, target, nSource, pfType, alpha, NC, own, seed = case[:10]
    return _make(kind, M, Cn, hbs, target, nSource, pfType, alpha, NC, seed, own if mask == "own" else mask)


def nframes(case):
    T, U = case[10], case[11]
    return np.array([T, T - 2, 1][:U], np.int32)


def snapshots(case, U=None):
    """X [U][C][T][F] complex64, drawn as tests/test_gpu_mmi.py draws them"""
    M, Cn, pfType, seed, T = case[0], case[1], case[5], case[9], case[10]
    U = case[11] if U is None else U
    F = bins(case)[0]
    rng = np.random.default_rng(seed + 1)
    X = (rng.standard_normal((U, Cn, T, F)) + 1j * rng.standard_normal((U, Cn, T, F))).astype(np.complex64)
    X *= (0.2 + rng.random((U, 1, T, F)) * 2.0).astype(np.float32)
    if pfType & 0x04:                                                          # APAB: the reference channel loud in half of the points, so that weights below 1 occur
        X[:, Cn // 2] *= np.where(rng.random((U, T, F)) < 0.5, 8.0, 1.0).astype(np.float32)
    return X


def oracle_run(case, Xu, mask="own"):
    """a fresh oracle object over the frames of one utterance [C][T][F] -> [T][outBins] complex128"""
    return make("orc", case, mask).run(Xu.astype(np.complex128))[:, :bins(case)[1]]


@functools.lru_cache(maxsize=None)
def reference(i):
    """(X, nframes, [U] oracle outputs over each utterance's own frames) of CASES[i], computed once"""
    case = CASES[i]
    X = snapshots(case); nfr = nframes(case)
    return X, nfr, [oracle_run(case, X[u, :, :nfr[u], :]) for u in range(X.shape[0])]


def check(case, Y, X, nfr, refs):
    """the assertions of test_subband_mmi_apply on a batch; -> the largest error relative to TOL"""
    worst = 0.0
    for u in range(X.shape[0]):
        ref = refs[u]; got = Y[u, :nfr[u]]
        scale = np.maximum(1e-30, np.abs(ref).max(axis=1, keepdims=True))
        err = (np.abs(got - ref) / scale).max()
        worst = max(worst, err / TOL)
        assert err <= TOL, (u, err)
        assert np.all(Y[u, nfr[u]:] == 0)
    return worst
