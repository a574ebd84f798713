"""Inputs shared by tests/test_gcc_np_cpu.py and tests/test_gpu_gcc.py: synthetic array spectra, speech / noise patterns, the case list of
the GPU comparison, and the rule that says which frames the peak-index and interpolation comparisons may leave out."""
import numpy as np

from tests import gcc_np as G

SR = 16000.0


def array_frames(seed, U, C, T, N, noise=0.1):
    """[U][C][T][N] Hann-windowed frames (hop N/2) of one white source reaching channel c after (3c mod 7) - 3 samples, plus own noise"""
    r = np.random.default_rng(seed)
    hop = N // 2; L = (T - 1) * hop + N + 16
    w = G.hann(N)
    out = np.zeros((U, C, T, N))
    for u in range(U):
        s = r.standard_normal(L + 16)
        for c in range(C):
            d = (3 * c) % 7 - 3
            x = s[8 - d:8 - d + L] + noise * r.standard_normal(L)
            for t in range(T):
                out[u, c, t] = w * x[t * hop:t * hop + N]
    return out


def spectra(seed, U, C, T, N, noise=0.1):
    return np.fft.rfft(array_frames(seed, U, C, T, N, noise), axis=-1)


def star(C):
    return [(0, c) for c in range(1, C)]


def all_pairs(C):
    return [(a, b) for a in range(C) for b in range(a + 1, C)]


def sad_pattern(name, U, T):
    """-> (sad [U][T] int32, timestamps [U][T])"""
    sad = np.ones((U, T), np.int32); ts = np.tile(0.01 * (1 + np.arange(T)), (U, 1))
    if name == "lead":                       # a noise lead-in and noise stretches in mid-utterance
        sad[:, :3] = 0; sad[:, T // 2:T // 2 + 2] = 0
        if T > 8:
            sad[:, T - 3] = 0
    elif name == "speech_first":             # speech before any noise, noise later
        sad[:, 2:4] = 0
    elif name == "ts0":                      # the first (noise) frame is stamped 0.0: the powers skip it, the cross-spectrum does not
        sad[:, :2] = 0; ts = ts - 0.01
    elif name == "repeat":                   # a repeated timestamp on two noise frames in a row
        sad[:, :4] = 0; ts[:, 2] = ts[:, 1]; sad[:, T // 2] = 0
    return sad, ts


def nframes(U, T):
    n = np.full(U, T, np.int32)
    if U > 1:
        n[1] = max(1, T - 3)
    if U > 2:
        n[2] = 1
    return n


# kind, fftLen, C, pair list, T, sad pattern, smooth, window (None = infinite), interpolate, complex128 input, seed
CASES = [
    dict(kind="raw", N=64, C=2, pairs="star", T=16, sad="lead", smooth=True, win=None, interp=True, dbl=True, seed=1),
    dict(kind="gnnsub", N=256, C=4, pairs="all", T=14, sad="lead", smooth=True, win=None, interp=True, dbl=True, seed=2),
    dict(kind="phat", N=256, C=8, pairs="star", T=14, sad="speech_first", smooth=True, win=None, interp=False, dbl=False, seed=3),
    dict(kind="gnnsubphat", N=256, C=3, pairs="all", T=12, sad="speech_first", smooth=False, win=12, interp=True, dbl=True, seed=4),
    dict(kind="mlrraw", N=256, C=4, pairs="star", T=12, sad="ts0", smooth=True, win=None, interp=True, dbl=True, seed=5),
    dict(kind="mlrgnnsub", N=256, C=4, pairs="all", T=12, sad="repeat", smooth=True, win=20, interp=True, dbl=False, seed=6),
    dict(kind="mlrgnnsub", N=64, C=3, pairs="star", T=10, sad="speech_first", smooth=True, win=None, interp=False, dbl=True, seed=7),
    dict(kind="phat", N=64, C=64, pairs="star", T=8, sad="lead", smooth=True, win=None, interp=True, dbl=False, seed=8),
    dict(kind="raw", N=2048, C=3, pairs="all", T=8, sad="lead", smooth=False, win=None, interp=True, dbl=True, seed=9),
    dict(kind="phat", N=4096, C=2, pairs="star", T=6, sad="ts0", smooth=True, win=30, interp=True, dbl=True, seed=10),
    dict(kind="gnnsubphat", N=2048, C=2, pairs="star", T=7, sad="repeat", smooth=True, win=None, interp=False, dbl=False, seed=11),
    dict(kind="raw", N=256, C=16, pairs="all", T=8, sad="repeat", smooth=True, win=None, interp=True, dbl=False, seed=12),
]


def build(case, U=3):
    """-> dict(X complex128 [U][C][T][len] (rounded through complex64 when the case feeds complex64), nframes, sad, ts, pairs, minDelay, maxDelay)"""
    N, C, T = case["N"], case["C"], case["T"]
    X = spectra(case["seed"], U, C, T, N)
    if not case["dbl"]:
        X = X.astype(np.complex64).astype(np.complex128)
    sad, ts = sad_pattern(case["sad"], U, T)
    pairs = star(C) if case["pairs"] == "star" else all_pairs(C)
    w = case["win"]
    return dict(X=X, nframes=nframes(U, T), sad=sad, ts=ts, pairs=pairs, minDelay=-G.HUGE if w is None else -w / SR, maxDelay=G.HUGE if w is None else w / SR)


def reference(case, b):
    return G.run_batch(case["kind"], b["X"], b["nframes"], b["sad"], b["ts"], b["pairs"], SR, case["N"], interpolate=case["interp"], smooth=case["smooth"],
                       minDelay=b["minDelay"], maxDelay=b["maxDelay"])


def comparable(info, corr):
    """which comparisons one (frame, pair) item supports: (index, ratio, interpolation) -- the index where best and second best differ by more
    than 1e-9 of the frame's scale, the ratio where |maxCorr2| exceeds 1e-6 of it, the interpolated delay where the restatement's denominator
    exceeds 1e-6 of the two slopes it subtracts"""
    scale = np.abs(corr).max()
    idx = (info["maxCorr"] - info["maxCorr2"]) > 1e-9 * scale
    ratio = abs(info["maxCorr2"]) > 1e-6 * scale
    interp = idx and abs(info["den"]) > 1e-6 * info["denScale"]
    return idx, ratio, interp


def cctde_noise(n, nHeld):
    return np.random.default_rng(1000 + n + nHeld).standard_normal(5 * n).astype(np.float32)


def cctde_blocks(s, n, bl):
    """six block pairs of test_cctde_batch out of the noise s: block k of b lags block k of a by (k - 2) * 3 samples, the last a is silent"""
    a = np.stack([s[n + k * 7:n + k * 7 + bl] for k in range(6)]); b = np.stack([s[n + k * 7 - (k - 2) * 3:n + k * 7 - (k - 2) * 3 + bl] for k in range(6)])
    a[5] = 0.0                                                               # atan2(0, 0) = 0: a silent block gives a flat phase
    return a, b


def cctde_recording():
    """two recordings of unequal length, the second 11 samples behind the first"""
    s = (1000 * np.random.default_rng(31).standard_normal(21000)).astype(np.float32)
    return s[100:20100].copy(), s[89:19089].copy()

