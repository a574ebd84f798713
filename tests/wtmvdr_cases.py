"""The cases of the WarpedTwiceMVDRFeature tests and their restated results, computed once a process and shared."""
import functools

import numpy as np

from tests import wtmvdr_np as W

# (dim, order, correlate, warp, fixed, sensibility, nFrames)
CASES = [
    (64, 8, 0, 0.4595, False, 0.1, 8),       # N = dim
    (64, 32, 0, 0.3, False, 0.2, 8),         # the largest order allowed: tim = dim + 1
    (80, 20, 0, 0.4595, True, 0.1, 8),       # N = 128 > dim, fixed mode
    (100, 13, 40, -0.2, False, 0.1, 8),      # correlate used, negative warp
    (64, 8, 0, 0.0, True, 0.0, 8),           # degenerate: rewarp 0, the chain a pure delay
    (320, 60, 0, 0.4595, False, 0.1, 4),     # the reference's defaults at 16 kHz
    (512, 256, 0, 0.3, False, 0.1, 2),       # an order whose state cannot sit in LDS
    (2050, 4, 0, 0.3, False, 0.1, 1),        # a frame whose transform does not stage in LDS (twiddles alone take 64 KiB)
    (256, 100, 0, 0.4595, False, 0.1, 2),    # state in LDS beyond the 64 KiB a kernel gets without asking (77 KiB)
]
DEGENERATE = 4


def ar_frames(T, dim, seed):
    """a stable resonance times a Hamming window (as _ar_frames of tests/test_gpu_parity.py)"""
    rng = np.random.default_rng(seed)
    fr = np.zeros((T, dim), np.float32)
    for t in range(T):
        rad, th = rng.uniform(0.5, 0.95), rng.uniform(0.2, 2.8); a1, a2 = 2 * rad * np.cos(th), -rad * rad
        e = rng.standard_normal(dim + 64) * 300.0; y = np.zeros(dim + 64)
        for n in range(2, dim + 64):
            y[n] = a1 * y[n - 1] + a2 * y[n - 2] + e[n]
        fr[t] = (y[64:] * np.hamming(dim)).astype(np.float32)
    return fr


@functools.lru_cache(maxsize=None)
def frames(ci):
    """the case's nFrames resonances + an all-zero frame, a frame with a single non-zero sample, a constant frame"""
    dim, nF = CASES[ci][0], CASES[ci][6]
    fr = np.zeros((nF + 3, dim), np.float32)
    fr[:nF] = ar_frames(nF, dim, seed=200 + ci)
    fr[nF + 1, dim // 3] = 1234.5
    fr[nF + 2] = 100.0
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def restated(ci, streamed=True, warp=None):
    """-> list of wtmvdr_frame dicts, one a frame of the case (warp: in place of the case's)"""
    dim, order, corr, wp, fixed, sens, _ = CASES[ci]
    return [W.wtmvdr_frame(x, order, corr, wp if warp is None else warp, fixed, sens, streamed) for x in frames(ci)]
