"""The shapes of the block-convolution and frame-filter tests, shared by tests/test_conv_np_cpu.py and tests/test_gpu_conv.py.
Inputs are float32(3000 N(0,1)), responses N(0,1) exp(-6 k / P); every seed is fixed."""
import functools

import numpy as np

from tests import conv_np as R

# OverlapAdd: (L, P, fftLen, T, C)
ADD = {
    1: (4, 3, 0, 5, 1),            # minimum, N = 8
    2: (8, 8, 0, 6, 1),            # the tail spans a whole block
    3: (64, 200, 0, 9, 3),         # P-1 > 3L: four-deep fp32 chains; several channels
    4: (64, 3, 512, 4, 1),         # explicit fftLen above the minimum
    5: (160, 3000, 0, 24, 2),      # N = 4096, 19-deep chain
    6: (4096, 4097, 0, 2, 1),      # N = 8192, the LDS limit
    7: (5000, 6000, 0, 3, 1),      # N = 16384, the global path; L not a power of two
    8: (16, 1, 0, 3, 1),           # P = 1, an empty carried state
}
# OverlapSave: (L, P, T, C)
SAVE = {
    1: (8, 3, 4, 1),
    2: (256, 100, 5, 2),
    3: (8192, 4000, 2, 1),
    4: (16384, 100, 1, 1),
    5: (64, 63, 3, 1),             # one output sample
}
# FilterFeature: (dim, lenA, T)
FIR = {
    1: (1, 3, 1),
    2: (13, 5, 40),
    3: (39, 9, 4),                 # T = o
    4: (13, 9, 3),                 # empty
    5: (13, 1, 6),                 # 7 frames
    6: (512, 7, 33),
}


def signal(seed, T, L):
    return (3000.0 * np.random.default_rng(seed).standard_normal((T, L))).astype(np.float32)


def responses(seed, C, P):
    return np.random.default_rng(seed).standard_normal((C, P)) * np.exp(-6.0 * np.arange(P) / P)


@functools.lru_cache(maxsize=None)
def add_case(k):
    """x [T][L], h [C][P], N, the ld-flavour reference y [C][T][L] and its final buffers [C][L+P-1]; computed once, never written to"""
    L, P, fftLen, T, C = ADD[k]
    x = signal(100 + k, T, L); h = responses(200 + k, C, P)
    N = R.fft_len(L, P, fftLen)
    out = [R.overlap_add(x, h[c], fftLen, "ld") for c in range(C)]
    y = np.stack([o[0] for o in out]); buf = np.stack([o[1] for o in out])
    for a in (x, h, y, buf):
        a.setflags(write=False)
    return x, h, N, y, buf


@functools.lru_cache(maxsize=None)
def save_case(k):
    L, P, T, C = SAVE[k]
    x = signal(300 + k, T, L); h = responses(400 + k, C, P)
    y = np.stack([R.overlap_save(x, h[c], "ld") for c in range(C)])
    for a in (x, h, y):
        a.setflags(write=False)
    return x, h, y


def fir_coeffs(k, kind):
    dim, lenA, T = FIR[k]
    o = (lenA - 1) // 2
    if kind == "delta" and o >= 1:
        return R.regression_delta(o)
    return np.random.default_rng(600 + k).standard_normal(lenA)


@functools.lru_cache(maxsize=None)
def fir_case(k, kind):
    dim, lenA, T = FIR[k]
    x = signal(500 + k, T, dim); a = fir_coeffs(k, kind)
    y = R.filter_feature(x, a)
    for v in (x, a, y):
        v.setflags(write=False)
    return x, a, y


def differing(a, b):
    """elements whose bits differ (-0 and +0 count as different, NaNs never appear here)"""
    return int(np.count_nonzero(np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)))
