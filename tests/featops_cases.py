"""The cases the CPU and the GPU tests of the scalar feature operators share (tests/featops_np.py is the reference).  References are computed
once and handed out read-only."""
import functools
import os

import numpy as np

from tests import featops_np as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

YIN_N, YIN_SHIFT, YIN_FRAMES, YIN_MISSES, YIN_CHUNK_HITS = 512, 160, 840, 366, (16, 406, 30, 22)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def headset():
    return _ro(np.load(os.path.join(GOLDEN, "Headset1_16k_s16.npy")).astype(np.float32))


def frames(N, shift, count=None, start=0):
    """blocks of N samples of the Headset1 recording every `shift` samples (SampleFeature without padding)"""
    s = headset()[start:]
    T = (len(s) - N + shift - 1) // shift if len(s) > N else 0
    if count is not None:
        T = min(T, count)
    idx = np.arange(N)[None, :] + shift * np.arange(T)[:, None]
    return _ro(np.ascontiguousarray(s[idx]))


@functools.lru_cache(maxsize=None)
def yin_headset(threshold=0.5):
    """(frames [840][512], pitch, value, tau) of the restatement"""
    x = frames(YIN_N, YIN_SHIFT)
    p, v, tau = R.yin_pitch(x, 16000, threshold, details=True)
    return (x,) + _ro(p, v, tau)


def yin_chunk_histogram(tau, W=YIN_N // 2):
    """hits per chunk of 64 lags (tau = 64c .. 64c+63 is chunk c, as the kernel takes them) and the frames without one"""
    hit = tau[tau > 0]
    return tuple(int(c) for c in np.bincount(hit // 64, minlength=(W - 1) // 64 + 1)), int((tau == 0).sum())


def sine_frame(freq=200.0, rate=16000.0, N=512, amp=8000.0):
    return _ro((amp * np.sin(2.0 * np.pi * freq * np.arange(N) / rate)).astype(np.float32)[None, :])


def signed_zero_frame(N):
    """a frame with exact zeros of both signs between its samples"""
    x = frames(N, N, 1, start=8000)[0].copy()
    x[::3] = 0.0
    x[1::5] = -0.0
    return _ro(x[None, :])


def ties_block(n, seed):
    """small integers: every window of the median holds repeated values"""
    return _ro(np.random.default_rng(seed).integers(-2, 3, size=(4, n)).astype(np.float32))


SPIKE_BLOCK = 320


def spike_blocks(T=12, start=16000):
    return frames(SPIKE_BLOCK, SPIKE_BLOCK, T, start)


def with_spikes(x, where):
    """x [T][n] with +-20000 added at the (block, sample, sign) triples of `where`"""
    y = np.array(x, np.float32)
    for t, i, sg in where:
        y[t, i] += np.float32(sg * 20000.0)
    return _ro(y)


# spikes in the middle of a block, at samples 0 and 1, within `width` of the block's end, and in consecutive blocks
SPIKES = {"middle": [(2, 150, 1), (5, 200, -1)],
          "start": [(1, 0, 1), (3, 1, -1)],
          "end": [(2, 318, 1), (4, 317, -1), (6, 319, 1)],
          "consecutive": [(3, 100, 1), (4, 100, -1), (5, 101, 1), (6, 40, 1), (6, 41, 1)]}


def energy_chain(T=60, N=400, shift=160, start=4000):
    """SignalPower of Headset1 blocks [T][1]: what ALog and Normalize see in the speech-activity chain"""
    return _ro(R.signal_power(frames(N, shift, T, start)))


def differing(a, b):
    """elements whose bits differ; a NaN equals a NaN of any payload"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    iv = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    same = (np.ascontiguousarray(a).view(iv) == np.ascontiguousarray(b).view(iv)) | (np.isnan(a) & np.isnan(b))
    return int((~same).sum())
