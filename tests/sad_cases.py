"""The cases the CPU and the GPU tests of speech activity detection share (tests/sad_np.py is the reference).  References are computed once
and handed out read-only."""
import functools
import os

import numpy as np

from tests import sad_np as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATE = 16000.0


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def headset():
    return _ro(np.load(os.path.join(GOLDEN, "Headset1_16k_s16.npy")).astype(np.float32))


@functools.lru_cache(maxsize=None)
def blocks(N=160, count=None, start=0):
    """consecutive blocks of N samples of the Headset1 recording [T][N]"""
    s = headset()[start:]
    T = len(s) // N if count is None else min(len(s) // N, count)
    return _ro(np.ascontiguousarray(s[:T * N].reshape(T, N)))


# (energiesN, block length, headN, tailN, threshold): every history size on either side of the 64-lane chunk, the shortest block, every
# head / tail / threshold of the issue
ENERGY_CONFIGS = [(200, 160, 4, 10, 0.5), (5, 160, 4, 10, 0.5), (1, 160, 1, 1, 0.0), (64, 160, 10, 4, 0.31), (65, 160, 1, 10, 0.31),
                  (800, 160, 4, 4, 0.5), (200, 1, 4, 10, 0.5), (5, 1, 10, 1, 0.0)]
ENERGY_INITIAL = 5.0e+07


def energy_blocks(blockLen):
    """all 842 blocks of 160 samples; 400 single-sample blocks out of the first utterance's onset"""
    return blocks(160) if blockLen == 160 else blocks(1, 400, 17 * 160)


@functools.lru_cache(maxsize=None)
def energy_reference(cfg):
    """(decision, score, history, counters, updates, segment) of the restatement over the whole recording, segment = hangover(kind 0) of the decisions"""
    N, blockLen, headN, tailN, thr = cfg
    m = R.EnergyVADMetric(ENERGY_INITIAL, thr, headN, tailN, N)
    dec, score = m.run(energy_blocks(blockLen))
    hist, cnt = m.state()
    seg = R.hangover(dec[None], [0.5], headN, tailN, 0)
    return _ro(dec, score, hist, cnt) + (m.updates, (seg["start"], seg["start"] + seg["length"]))


@functools.lru_cache(maxsize=None)
def channels(C, fftLen, T, start=16000, coherent=True):
    """Headset1-derived array channels: channel c is the recording delayed by 3c samples and attenuated, plus its own weak noise.
    -> (spectra complex128 [C][T][fftLen], power float32 [C][T][fftLen/2+1]) of Hamming-windowed frames every fftLen/2 samples"""
    s = headset().astype(np.float64)
    rng = np.random.default_rng(100 * C + fftLen)
    w = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(fftLen) / (fftLen - 1))
    idx = start + np.arange(fftLen)[None, :] + (fftLen // 2) * np.arange(T)[:, None]
    X = np.zeros((C, T, fftLen), np.complex128)
    for c in range(C):
        x = s[idx - 3 * c] / (1.0 + 0.3 * c) + 20.0 * rng.standard_normal((T, fftLen))
        if not coherent and c > 0:
            x = 300.0 * rng.standard_normal((T, fftLen))
        X[c] = np.fft.fft(x * w, axis=1)
    P = (X[:, :, :fftLen // 2 + 1].real ** 2 + X[:, :, :fftLen // 2 + 1].imag ** 2).astype(np.float32)
    return _ro(X, P)


# (C, fftLen, lowCutoff, highCutoff)
POWER_CASES = [(2, 64, -1.0, -1.0), (3, 512, -1.0, -1.0), (8, 64, 187.0, 1000.0), (3, 512, 187.0, 1000.0), (8, 512, -1.0, -1.0)]
POWER_T = 24

# (C, fftLen, nCand, lowX, highX): highX None = fftLen / 2
CCC_CASES = [(2, 64, 1, 0, None), (3, 256, 3, 0, None), (3, 256, 4, 6, 62), (5, 512, 8, 0, None)]
CCC_T = 10
CCC_THRESHOLD = 0.1


@functools.lru_cache(maxsize=None)
def ccc_input(case, silent=True):
    C, N, nCand, lowX, highX = case
    X = np.array(channels(C, N, CCC_T)[0])
    if silent:
        X[:, 3, :] = 0.0                                                  # a silent frame: 0 / 0 in the PHAT weighting
    return _ro(X)


@functools.lru_cache(maxsize=None)
def ccc_reference(case, **kw):
    C, N, nCand, lowX, highX = case
    return _ro(*R.ccc_metric(ccc_input(case), lowX, N // 2 if highX is None else highX, nCand, CCC_THRESHOLD, **kw))


def left_out(score, threshold, tol):
    """frames whose score lies within tol of the threshold: their decision is not compared.  A score that is no number is compared: its
    decision follows from IEEE comparisons alone."""
    with np.errstate(invalid="ignore"):
        return np.abs(score - threshold) <= tol


LEFT_OUT_CAP = 0.02


def pattern(s):
    """a decision row from a string: '1' above, '0' below"""
    return np.array([1.0 if ch == "1" else 0.0 for ch in s], np.float64)


# (name, kind, decisions [K] as strings, headN, tailN): speech at frame 0, speech never, the source ending inside a segment, tailN reached
# exactly at the last frame, a second segment that must not be emitted, and the MI / multi-stage codes
HANGOVER_CASES = [
    ("base_at_zero", 0, ["1111100000000"], 4, 3),
    ("base_never", 0, ["0101011010110"], 3, 2),
    ("base_source_ends", 0, ["0011111111"], 4, 5),
    ("base_tail_at_last", 0, ["0111101000"], 4, 3),
    ("base_second_segment", 0, ["00111100001111000"], 2, 3),
    ("base_head1_tail1", 0, ["0010"], 1, 1),
    ("base_shorter_than_head", 0, ["111"], 4, 2),
    ("mi_codes", 1, ["0111111111100000", "0001110011111111", "0001100000000000"], 2, 3),
    ("mi_never", 1, ["1111", "1111", "0000"], 2, 2),
    ("multi_two_metrics", 2, ["11111111", "11111111"], 2, 2),
    ("multi_three", 2, ["011111111100000", "001100110011001", "000011110000111"], 3, 2),
    ("multi_four", 2, ["1111111111", "0000011111", "0011000000", "0100100100"], 2, 4),
]


def hangover_input(case):
    name, kind, rows, headN, tailN = case
    dec = np.stack([pattern(r) for r in rows])
    if kind != 0:
        dec[1:] = 2.0 * dec[1:] - 1.0                                     # the later stages are +-1 metrics
    return dec


# the spectral-shape operators: (dim, T) with one frame of zeros (0 / 0 in every normalisation) and one of a single spike
SHAPE_CASES = [(257, 60), (33, 7), (1000, 5)]


@functools.lru_cache(maxsize=None)
def shape_input(case):
    dim, T = case
    fftLen = 2 * (dim - 1) if dim in (257, 33) else 2048
    x = np.array(channels(1, fftLen, T)[1][0][:, :dim])
    if dim == 1000:
        x = np.array(blocks(1000, T, 20000))                              # signed samples: the rectifier of NegativeEntropy has work
    x[2] = 0.0
    x[3] = 0.0; x[3, dim // 3] = 7.0
    return _ro(x)


# the generalised-Gaussian metrics: (fftLen, mixed shape factors, twiddle, lowCutoff, highCutoff), T frames of two coherent channels
GG_CASES = [(64, False, -1.0, -1.0, -1.0), (64, True, 1.0, -1.0, -1.0), (512, True, -1.0, 187.0, 1000.0), (512, False, 1.0, -1.0, -1.0)]
GG_T = 60
GG_THRESHOLDS = {"negentropy": 0.5, "mi": 1.3, "lr": 0.0}


def gg_shape_factors(fftLen):
    """mixed shape factors in [0.3, 1.9], one a bin"""
    return _ro(np.round(np.random.default_rng(fftLen).uniform(0.3, 1.9, fftLen // 2 + 1), 4))


def write_shape_factors(directory, sf):
    """the reference's directory: one file _M-%04d a bin, the shape factor the second token of its first line"""
    for b, f in enumerate(sf):
        with open(os.path.join(str(directory), "_M-%04d" % b), "w") as fp:
            fp.write("%d %.4f 1.0\nignored\n" % (b, f))


@functools.lru_cache(maxsize=None)
def gg_input(fftLen, T=GG_T):
    """(X1, X2 complex128 [T][fftLen], env1, env2 float32 [T][fftLen/2+1]): channel 2 is channel 1 delayed and attenuated (coherent); the
    envelopes are the power spectra smoothed over five bins"""
    X, P = channels(2, fftLen, T, start=30000)
    k = np.ones(5) / 5.0
    env = np.stack([[np.convolve(np.pad(P[c, t].astype(np.float64), 2, mode="edge"), k, mode="valid") for t in range(T)] for c in range(2)]).astype(np.float32)
    return _ro(np.ascontiguousarray(X[0]), np.ascontiguousarray(X[1]), np.ascontiguousarray(env[0]), np.ascontiguousarray(env[1]))


@functools.lru_cache(maxsize=None)
def gg_reference(case, reverse=False):
    """dict of the three metrics' (decision, score, [threshold,] tolerance base) and the final rho, from tests/sad_np.py"""
    fftLen, mixed, twiddle, lo, hi = case
    lowX, highX, _ = R.band(fftLen, RATE, lo, hi)
    m = R.GGModel(gg_shape_factors(fftLen) if mixed else None, fftLen, lowX, highX); m.reverse = reverse
    X1, X2, e1, e2 = gg_input(fftLen)
    rho = np.zeros(m.F, np.complex128)
    mi = R.mutual_information(m, X1, X2, e1, e2, rho, twiddle, GG_THRESHOLDS["mi"], 0.95)
    return dict(model=m, negentropy=R.negentropy(m, X1, e1, GG_THRESHOLDS["negentropy"]), lr=R.likelihood_ratio(m, X1, X2, e1, e2, GG_THRESHOLDS["lr"]), mi=mi, rho=rho)
