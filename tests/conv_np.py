"""numpy restatement of OverlapAdd, OverlapSave (btk/convolution/convolution.cc:43-290), FilterFeature and MergeFeature
(btk/feature/feature.cc:3206-3350), statement by statement where the order of the roundings can be seen.

OverlapAdd's sections come in two flavours: `fft` (np.fft.rfft / irfft in fp64, what the reference computes with gsl) and `ld` (the linear
convolution of the block by np.convolve in longdouble, rounded to fp64: the value the transforms approximate).  Both go through the same fp32
buffer recurrence, float(double(buffer) + section) for every block in turn."""
import numpy as np


def fft_len(L, P, fftLen=0):
    """OverlapAdd::_checkFFTLen (convolution.cc:80-102)"""
    if fftLen == 0:
        N = 1
        while N < L + P - 1:
            N *= 2
        return N
    if fftLen < L + P - 1:
        raise ValueError("Section (%d) and impulse response (%d) lengths inconsistent with FFT length (%d)." % (L, P, fftLen))
    return fftLen


def sections_fft(x, h, N):
    """x float32 [T][L], h float64 [P] -> the first L+P-1 samples of every block's section, fp64 [T][L+P-1]"""
    L, P = x.shape[1], h.size
    H = np.fft.rfft(h, N)
    H[0] = H[0].real; H[-1] = H[-1].real                              # _halfComplexUnpack keeps the real parts of bins 0 and N/2
    return np.fft.irfft(np.fft.rfft(x.astype(np.float64), N, axis=1) * H, N, axis=1)[:, :L + P - 1]


def sections_ld(x, h):
    hl = h.astype(np.longdouble)
    return np.stack([np.convolve(b.astype(np.longdouble), hl).astype(np.float64) for b in x]) if len(x) else np.zeros((0, x.shape[1] + h.size - 1))


def ola_fold(sec, L, P, buffer=None):
    """OverlapAdd::next from "add contribution of new section to buffer" on (convolution.cc:148-160); returns (y [T][L], buffer)"""
    buf = np.zeros(L + P - 1, np.float32) if buffer is None else buffer.copy()
    y = np.zeros((len(sec), L), np.float32)
    for t, s in enumerate(sec):
        buf = (buf.astype(np.float64) + s).astype(np.float32)
        y[t] = buf[:L]
        buf[:P - 1] = buf[L:L + P - 1].copy()
        buf[P - 1:] = 0.0
    return y, buf


def overlap_add(x, h, fftLen=0, flavour="ld", buffer=None):
    L, P = x.shape[1], h.size
    N = fft_len(L, P, fftLen)
    sec = sections_fft(x, h, N) if flavour == "fft" else sections_ld(x, h)
    return ola_fold(sec, L, P, buffer)


def ola_fold_wrong(sec, L, P, how):
    """the two folds the reference does NOT compute: "once" sums a sample's contributions in fp64 and rounds once, "newest" rounds after every
    add but takes the newest block first"""
    T, S = sec.shape
    y = np.zeros((T, L), np.float32)
    D = (S - 1) // L                                                  # the oldest block that reaches block t is t - D
    for t in range(T):
        parts = [sec[t - d, d * L:d * L + L] for d in range(D + 1) if t - d >= 0]      # newest first; the last may be short
        parts = [np.pad(q, (0, L - q.size)) for q in parts]
        if how == "once":
            y[t] = np.sum(np.stack(parts), axis=0).astype(np.float32)
        else:
            acc = np.zeros(L, np.float32)
            for q in parts:
                acc = (acc.astype(np.float64) + q).astype(np.float32)
            y[t] = acc
    return y


def save_response(h, L, delta=None):
    """the response whose circular convolution OverlapSave computes: h padded to L, plus what update(delta) adds to bins 0..L/2"""
    hh = np.zeros(L); hh[:h.size] = h
    if delta is not None:
        hh = hh + np.fft.irfft(np.asarray(delta)[:L // 2 + 1], L)
    return hh


def overlap_save(x, h, flavour="ld", delta=None):
    """x float32 [T][L] -> float32 [T][L-P]: samples P..L-1 of the circular convolution (convolution.cc:250-271)"""
    L, P = x.shape[1], h.size
    if P >= L:
        raise ValueError("Cannot have P = %d and L = %d" % (P, L))
    if flavour == "fft":
        H = np.fft.rfft(h, L)
        if delta is not None:
            H = H + np.asarray(delta)[:L // 2 + 1]
        H[0] = H[0].real; H[-1] = H[-1].real
        return np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=1) * H, L, axis=1)[:, P:].astype(np.float32)
    hl = save_response(h, L, delta).astype(np.longdouble)
    if delta is None:
        hl = hl[:P]
    out = np.zeros((len(x), L - P), np.float32)
    for t, b in enumerate(x):
        lin = np.convolve(b.astype(np.longdouble), hl)
        circ = lin[:L].copy(); circ[:lin.size - L] += lin[L:]
        out[t] = circ[P:].astype(np.float64).astype(np.float32)
    return out


def fir_count(T, lenA):
    """frames FilterFeature delivers for T source frames (feature.cc:3230-3269): the priming loop reads o frames and ends the stream when they
    are not there; then one frame per source frame, one more when the source ends (before the count of padded frames is looked at), and
    further ones while that count is below o"""
    o = (lenA - 1) // 2
    if T < o:
        return 0
    return T + 1 if o == 0 else T


def filter_feature(x, a):
    """x float32 [T][dim], a float64 [lenA] -> float32 [fir_count][dim]; scalar loop, the product and the sum rounded separately"""
    T, dim = x.shape
    lenA = len(a)
    if lenA % 2 != 1:
        raise ValueError("Length of filter (%d) is not odd." % lenA)
    o = (lenA - 1) // 2
    y = np.zeros((fir_count(T, lenA), dim), np.float32)
    af = [float(v) for v in a]
    xs = x.astype(np.float64).tolist()
    for t in range(y.shape[0]):
        for c in range(dim):
            s = 0.0
            for i in range(-o, o + 1):
                k = t - i
                v = xs[k][c] if 0 <= k < T else 0.0
                p = af[i + o] * v
                s = s + p
            y[t, c] = np.float32(s)
    return y


def merge_feature(stat, delta, deltaDelta):
    T = min(len(stat), len(delta), len(deltaDelta))
    return np.concatenate([stat[:T], delta[:T], deltaDelta[:T]], axis=1).astype(np.float32)


def regression_delta(o):
    """the usual regression window: a[i+o] weighs x[t-i], so the slope sum_k k (x[t+k] - x[t-k]) / (2 sum k^2) has a[i+o] = -i / (2 sum k^2)"""
    den = 2.0 * sum(k * k for k in range(1, o + 1))
    return np.array([-i / den for i in range(-o, o + 1)], np.float64)


def tolerance(ref, N, xnorm, hnorm):
    """per element: one fp32 rounding of the reference plus a ~500-fold margin over the fp64 radix-2 bound eps64 log2(N) |x| |h|"""
    return 2.0 ** -23 * np.abs(ref.astype(np.float64)) + 2.0 ** -44 * np.log2(N) * xnorm * hnorm
