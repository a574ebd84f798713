"""numpy restatement of the sample-rate converter of include/dsr.h section 6d (the definition behind SamplerateConversionFeature,
btk/feature/feature.h:794-816): the sinc methods in fp64, zoh and linear in float32 exactly as defined, the one-shot call and the block-by-block
stream with its carried state.  Nothing here calls the library."""
from math import gcd

import numpy as np

METHODS = {"fastest": (10, 7.0, 0.84), "medium": (16, 9.5, 0.90), "best": (32, 12.0, 0.95)}
SINC = tuple(METHODS)
TABLE_CAP = 1 << 22


def ratio(src, dst, method="fastest"):
    """-> (L, M, K); K = ceil(Z / s) for a sinc method, 0 for zoh and for equal rates, 1 for linear"""
    if method not in METHODS and method not in ("zoh", "linear"):
        raise KeyError("Cannot recognize type (%s) of sample rate converter." % method)
    if src <= 0 or dst <= 0:
        raise ValueError("sample rates must be positive")
    g = gcd(src, dst); L, M = dst // g, src // g
    if src == dst or method == "zoh":
        return L, M, 0
    if method == "linear":
        return L, M, 1
    Z = METHODS[method][0]
    K = -(-Z * M // L) if L < M else Z
    if 2 * K * L > TABLE_CAP:
        raise ValueError("a table of %d x %d coefficients is above 2^22" % (L, 2 * K))
    return L, M, K


def out_samples(src, dst, n):
    L, M, _ = ratio(src, dst, "zoh")
    return n * L // M


def table(src, dst, method):
    """fp64 [L][2K]: row p holds h_p[j], j = -K+1 .. K, divided by the row's sum"""
    L, M, K = ratio(src, dst, method); Z, beta, c = METHODS[method]
    s = min(1.0, L / M)
    j = np.arange(-K + 1, K + 1, dtype=np.float64)
    d = (np.arange(L, dtype=np.float64) / L)[:, None] - j[None, :]
    v = d * s / Z
    w = np.where(np.abs(v) < 1.0, np.i0(beta * np.sqrt(np.maximum(1.0 - v * v, 0.0))) / np.i0(beta), 0.0)
    h = s * c * np.sinc(s * c * d) * w
    return h / h.sum(axis=1, keepdims=True)


def _window(x, first, n):
    """x[first : first + n] with zeros outside the array"""
    out = np.zeros(n, x.dtype); lo, hi = max(first, 0), min(first + n, x.size)
    if hi > lo:
        out[lo - first:hi - first] = x[lo:hi]
    return out


def _outputs(x, first, src, dst, method, n0, n1, tab=None):
    """outputs n0 .. n1-1 of a stream whose samples first .. first + len(x) - 1 are x and whose other samples are zero -> (y, sum_j |h_j x_j|);
    y is fp64 for a sinc method, float32 for zoh and linear"""
    L, M, K = ratio(src, dst, method)
    n = np.arange(n0, max(n1, n0), dtype=np.int64); base = n * M // L - first; p = n * M % L
    if src == dst or method == "zoh":
        y = np.array([_window(x, int(b), 1)[0] for b in base], x.dtype)
        return y, np.abs(y).astype(np.float64)
    if method == "linear":
        x = x.astype(np.float32)
        x0 = np.array([_window(x, int(b), 1)[0] for b in base], np.float32); x1 = np.array([_window(x, int(b) + 1, 1)[0] for b in base], np.float32)
        f = p.astype(np.float32) / np.float32(L)
        d = (x1 - x0).astype(np.float32); y = (x0 + (f * d).astype(np.float32)).astype(np.float32)
        return y, np.abs(y).astype(np.float64)
    tab = table(src, dst, method) if tab is None else tab
    xd = x.astype(np.float64); y = np.zeros(n.size); mag = np.zeros(n.size)
    for i in range(n.size):
        t = tab[p[i]] * _window(xd, int(base[i]) - K + 1, 2 * K)
        y[i] = t.sum(); mag[i] = np.abs(t).sum()
    return y, mag


def convert(x, src, dst, method, with_mag=False):
    """the one-shot call: floor(N L / M) outputs of the N samples x"""
    y, mag = _outputs(np.asarray(x), 0, src, dst, method, 0, out_samples(src, dst, len(x)))
    return (y, mag) if with_mag else y


def block_end(src, dst, method, b, flush):
    """the count of outputs a stream has produced once b input samples are in: those whose last tap base + K lies below b, or with flush
    floor(b L / M)"""
    L, M, K = ratio(src, dst, method); total = b * L // M
    if flush:
        return total
    t = b - K
    return min(-(-t * L // M) if t > 0 else 0, total)


class Stream:
    """the carried state of one row: the last 2K input samples and the counts of inputs consumed and outputs produced.  zoh and linear keep
    ceil(M / L) samples more: the count floor(b L / M) can hold back an output whose taps were all there, and its base lies that far back."""

    def __init__(self, src, dst, method):
        L, M, self.K = ratio(src, dst, method); self.args = (src, dst, method)
        self.H = 0 if src == dst else 2 * self.K if method in METHODS else 2 * self.K + -(-M // L)
        self.hist = None; self.nin = 0; self.nout = 0
        self.tab = table(src, dst, method) if (method in METHODS and src != dst) else None

    def push(self, block, flush=False):
        """-> the outputs this block releases; reads nothing but the block and the 2K samples kept"""
        block = np.asarray(block); H = self.H
        if self.hist is None:
            self.hist = np.zeros(H, block.dtype)
        a, b = self.nin, self.nin + block.size
        end = max(block_end(*self.args, b, flush), self.nout)
        known = np.concatenate([self.hist, block])                                     # samples a - H .. b - 1 of the stream
        y, _ = _outputs(known, a - H, *self.args, self.nout, end, self.tab)
        self.hist = known[known.size - H:]; self.nin, self.nout = b, end
        return y


def stream_convert(x, src, dst, method, block_lens):
    """x cut into blocks of the given lengths (the last one flushed) through Stream -> the concatenated outputs"""
    assert sum(block_lens) == len(x)
    s = Stream(src, dst, method); out = []; pos = 0
    for i, n in enumerate(block_lens):
        out.append(s.push(x[pos:pos + n], flush=(i == len(block_lens) - 1))); pos += n
    return np.concatenate(out) if out else np.zeros(0)


def feature_size(src_size, sourcerate, destrate, length=0):
    """size() of SamplerateConversionFeature (feature.cc:1612), in float arithmetic"""
    if length:
        return int(length)
    return int(np.float32(np.float32(src_size) * np.float32(destrate)) / np.float32(sourcerate))


def tone(freq, rate, seconds=0.5):
    return np.sin(2.0 * np.pi * freq * np.arange(int(rate * seconds)) / rate)


def tone_amplitude(y, freq, rate):
    """amplitude of the tone at freq from a Hann-windowed DFT at that frequency (the window's mean is its coherent gain)"""
    n = np.arange(y.size); w = np.hanning(y.size)
    return 2.0 * np.abs(np.sum(w * y * np.exp(-2j * np.pi * freq * n / rate))) / w.sum()


def central_half(y):
    return y[y.size // 4: y.size - y.size // 4]
