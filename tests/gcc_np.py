"""Numpy fp64 restatement of the pairwise time-delay estimators: the GCC family (btk/localization/localization.h:75-218,
localization.cc:1156-1413: NoisePowerSpectrum::add, NoiseCrossSpectrum::add, the six calcCrossSpectrumValue forms, GCC::calculate,
GCC::findMaximum, getInterpolation :872-894) and CCTDE (btk/TDEstimator/CCTDE.cc:46-342), in the reference's order of operations.
The GPU tests check the device against it; tests/test_gcc_np_cpu.py checks it against independent forms.

Stated values where the reference reads undefined memory: the constructor's alpha is honoured, the smoothed cross-spectrum
and the correlation start at zero, one smoothed cross-spectrum per pair, GCCGnnSub before any noise frame raises."""
import numpy as np

RAW, GNNSUB, PHAT, GNNSUBPHAT, MLRRAW, MLRGNNSUB = range(6)
KINDS = {"raw": RAW, "gnnsub": GNNSUB, "phat": PHAT, "gnnsubphat": GNNSUBPHAT, "mlrraw": MLRRAW, "mlrgnnsub": MLRGNNSUB}
HUGE = float(np.finfo(np.float32).max)          # <math.h> HUGE, the default window of findMaximum (localization.h:126)


def cmul(a, b):
    """gsl_complex_mul"""
    return (a.real * b.real - a.imag * b.imag) + 1j * (a.real * b.imag + a.imag * b.real)


def cabs(a):
    """gsl_complex_abs = hypot"""
    return np.hypot(a.real, a.imag)


def cross_value(kind, x1, x2, Gn, N1, N2, q):
    """calcCrossSpectrumValue (:1342-1413) for all bins; Gn / N1 / N2 None = no estimate yet (the reference's NULL)"""
    with np.errstate(all="ignore"):
        G = cmul(x1, np.conj(x2))
        if kind == RAW:
            return G
        if kind == GNNSUB:
            if Gn is None:
                raise RuntimeError("GCCGnnSub: no noise cross-spectrum yet")       # the reference dereferences NULL
            return G - Gn
        if kind == PHAT:
            w = cabs(G)
            out = np.zeros_like(G)
            nz = w != 0.0
            out[nz] = G[nz].real / w[nz] + 1j * (G[nz].imag / w[nz])
            return out
        if kind == GNNSUBPHAT:
            D = G - Gn if Gn is not None else G
            w = cabs(D)
            return D.real / w + 1j * (D.imag / w)
        X1 = cabs(x1); X12 = X1 * X1; X2 = cabs(x2); X22 = X2 * X2
        q1, q2 = 1 - q, 2 * q
        if kind == MLRRAW:
            w = X1 * X2 / (q2 * X12 * X22 + q1 * (N2 * X12 + N1 * X22)) if (N1 is not None and N2 is not None) else X1 * X2 / (q2 * X12 * X22)
            return G.real * w + 1j * (G.imag * w)
        if Gn is not None and N1 is not None and N2 is not None:
            D = G - Gn
            w = X1 * X2 / (q2 * X12 * X22 + q1 * (N2 * X12 + N1 * X22))
            return D.real * w + 1j * (D.imag * w)
        w = X1 * X2 / (q2 * X12 * X22)
        return G.real * w + 1j * (G.imag * w)


def half_complex_pack(spec, fftLen):
    """halfComplexPack (feature.cc:65-83): r0, r1 .. r(n/2), i(n/2-1) .. i1"""
    h = np.zeros(fftLen)
    n2 = fftLen // 2
    h[0] = spec[0].real
    h[1:n2] = spec[1:n2].real
    h[fftLen - 1:n2:-1] = spec[1:n2].imag
    h[n2] = spec[n2].real
    return h


def fft_radix2(z, sign):
    """unscaled radix-2 decimation-in-time transform of a power-of-two length, exponent sign `sign`, vectorised over the butterflies of a stage"""
    n = len(z); bits = n.bit_length() - 1
    rev = np.zeros(n, np.int64)
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    a = np.asarray(z, np.complex128)[rev]
    h = 1
    while h < n:
        w = np.exp(sign * 1j * np.pi * np.arange(h) / h)
        a = a.reshape(-1, 2, h)
        t = a[:, 1, :] * w
        a = np.stack([a[:, 0, :] + t, a[:, 0, :] - t], axis=1).reshape(-1)
        h *= 2
    return a


def half_complex_inverse(h):
    """gsl_fft_halfcomplex_radix2_inverse: the real sequence whose spectrum the packed array holds, scaled by 1/n"""
    n = len(h); n2 = n // 2
    full = np.zeros(n, np.complex128)
    full[0] = h[0]; full[n2] = h[n2]
    k = np.arange(1, n2)
    full[k] = h[k] + 1j * h[n - k]
    full[n - k] = h[k] - 1j * h[n - k]
    return fft_radix2(full, +1.0).real / n


def correlation(spec, fftLen):
    return half_complex_inverse(half_complex_pack(spec, fftLen))


def interpolation(xv, yv, pos):
    """getInterpolation (:872-894) on the delay-ordered table; returns (delay, denominator, |terms|) so callers can see the conditioning"""
    n = len(xv)
    if pos == 0:
        pos = 1
    elif pos == n - 1:
        pos = n - 2
    x0, y0, x1, y1, x2, y2 = xv[pos - 1], yv[pos - 1], xv[pos], yv[pos], xv[pos + 1], yv[pos + 1]
    with np.errstate(all="ignore"):
        a = np.float64(y2 - y1) / (x2 - x1); b = np.float64(y1 - y0) / (x1 - x0)
        den = a - b
        delay = 0.5 * ((x0 + x1) - b * (x2 - x0) / den)
    return float(delay), float(den), float(abs(a) + abs(b))


def find_maximum(corr, sampleRate, minDelay=-HUGE, maxDelay=HUGE, interpolate=True):
    """GCC::findMaximum (:1297-1340) -> dict(delay, maxCorr, ratio, pos (index into the delay-ordered table), maxCorr2, den, denScale)"""
    n = len(corr); n2 = (n + 1) // 2
    maxCorr, maxCorr2, pos, delay = -HUGE, -HUGE, 0, 0.0
    xv = np.zeros(n); yv = np.zeros(n)
    for i in range(n):
        if i < n2:
            idx = i + n2; d = i / sampleRate
        else:
            idx = i - n2; d = -((n - i) / sampleRate)
        c = corr[i]
        xv[idx] = d; yv[idx] = c
        if d >= minDelay and d <= maxDelay and c > maxCorr:
            maxCorr2 = maxCorr; maxCorr = c; pos = idx; delay = d
        elif d >= minDelay and d <= maxDelay and c > maxCorr2:
            maxCorr2 = c
    with np.errstate(all="ignore"):
        ratio = float(np.float64(maxCorr) / np.float64(maxCorr2))
    den = scale = 0.0
    if interpolate:
        delay, den, scale = interpolation(xv, yv, pos)
    return dict(delay=delay, maxCorr=float(maxCorr), ratio=ratio, pos=pos, maxCorr2=float(maxCorr2), den=den, denScale=scale)


class NoisePower:
    """NoisePowerSpectrum (:1156-1183): updates only when the timestamp differs from the last one, which starts at 0.0"""

    def __init__(self, alpha):
        self.alpha, self.p, self.ts = alpha, None, 0.0

    def add(self, spec, ts, ln):
        if self.ts != ts:
            v = cabs(spec[:ln])
            a1 = 1 - self.alpha
            self.p = self.alpha * self.p + a1 * v * v if self.p is not None else a1 * v * v
            self.ts = ts


class NoiseCross:
    """NoiseCrossSpectrum (:1185-1218)"""

    def __init__(self, alpha):
        self.alpha, self.g = alpha, None

    def add(self, s1, s2, ln):
        v = cmul(s1[:ln], np.conj(s2[:ln]))
        a1 = 1 - self.alpha
        v = v.real * a1 + 1j * (v.imag * a1)
        self.g = (self.g.real * self.alpha + v.real) + 1j * (self.g.imag * self.alpha + v.imag) if self.g is not None else v


class GCC:
    """GCC (:1220-1340) with one smoothed cross-spectrum and one correlation per pair"""

    def __init__(self, kind, sampleRate=44100.0, fftLen=2048, nChan=16, pairs=6, alpha=0.95, beta=0.5, q=0.3, interpolate=True, noisereduction=True):
        self.kind = KINDS[kind] if isinstance(kind, str) else kind
        self.sampleRate, self.fftLen, self.len = sampleRate, fftLen, fftLen // 2 + 1
        self.beta, self.q, self.interpolate = beta, q, interpolate
        self.np_ = [NoisePower(alpha) for _ in range(nChan)]
        self.nc = [NoiseCross(alpha) for _ in range(pairs)]
        self.cross = [np.zeros(self.len, np.complex128) for _ in range(pairs)]
        self.corr = [np.zeros(fftLen) for _ in range(pairs)]
        self.valid = [0] * pairs
        self.last = 0

    def setAlpha(self, alpha):
        for o in self.np_ + self.nc:
            o.alpha = alpha

    def calculate(self, s1, chan1, s2, chan2, pair, timestamp, sad=False, smooth=True):
        s1 = np.asarray(s1, np.complex128); s2 = np.asarray(s2, np.complex128)
        self.last = pair
        if sad:
            G = cross_value(self.kind, s1[:self.len], s2[:self.len], self.nc[pair].g, self.np_[chan1].p, self.np_[chan2].p, self.q)
            if smooth:
                b, b1 = self.beta, 1 - self.beta
                c = self.cross[pair]
                self.cross[pair] = (c.real * b + G.real * b1) + 1j * (c.imag * b + G.imag * b1)
            else:
                self.cross[pair] = G
            self.corr[pair] = correlation(self.cross[pair], self.fftLen)
            self.valid[pair] = 1
        else:
            self.np_[chan1].add(s1, timestamp, self.len)
            self.np_[chan2].add(s2, timestamp, self.len)
            self.nc[pair].add(s1, s2, self.len)

    def findMaximum(self, minDelay=-HUGE, maxDelay=HUGE, pair=None):
        return find_maximum(self.corr[self.last if pair is None else pair], self.sampleRate, minDelay, maxDelay, self.interpolate)


def run_batch(kind, X, nframes, sad, ts, pairs, sampleRate, fftLen, alpha=0.95, beta=0.5, q=0.3, interpolate=True, smooth=True,
              minDelay=-HUGE, maxDelay=HUGE, gcc=None):
    """the frame loop a driver runs: per utterance, per frame, per pair calculate() then findMaximum().  X [U][C][T][len].
    -> dict(result [U][T][P][3], valid [U][T][P], xspec [U][T][P][len], corr [U][T][P][fftLen], info [U][T][P] dicts, gcc [U] objects).
    gcc: the objects of an earlier block to continue from."""
    U, C, T, ln = X.shape; P = len(pairs)
    res = np.zeros((U, T, P, 3)); valid = np.zeros((U, T, P), np.int32)
    xs = np.zeros((U, T, P, ln), np.complex128); co = np.zeros((U, T, P, fftLen)); info = np.empty((U, T, P), object)
    objs = gcc if gcc is not None else [GCC(kind, sampleRate, fftLen, C, P, alpha, beta, q, interpolate) for _ in range(U)]
    for u in range(U):
        g = objs[u]
        for t in range(int(nframes[u])):
            for p, (c1, c2) in enumerate(pairs):
                g.calculate(X[u, c1, t], c1, X[u, c2, t], c2, p, float(ts[u, t]), bool(sad[u, t]), smooth)
                if g.valid[p]:
                    r = g.findMaximum(minDelay, maxDelay, p)
                    res[u, t, p] = (r["delay"], r["maxCorr"], r["ratio"]); info[u, t, p] = r
                valid[u, t, p] = g.valid[p]
                xs[u, t, p] = g.cross[p]; co[u, t, p] = g.corr[p]
    return dict(result=res, valid=valid, xspec=xs, corr=co, info=info, gcc=objs)


def channel_delays(pairs, pairDelays, chanN):
    """per-channel propagation delays tau with tau_0 = 0 from pair delays d_p = tau_c1 - tau_c2 (the peak of x1 conj(x2) sits at minus the
    lag of channel 2 behind channel 1), least squares over the pair graph"""
    A = np.zeros((len(pairs), chanN))
    for p, (a, b) in enumerate(pairs):
        A[p, a] += 1.0; A[p, b] -= 1.0
    sol = np.linalg.lstsq(A[:, 1:], np.asarray(pairDelays, np.float64), rcond=None)[0]
    return np.concatenate([[0.0], sol])


# ---- CCTDE --------------------------------------------------------------------------------------------------------------------------------
def hann(n):
    """getWindow(2, n) (modulated.cc:82-87)"""
    return 0.5 * (1 - np.cos((2.0 * np.pi * np.arange(n)) / float(n - 1)))


def cctde_cc(b1, b2, fftLen):
    """CCTDE::next's windowing and real FFTs, then detectPeaksOfCCFunction's phase-only cross-spectrum (:157-184) and scaled inverse FFT
    (:207).  The band-discard block (:186-205) is dead code and not restated."""
    w = hann(fftLen)
    s = []
    for b in (b1, b2):
        x = np.zeros(fftLen); b = np.asarray(b, np.float32)[:fftLen]
        x[:len(b)] = w[:len(b)] * b.astype(np.float64)
        s.append(np.fft.fft(x))
    n2 = fftLen // 2
    cc = np.zeros(fftLen, np.complex128)
    for j in range(0, n2 + 1):
        re0, im0, re1, im1 = s[0][j].real, s[0][j].imag, s[1][j].real, s[1][j].imag
        if j == 0 or j == n2:
            im0 = im1 = 0.0
        val = np.arctan2(im1, re1) - np.arctan2(im0, re0)
        cc[j] = np.cos(val) + 1j * np.sin(val)
        if 0 < j < n2:
            val = np.arctan2(-im1, re1) - np.arctan2(-im0, re0)
            cc[fftLen - j] = np.cos(val) + 1j * np.sin(val)
    return np.fft.ifft(cc).real


def cctde_peaks(cc, nHeld, sampleRate):
    """the N-best insertion (:210-254): rank 0 seeded with lag 0, `>` against the last held value, `>=` against the others;
    -> (delays seconds (through float, :241-252), sample delays, values)"""
    n = len(cc)
    args = [0] + [-1] * (nHeld - 1); vals = [cc[0]] + [-10e10] * (nHeld - 1)
    for i in range(1, n):
        c = cc[i]
        if c > vals[nHeld - 1]:
            for k in range(nHeld):
                if c >= vals[k]:
                    vals[k + 1:] = vals[k:nHeld - 1]; args[k + 1:] = args[k:nHeld - 1]
                    vals[k] = c; args[k] = i
                    break
    delays = np.zeros(nHeld); samp = np.zeros(nHeld, np.int64)
    for k in range(nHeld):
        a = args[k] if args[k] >= 0 else 2 ** 32 - 1                                  # maxArgs is unsigned: -1 wraps
        if a < n // 2:
            delays[k] = np.float32(a * 1.0 / sampleRate); samp[k] = a
        else:
            delays[k] = np.float32(np.float64(-(np.float32(n) - np.float32(a))) * 1.0 / sampleRate); samp[k] = -(n - a)
    return delays, samp, np.array(vals, np.float64)


def cctde(b1, b2, fftLen, nHeld, sampleRate):
    return cctde_peaks(cctde_cc(b1, b2, fftLen), nHeld, sampleRate)
