"""numpy restatement of the speech activity detectors of btk/sad/sad.{h,cc}: EnergyVADMetric, SimpleEnergyVAD, PowerSpectrumVADMetric,
NormalizedEnergyMetric, TSPSVADMetric, CCCVADMetric and the three hangover segmenters.  Line numbers are sad.cc's.

Every sum keeps the reference's order and the float / double of every intermediate; sums that are serial within a frame are vectorised
across frames only.  Carried state is kept in the layout the library documents (include/dsr.h section 7b): the energy history is a ring,
which is allowed because the reference only ever sorts it."""
import numpy as np

f64 = np.float64


# ---- EnergyVADMetric (:438-554) ----
def frame_energy(x):
    """fp64 sum of squares of the widened floats, i ascending (:486-490): x float32 [T][dim] -> [T]"""
    x = np.asarray(x, np.float32)
    s = np.zeros(x.shape[0], f64)
    for i in range(x.shape[1]):
        v = x[:, i].astype(f64)
        s = s + v * v
    return s


class EnergyVADMetric:
    def __init__(self, initialEnergy=5.0e+07, threshold=0.5, headN=4, tailN=10, energiesN=200):
        if not (0.0 <= threshold < 1.0) or energiesN < 1:
            raise ValueError("threshold %r / energiesN %r index past the sorted history" % (threshold, energiesN))
        self.initialEnergy, self.headN, self.tailN, self.energiesN = float(initialEnergy), int(headN), int(tailN), int(energiesN)
        self.medianIndex = int(threshold * energiesN)                     # unsigned(threshold * _energiesN), :443
        self.nextSpeaker()

    def reset(self):                                                      # :459-463: the history stays
        self.aboveN = self.belowN = 0; self.recognizing = False

    def nextSpeaker(self):                                                # :465-472
        self.reset(); self.hist = np.full(self.energiesN, self.initialEnergy, f64); self.pos = 0; self.updates = 0

    def state(self):
        """(history ring, (aboveThresholdN, belowThresholdN, recognizing, ring position))"""
        return self.hist.copy(), np.array([self.aboveN, self.belowN, int(self.recognizing), self.pos], np.int32)

    def _above(self, e, count_form=False):
        if count_form:
            above = int((self.hist < e).sum()) > self.medianIndex
        else:
            above = bool(e > np.sort(self.hist)[self.medianIndex])        # :492-493, :507
        if not self.recognizing and self.aboveN == 0:                     # :495, before this frame's counters change
            self.hist[self.pos] = e; self.pos = (self.pos + 1) % self.energiesN; self.updates += 1
        return above

    def step(self, e, count_form=False):                                  # next(), :521-554
        if self.recognizing:
            if self._above(e, count_form):
                self.belowN = 0; return 1.0
            self.belowN += 1
            if self.belowN == self.tailN:
                self.recognizing = False; self.aboveN = 0
            return 0.0
        if self._above(e, count_form):
            self.aboveN += 1
            if self.aboveN == self.headN:
                self.recognizing = True; self.belowN = 0
            return 1.0
        self.aboveN = 0
        return 0.0

    def run(self, x, count_form=False):
        """x float32 [T][dim] -> (decision [T], score [T])"""
        e = frame_energy(x)
        return np.array([self.step(v, count_form) for v in e], f64), e

    def energyPercentile(self, percentile):                               # :510-519
        if percentile < 0.0 or percentile > 100.0:
            raise ValueError("Percentile %g is out of range [0.0, 100.0]." % percentile)
        return np.sort(self.hist)[int((percentile / 100.0) * self.energiesN)] / self.energiesN


# ---- SimpleEnergyVAD (:159-199) ----
class SimpleEnergyVAD:
    def __init__(self, threshold, gamma):
        self.threshold, self.gamma, self.E = float(threshold), float(gamma), 0.0

    def nextSpeaker(self):
        self.E = 0.0

    def run(self, X):
        """X complex128 [T][fftLen] -> (decision [T] 1.0 / 0.0, score [T] = e / E)"""
        X = np.asarray(X, np.complex128)
        e = np.zeros(X.shape[0], f64)
        for k in range(X.shape[1]):
            e = e + (X[:, k].real * X[:, k].real + X[:, k].imag * X[:, k].imag)          # gsl_complex_abs2
        dec, score = np.zeros(len(e), f64), np.zeros(len(e), f64)
        with np.errstate(all="ignore"):
            for t, cur in enumerate(e):
                self.E = self.gamma * self.E + (1.0 - self.gamma) * cur
                score[t] = np.float64(cur) / np.float64(self.E)
                dec[t] = 1.0 if score[t] > self.threshold else 0.0
        return dec, score


# ---- MultiChannelVADMetric (:595-629) ----
def band(fftLen, sampleRate, lowCutoff=-1.0, highCutoff=-1.0):
    """(lowX, highX, binN); a cutoff at or above Nyquist raises as the reference does"""
    lowX, highX = 0, fftLen // 2
    if not lowCutoff < 0.0:
        if lowCutoff >= sampleRate / 2.0:
            raise ValueError("Low cutoff cannot be %10.1f" % lowCutoff)
        lowX = int((lowCutoff / sampleRate) * fftLen)
    if not highCutoff < 0.0:
        if highCutoff >= sampleRate / 2.0:
            raise ValueError("High cutoff cannot be %10.1f" % highCutoff)
        highX = int((highCutoff / sampleRate) * fftLen + 0.5)
    return lowX, highX, (2 * (highX - lowX + 1) if lowX > 0 else 2 * (highX - lowX) + 1)


def band_power(P, fftLen, lowX, highX):
    """P float32 [C][T][fftLen/2+1] -> [T][C] fp64: bin 0 once, every other bin -- the Nyquist bin too -- twice (:680-687)"""
    P = np.asarray(P, np.float32)
    p = np.zeros(P.shape[:2], f64)
    for b in range(lowX, highX + 1):
        v = P[:, :, b].astype(f64)
        p = p + (v if b == 0 else 2.0 * v)
    return np.ascontiguousarray((p / f64(fftLen)).T)


def power_metric(P, fftLen, lowX, highX, kind, E0=None):
    """kind 0 PowerSpectrumVADMetric (:660-705), 1 NormalizedEnergyMetric (:743-796), 2 TSPSVADMetric (:972-1024)
    -> (decision [T] +-1, powers [T][C], score [T])"""
    if E0 is None:
        E0 = 5000.0 if kind == 2 else 1.0
    pw = band_power(P, fftLen, lowX, highX)
    T, C = pw.shape
    total = np.zeros(T, f64)
    for c in range(C):
        total = total + (np.sqrt(pw[:, c]) if kind == 1 else pw[:, c])
    with np.errstate(all="ignore"):
        if kind == 0:
            score = pw[:, 0] / total; speech = score > E0 / f64(C)
        elif kind == 1:
            score = np.sqrt(pw[:, 0]) / total; speech = score > E0 / f64(C)
        else:
            tgt = pw[:, 0]; score = np.log(tgt / (total - tgt)) - np.log(E0 / total); speech = score > 0
    return np.where(speech, 1.0, -1.0), pw, score


# ---- CCCVADMetric (:815-959) ----
def _nbest(r, nCand, as_written=True):
    cc = [-1e10] * nCand; cc[0] = r[0]                                    # :881-886
    for k in range(1, len(r)):
        c = r[k]
        if c > cc[nCand - 1]:
            if as_written:                                                # :891-901: the store and the break sit outside the inner `if`
                if c > cc[0]:
                    cc[1:] = cc[:-1]
                cc[0] = c
            else:                                                         # what the comment above the loop promises: a sorted n-best list
                i = next(i for i in range(nCand) if c > cc[i])
                cc[i + 1:] = cc[i:-1]; cc[i] = c
    s = 0.0
    for v in cc:
        s += v
    return s / nCand


def ifft_radix2(z):
    """the inverse transform by decimation in time on a bit-reversed copy, stage by stage, then times 1 / n: another order of the same sums"""
    n = len(z); logn = n.bit_length() - 1
    assert 1 << logn == n
    rev = np.array([int(format(k, "0%db" % logn)[::-1], 2) for k in range(n)]) if logn else np.zeros(1, int)
    a = np.array(z, np.complex128)[rev]
    h = 1
    while h < n:
        w = np.exp(2j * np.pi * np.arange(h) / (2 * h))
        a = a.reshape(-1, 2 * h)
        t = a[:, h:] * w
        a = np.concatenate([a[:, :h] + t, a[:, :h] - t], axis=1).reshape(-1)
        h *= 2
    return a * (1.0 / n)


def ccc_metric(X, lowX, highX, nCand, threshold=0.1, as_written=True, stale_buffer=True, second_order=False):
    """X complex [C][T][fftLen] -> (decision [T], score [T]).  as_written / stale_buffer switch the two kept quirks off (for the tests that show
    they matter); second_order evaluates the inverse transform by ifft_radix2, for the near-threshold count."""
    X = np.asarray(X); C, T, N = X.shape
    X = X.astype(np.complex128)
    score = np.zeros(T, f64)
    with np.errstate(all="ignore"):
        for t in range(T):
            buf = np.zeros(N, np.complex128)                              # once a frame (:855)
            total = 0.0
            for c in range(1, C):
                if not stale_buffer:
                    buf[:] = 0.0
                for b in range(lowX, highX + 1):
                    v1, v2 = X[0, t, b], X[c, t, b]
                    x1, y1, x2, y2 = v1.real, -v1.imag, v2.real, v2.imag
                    cr, ci = x1 * x2 - y1 * y2, x1 * y2 + y1 * x2         # gsl_complex_mul(conj(val1), val2)
                    a = np.hypot(cr, ci)
                    pr, pi = np.float64(cr) / a, np.float64(ci) / a
                    buf[b] = complex(pr, pi)
                    if b > 0:
                        buf[N - b] = complex(pr, -pi)
                buf = ifft_radix2(buf) if second_order else np.fft.ifft(buf)
                total += _nbest(buf.real, nCand, as_written)
            score[t] = total / (C - 1)
    return np.where(score < threshold, 1.0, -1.0), score


# ---- HangoverVADFeature, HangoverMIVADFeature, HangoverMultiStageVADFeature (:1705-1945) ----
def hangover(dec, thresholds, headN, tailN, kind):
    """A literal walk of next() (:1767-1837) over the metrics' decisions dec [K][T].  kind 0 / 1 / 2: the base, MI and multi-stage decision
    logic.  Returns dict(start, length, consumed, codes [T] (_decisionMetric after each pulled source frame), emitted (source frame of every
    output frame), trace ((prefixN(), decisionMetric()) after every output frame))."""
    dec = np.asarray(dec, f64); K, T = dec.shape
    st = dict(code=0)
    codes = np.zeros(T, np.int32)

    def above(s):
        if kind == 0:
            r = bool(dec[0, s] > thresholds[0])                           # :1756-1765
        elif kind == 1:                                                   # :1853-1879
            if dec[0, s] < 0.5:
                st["code"] = -1; r = False
            elif dec[1, s] < 0.5:
                st["code"] = 2; r = True
            elif dec[2, s] > 0.5:
                st["code"] = 3; r = True
            else:
                st["code"] = -3; r = False
        else:                                                             # :1904-1945
            if K < 3:
                r = False
            elif dec[0, s] < 0.5:
                st["code"] = -1; r = False
            else:
                r = False
                for stage in range(1, K):
                    if dec[stage, s] > 0.5:
                        st["code"] = stage + 1; r = True
                        break
                if not r:
                    st["code"] = -K
        codes[s] = st["code"]
        return r

    prefixN = aboveN = belowN = bufferIndex = bufferedN = pulled = 0
    recognizing = False
    buf = [None] * headN
    emitted, trace = [], []
    frameX = -1
    while True:                                                           # one pass = one next(frameX + 1)
        fx = frameX + 1
        if recognizing:
            if bufferedN > 0:
                emitted.append(buf[bufferIndex]); bufferIndex = (bufferIndex + 1) % headN; bufferedN -= 1
            else:
                s = fx + (prefixN - headN)
                if s >= T:
                    break                                                 # the source's end of samples
                pulled = s + 1
                if above(s):
                    belowN = 0
                else:
                    belowN += 1
                    if belowN == tailN:
                        break
                emitted.append(s)
        else:
            ended = False
            while True:
                if prefixN >= T:
                    ended = True
                    break
                pulled = prefixN + 1
                buf[bufferIndex] = prefixN; bufferIndex = (bufferIndex + 1) % headN; bufferedN = min(headN, bufferedN + 1)
                a = above(prefixN); prefixN += 1
                if a:
                    aboveN += 1
                    if aboveN == headN:
                        recognizing = True
                        emitted.append(buf[bufferIndex]); bufferIndex = (bufferIndex + 1) % headN; bufferedN -= 1
                        break
                else:
                    aboveN = 0
            if ended:
                break
        frameX += 1
        trace.append((prefixN - headN, st["code"]))
    for t in range(pulled, T):
        codes[t] = 0
    return dict(start=prefixN - headN, length=len(emitted), consumed=pulled, codes=codes, emitted=emitted, trace=trace, last=(prefixN - headN, st["code"]))


def gather(x, start, length):
    """the emitted frames packed at the front of a zero array of x's shape"""
    y = np.zeros_like(x)
    y[:length] = x[start:start + length]
    return y


# ---- NegentropyVADMetric, MutualInformationVADMetric, LikelihoodRatioVADMetric (:1032-1640) ----
import ctypes
import ctypes.util
import math

# The bisection of _match stops where a difference falls below 1e-6, so its result depends on the last bits of lgamma / gamma: a different
# implementation can stop one step earlier or later and move the joint shape factor by 1e-6.  The product uses the C library's lgamma / tgamma
# (include/dsr.h section 7b); the restatement calls the same two functions rather than CPython's own.
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgamma.restype = _libm.tgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = _libm.tgamma.argtypes = [ctypes.c_double]


def _lgamma(x):
    return _libm.lgamma(x)


def _gamma(x):
    return _libm.tgamma(x)


class MatchError(ArithmeticError):
    """the bisection of _match (:1338-1369) did not converge; the reference would loop for ever"""


def _match_marginal(f):                                                   # :1312-1321
    Bc2 = math.exp(_lgamma(2.0 / f) - _lgamma(4.0 / f))
    return -(2.0 * ((2.0 / f) - math.log(f / (2.0 * math.pi * Bc2 * _gamma(2.0 / f)))))


def _match_joint(fJ):                                                     # :1323-1332
    BJ4 = math.exp((_lgamma(4.0 / fJ) - _lgamma(6.0 / fJ)) * 2.0)
    return -((4.0 / fJ) - math.log(fJ / (8.0 * math.pi * math.pi * BJ4 * _gamma(4.0 / fJ))))


def gg_match(f, cap=200):
    try:
        return _gg_match(f, cap)
    except (OverflowError, ValueError, ZeroDivisionError):                # where C's gamma returns inf and the comparison never holds
        raise MatchError("_match(%r) did not converge" % (f,))


def _gg_match(f, cap):
    a, c, match = f / 3.0, 2.0, _match_marginal(f)
    for _ in range(cap):
        b = (a + c) / 2.0
        rb = _match_joint(b)
        if abs(match - rb) < 1.0e-06:
            return b
        if rb > match:
            a = b
        else:
            c = b
    raise MatchError("_match(%r) did not converge in %d steps" % (f, cap))


class GGModel:
    """the host side of the three metrics: per bin (f, Bc, normalisation) of the marginal (:1038-1049), (fJ, BJ, normalisation) of the matched joint
    pdf (:1229-1246) and the fixed part of the decision threshold (:1399-1434)"""

    def __init__(self, shapeFactors, fftLen, lowX, highX, joint=True):
        self.fftLen, self.F, self.lowX, self.highX = fftLen, fftLen // 2 + 1, lowX, highX
        self.binN = 2 * (highX - lowX + 1) if lowX > 0 else 2 * (highX - lowX) + 1
        sf = [2.0] * self.F if shapeFactors is None else [float(v) for v in shapeFactors]
        assert len(sf) == self.F
        self.table = np.zeros((self.F, 6), f64)
        self.gauss = self._marginal(2.0)
        self.fixed = 0.0
        for b, f in enumerate(sf):
            Bc, nm = self._marginal(f)
            self.table[b, :3] = (f, Bc, nm)
            if joint:
                fJ = gg_match(f)
                BJ = math.exp((_lgamma(4.0 / fJ) - _lgamma(6.0 / fJ)) / 2.0)
                nJ = math.log(fJ / (8.0 * math.pi * math.pi * BJ * BJ * BJ * BJ * _gamma(4.0 / fJ)))
                self.table[b, 3:] = (fJ, BJ, nJ)
                thresh = 2.0 * ((2.0 / f) - math.log(f / (2.0 * math.pi * (Bc * Bc) * _gamma(2.0 / f))))
                thresh -= ((4.0 / fJ) - math.log(fJ / (8.0 * math.pi * math.pi * math.pow(BJ, 4.0) * _gamma(4.0 / fJ))))
                if lowX <= b <= highX:
                    self.fixed += thresh if b == 0 else 2.0 * thresh

    @staticmethod
    def _marginal(f):
        Bc = math.exp((_lgamma(2.0 / f) - _lgamma(4.0 / f)) / 2.0)
        return Bc, math.log(f / (2 * math.pi * Bc * Bc * _gamma(2.0 / f)))


def read_shape_factors(directory, fftLen):
    """the second token of the first line of <directory>/_M-%04d, one file a bin (:1077-1095)"""
    import os
    return [float(open(os.path.join(directory, "_M-%04d" % b)).readline().split(" ")[1]) for b in range(fftLen // 2 + 1)]


def _loglhood(absX, scale, f, Bc, nm):                                    # :1051-1058
    return nm - np.power(absX / (scale * Bc), f) - 2.0 * np.log(scale)


def _band_sum(model, terms):
    """the weighted bin sum, bins ascending (only bin 0 has weight 1), / binN; also the sum of the absolute weighted terms / binN"""
    s = np.zeros(terms.shape[0], f64); sa = np.zeros(terms.shape[0], f64)
    bins = range(model.lowX, model.highX + 1)
    for b in (reversed(bins) if getattr(model, "reverse", False) else bins):   # reverse: a second evaluation order, for the near-threshold count
        w = terms[:, b] if b == 0 else 2.0 * terms[:, b]
        s = s + w; sa = sa + np.abs(w)
    return s / model.binN, sa / model.binN


def negentropy(model, X, env, threshold=0.5):
    """X complex128 [T][fftLen], env float32 [T][>= F] -> (decision 1.0 / 0.0, score, sum |terms| / binN)"""
    F = model.F; aX = np.hypot(X[:, :F].real, X[:, :F].imag); sg = np.sqrt(env[:, :F].astype(f64))
    with np.errstate(all="ignore"):
        lr = _loglhood(aX, sg, model.table[:, 0], model.table[:, 1], model.table[:, 2]) - _loglhood(aX, sg, np.full(F, 2.0), model.gauss[0], model.gauss[1])   # the same pow as the bins': a Gaussian bin gives exactly 0
    score, sabs = _band_sum(model, lr)
    return np.where(score > threshold, 1.0, 0.0), score, sabs


def likelihood_ratio(model, X1, X2, env1, env2, threshold=0.0):
    """sigma = sqrt((env1 + env2) / 2) of the unrooted envelopes, as written (:1594-1599)"""
    F = model.F; sg = np.sqrt((env1[:, :F].astype(f64) + env2[:, :F].astype(f64)) / 2)
    f, Bc, nm = model.table[:, 0], model.table[:, 1], model.table[:, 2]
    with np.errstate(all="ignore"):
        m1 = _loglhood(np.hypot(X1[:, :F].real, X1[:, :F].imag), sg, f, Bc, nm); m2 = _loglhood(np.hypot(X2[:, :F].real, X2[:, :F].imag), sg, f, Bc, nm)
        a1 = np.abs(m1) + np.abs(m2)
    score, _ = _band_sum(model, m1 - m2)
    return np.where(score > threshold, 1.0, 0.0), score, _band_sum(model, a1)[1]


def mutual_information(model, X1, X2, env1, env2, rho, twiddle=-1.0, threshold=1.3, beta=0.95):
    """rho complex128 [F], used before it is updated and updated in place; -> (decision, score, threshold per frame, sum |terms| / binN, clamped)"""
    F = model.F; T = X1.shape[0]
    f, Bc, nm, fJ, BJ, nJ = (model.table[:, k] for k in range(6))
    score, thr, sabs = np.zeros(T, f64), np.zeros(T, f64), np.zeros(T, f64)
    clamped = 0
    with np.errstate(all="ignore"):
        for t in range(T):
            if twiddle < 0.0:
                thr[t] = threshold
            else:                                                         # _calcTotalThreshold (:1437-1454) from the rho before the frame
                tot = model.fixed
                for b in range(model.lowX, model.highX + 1):
                    th = -math.log(1.0 - (rho[b].real * rho[b].real + rho[b].imag * rho[b].imag))
                    tot += th if b == 0 else 2.0 * th
                thr[t] = tot * (twiddle / model.binN)
            x1, x2 = X1[t, :F], X2[t, :F]
            s1, s2 = np.sqrt(env1[t, :F].astype(f64)), np.sqrt(env2[t, :F].astype(f64))
            s12 = rho * (s1 * s2)
            det = s1 * s1 * s2 * s2 * (1.0 - (rho.real * rho.real + rho.imag * rho.imag))
            inv = 1.0 / det
            m00, m11, m01, m10 = (s2 * s2) * inv, (s1 * s1) * inv, -s12 * inv, -np.conj(s12) * inv
            y0, y1 = m00 * x1 + m01 * x2, m10 * x1 + m11 * x2             # zgemv
            s = np.conj(x1) * y0 + np.conj(x2) * y1                       # zdotc
            ssqrt = np.sqrt(np.hypot(s.real, s.imag))
            pj = np.power(ssqrt / (math.sqrt(2.0) * BJ), fJ); ld = np.log(det)
            a1, a2 = np.hypot(x1.real, x1.imag), np.hypot(x2.real, x2.imag)
            p1, p2 = np.power(a1 / (s1 * Bc), f), np.power(a2 / (s2 * Bc), f)
            mutual = (nJ - pj - ld) - (nm - p1 - 2.0 * np.log(s1)) - (nm - p2 - 2.0 * np.log(s2))
            mag = np.abs(nJ) + pj + np.abs(ld) + 2 * np.abs(nm) + p1 + p2 + 2.0 * np.abs(np.log(s1)) + 2.0 * np.abs(np.log(s2))
            sc, _ = _band_sum(model, mutual[None]); score[t] = sc[0]
            sabs[t] = _band_sum(model, mag[None])[1][0]
            cross = (x1 * np.conj(x2)) / (s1 * s2)
            new = rho * beta + cross * (1.0 - beta)
            an = np.hypot(new.real, new.imag)
            big = an >= (1.0 - 0.10)
            clamped += int(big.sum())
            new = np.where(big, new * ((1.0 - 0.10) / an), new)
            rho[:] = new
    return np.where(score > thr, 1.0, 0.0), score, thr, sabs, clamped


# ---- sadFeature.cc ----
f32 = np.float32


def _sigma(x):
    """norm() (:27-33): float products added to an fp64 sum; the root comes back as a float and normalize() widens it again (:35-39)"""
    n = np.zeros(x.shape[0], f64)
    for i in range(x.shape[1]):
        n = n + (x[:, i] * x[:, i]).astype(f64)
    return np.sqrt(n).astype(f32).astype(f64)


def energy_diffusion(x, second_order=False):
    """EnergyDiffusionFeature::next (:93-118): x float32 [T][dim] -> float32 [T]; second_order: log10 as ln / ln 10, for the ulp count"""
    x = np.asarray(x, f32); xd = x.astype(f64)
    norm = np.zeros(x.shape[0], f64)
    for j in range(x.shape[1]):
        norm = norm + xd[:, j] * xd[:, j]
    norm = np.sqrt(norm)
    diff = np.zeros(x.shape[0], f64)
    with np.errstate(all="ignore"):
        for j in range(x.shape[1]):
            nval = xd[:, j] / norm
            lg = np.log(nval) / np.log(10.0) if second_order else np.log10(nval)
            diff = diff - np.where(nval > 0.0, nval * lg, 0.0)
    return diff.astype(f32)


def band_ratio_index(dim, sampleRate, threshF=0.0):
    mx = f32(f32(sampleRate) / 2.0); df = f32(mx / f32(dim)); tf = f32(threshF) if threshF > 0.0 else f32(mx / f32(2.0))   # :124-125
    return int(np.floor(f32(tf / df)))


def band_energy_ratio(x, sampleRate, threshF=0.0):
    """BandEnergyRatioFeature::next (:129-153): float sums"""
    x = np.asarray(x, f32); tx = band_ratio_index(x.shape[1], sampleRate, threshF)
    lo, hi = np.zeros(x.shape[0], f32), np.zeros(x.shape[0], f32)
    for j in range(tx):
        lo = lo + x[:, j] * x[:, j]
    for j in range(tx, x.shape[1]):
        hi = hi + x[:, j] * x[:, j]
    with np.errstate(all="ignore"):
        return np.sqrt(lo / hi)


def negative_entropy(x, second_order=False):
    """NegativeEntropyFeature::next (:205-243); second_order: ln cosh z as |z| + log1p(exp(-2|z|)) - ln 2, for the ulp count"""
    x = np.asarray(x, f32); w = np.abs(x); n = x.shape[1]
    s, ss = np.zeros(x.shape[0], f64), np.zeros(x.shape[0], f64)
    for j in range(n):
        s = s + w[:, j].astype(f64); ss = ss + (w[:, j] * w[:, j]).astype(f64)
    with np.errstate(all="ignore"):
        mean = s / f64(n); dev = np.sqrt(ss / f64(n - 1) - mean * mean)
        g = np.zeros(x.shape[0], f64)
        for j in range(n):
            z = ((w[:, j].astype(f64) - mean) / dev).astype(f32).astype(f64)
            g = g + (np.abs(z) + np.log1p(np.exp(-2.0 * np.abs(z))) - np.log(2.0) if second_order else np.log(np.cosh(z)))
        EGy = g / f64(n)
        return (100.0 * (EGy - 0.374576) * (EGy - 0.374576)).astype(f32)


def significant_subbands(x, thresh=0.0):
    """SignificantSubbandsFeature::next (:253-274)"""
    x = np.asarray(x, f32); sigma = _sigma(x)
    with np.errstate(all="ignore"):
        w = (x.astype(f64) / sigma[:, None]).astype(f32)
    return (w > f32(thresh)).sum(axis=1).astype(f32)


def ulps(a, b):
    """the distance of two float32 arrays in units in the last place (NaN against NaN: 0)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia); ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(ia - ib))


def differing(a, b):
    """elements whose bits differ; a NaN equals a NaN of any payload"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind in "iub":
        return int((a != b).sum())
    iv = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    same = (np.ascontiguousarray(a).view(iv) == np.ascontiguousarray(b).view(iv)) | (np.isnan(a) & np.isnan(b))
    return int((~same).sum())
