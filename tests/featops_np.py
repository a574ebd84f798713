"""numpy restatement of the scalar feature operators of btk/feature/feature.{h,cc}: SignalPower, ZeroCrossingRateHamming, YINPitch, SpikeFilter,
SpikeFilter2, ALog, Normalize, Threshold, Amplification, SpectralResampling and SphinxMel.

Every intermediate has the type the reference's C++ gives it (numpy float32 arithmetic rounds at every operation and does not contract); the
libm functions of the host-side designs (cos, log10, pow) are Python's math module, i.e. the C library's, as in the reference.  Two places where
the C++ types decide the bits:
  * ALogFeature::next: `double val = b + x` adds two floats, so the sum is rounded to fp32 before it is widened (feature.cc:1395-1398);
  * SpikeFilter2::next: in `(1.0 - lambda) * a + lambda * b` the second product is float * float, rounded to fp32, the first one and the sum
    are fp64 (feature.cc:3761-3762)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
HUGE = float(np.finfo(np.float32).max)          # <math.h> HUGE = 3.40282347e+38F
ADC_RANGE = float(f32(65536.0) * f32(65536.0)) / 4.0


# ---- SignalPowerFeature::next (feature.cc:1360-1378) ----
def signal_power(x):
    """x [T][N] float32 -> [T][1] float32"""
    x = np.asarray(x, f32)
    T, N = x.shape
    p = np.zeros(T, f64)
    for i in range(N):
        v = x[:, i].astype(f64)
        p = p + v * v
    return (p / f64(N) / f64(ADC_RANGE)).astype(f32)[:, None]


# ---- ZeroCrossingRateHammingFeature (feature.cc:3545-3577) ----
def hamming_zcr_window(N):
    if N < 2:
        return np.full(N, np.nan)
    temp = 2.0 * math.pi / float(N - 1)
    return np.array([0.54 - 0.46 * math.cos(temp * i) for i in range(N)], f64)


def zero_crossing_rate(x):
    x = np.asarray(x, f32)
    T, N = x.shape
    w = hamming_zcr_window(N)
    s = np.where(x >= 0, 1, -1).astype(np.int32)        # -0.0 >= 0 holds
    total = np.zeros(T, f32)
    for i in range(N - 1):
        c = (np.abs(s[:, i + 1] - s[:, i]) // 2).astype(f64)
        total = (total.astype(f64) + c * w[i]).astype(f32)
    return (total / f32(N))[:, None]


# ---- YINPitchFeature (feature.cc:3584-3634) ----
def yin_difference(x, variant="ref"):
    """d [T][W]: d[:, tau] for tau = 1..W-1 (column 0 unused).  variant "ref": fp32, j ascending, rounded after the subtraction, the multiply
    and the add; "f64": fp64 accumulator rounded once; "four": four fp32 partial sums over j mod 4, added at the end."""
    x = np.asarray(x, f32)
    T, N = x.shape
    W = N // 2
    d = np.zeros((T, W), f32)
    if W < 2:
        return d
    if variant == "ref":
        for j in range(W):
            tmp = x[:, j, None] - x[:, j + 1:j + W]
            d[:, 1:] = d[:, 1:] + tmp * tmp
    elif variant == "f64":
        acc = np.zeros((T, W - 1), f64)
        for j in range(W):
            tmp = (x[:, j, None] - x[:, j + 1:j + W])
            acc += (tmp * tmp).astype(f64)
        d[:, 1:] = acc.astype(f32)
    elif variant == "four":
        part = np.zeros((4, T, W - 1), f32)
        for j in range(W):
            tmp = x[:, j, None] - x[:, j + 1:j + W]
            part[j % 4] = part[j % 4] + tmp * tmp
        d[:, 1:] = (part[0] + part[1]) + (part[2] + part[3])
    else:
        raise KeyError(variant)
    return d


def yin_pitch(x, samplerate=16000, threshold=0.5, variant="ref", details=False):
    """-> pitch [T][1] float32, value [T] float32 (y at the lag where _getPitch returned, y(W-1) when it ran to the end); with details also
    the lag tau of the hit (0: none)"""
    x = np.asarray(x, f32)
    T, N = x.shape
    W = N // 2
    tol = f32(threshold)
    with np.errstate(all="ignore"):
        d = yin_difference(x, variant)
        y = np.ones((T, max(W, 1)), f32)
        tmp2 = np.zeros(T, f32)
        for tau in range(1, W):
            tmp2 = tmp2 + d[:, tau]
            y[:, tau] = d[:, tau] * f32(tau) / tmp2
        hit = np.zeros((T, max(W, 1)), bool)
        if W > 1:
            hit[:, 1:] = (y[:, 1:] < tol) & (y[:, :-1] < y[:, 1:])
    anyhit = hit.any(axis=1)
    tau = np.where(anyhit, hit.argmax(axis=1), 0)
    lag = np.where(anyhit, tau - 1, 0)
    pitch = np.zeros(T, f32)
    pos = lag > 0
    pitch[pos] = (f64(samplerate) / lag[pos].astype(f64)).astype(f32)
    value = np.where(anyhit, y[np.arange(T), tau], y[:, max(W, 1) - 1]).astype(f32)
    if details:
        return pitch[:, None], value, tau
    return pitch[:, None], value


# ---- SpikeFilter::next (feature.cc:3656-3696) ----
def spike_filter(x, tapN):
    """the reference's own loop: insertion sort of the window, the delay queue; what it never writes stays at the vector's zeros"""
    x = np.asarray(x, f32)
    T, n = x.shape
    if tapN < 3:
        raise ValueError("tapN should be at least 3.")
    if n < tapN:
        raise ValueError("Cannot filter with adcN = %d and tapN = %d." % (n, tapN))
    if tapN % 2 == 0:
        raise ValueError("even tapN reads past the block")
    q = (tapN - 1) >> 1
    out = np.zeros((T, n), f32)
    for t in range(T):
        adc = x[t]
        queue = [adc[i] for i in range(q)]
        pnt = 0
        for adcX in range(q, n - q):
            window = []
            for wX in range(tapN):
                window.append(adc[adcX + wX - q])
                i, j = wX, wX - 1
                while j >= 0 and window[j] > window[i]:
                    window[i], window[j] = window[j], window[i]
                    i = j
                    j -= 1
            out[t, adcX - q] = queue[pnt]
            queue[pnt] = window[q]
            pnt = (pnt + 1) % q
    return out


# ---- SpikeFilter2 (feature.cc:3701-3776) ----
class SpikeFilter2:
    def __init__(self, width=3, maxslope=7000.0, startslope=100.0, thresh=15.0, alpha=0.2):
        self.width = int(width); self.maxslope = f32(maxslope); self.startslope = f32(startslope); self.thresh = f32(thresh)
        self.alpha = f32(alpha); self.beta = f32(1.0 - float(f32(alpha)))
        self.reset()

    def reset(self):
        self.meanslope = f32(self.startslope); self.count = 0

    def next(self, adc):
        v = np.array(adc, f32)
        n = v.size
        P, Q = 0, 1
        signE = 0
        while Q < n:
            slope = f32(v[Q] - v[P])
            if slope < 0.0:
                slope = f32(slope * f32(-1)); signB = -1
            else:
                signB = 1
            P = Q; Q += 1
            mx = f32(self.thresh * self.meanslope)
            if slope > mx and slope > self.maxslope:
                spikeB = P - 1
                spikeN = 0
                while Q < n and spikeN < self.width:
                    slope = f32(v[Q] - v[P])
                    if slope < 0:
                        slope = f32(f32(-1) * slope); signE = -1
                    else:
                        signE = 1
                    P = Q; Q += 1
                    spikeN += 1
                    if signB != signE and slope > mx and slope > self.maxslope:
                        break
                spikeE = P
                for sX in range(spikeB + 1, spikeE):
                    lam = f32(f32(sX - spikeB) / f32(spikeE - spikeB))
                    v[sX] = f32((1.0 - f64(lam)) * f64(v[spikeB]) + f64(f32(lam * v[spikeE])))
                self.count += 1
            else:
                self.meanslope = f32(f32(self.beta * self.meanslope) + f32(self.alpha * slope))
        return v

    def run(self, x):
        return np.stack([self.next(r) for r in np.asarray(x, f32)]) if len(x) else np.zeros((0, 0), f32)


# ---- ALogFeature / NormalizeFeature (feature.cc:1383-1514) ----
class _MinMax:
    def __init__(self, runon):
        self.runon = bool(runon); self.nextSpeaker()

    def nextSpeaker(self):
        self.mn, self.mx = f64(HUGE), f64(-HUGE)

    def _scan(self, block):
        for v in np.asarray(block, f32).reshape(-1):
            v = f64(v)
            if v < self.mn: self.mn = v
            if v > self.mx: self.mx = v

    def bounds(self, x):
        """per frame (min, max) as the operator holds them when it processes that frame; batch mode: reset() then the whole utterance"""
        x = np.asarray(x, f32)
        if not self.runon:
            self.nextSpeaker(); self._scan(x)
            return [(self.mn, self.mx)] * len(x)
        out = []
        for r in x:
            self._scan(r); out.append((self.mn, self.mx))
        return out


class ALog(_MinMax):
    def __init__(self, m=1.0, a=4.0, runon=False):
        _MinMax.__init__(self, runon); self.m, self.a = f64(m), f64(a)

    def run(self, x):
        """x [T][dim] -> [T][1] (the reference's constructor gives the operator size 1; min and max go over the whole source frame)"""
        x = np.asarray(x, f32)
        out = np.zeros((len(x), 1), f32)
        with np.errstate(all="ignore"):
            for t, (mn, mx) in enumerate(self.bounds(x)):
                b = f32(mx / math.pow(10.0, float(self.a)))
                val = f64(f32(b + x[t, 0]))
                if val <= 0.0:
                    val = f64(1.0)
                out[t, 0] = f32(self.m * f64(math.log10(float(val))))
        return out


class Normalize(_MinMax):
    def __init__(self, ymin=0.0, ymax=1.0, runon=False):
        _MinMax.__init__(self, runon); self.ymin, self.ymax = f64(ymin), f64(ymax); self.range = self.ymax - self.ymin

    def run(self, x):
        x = np.asarray(x, f32)
        out = np.zeros(x.shape, f32)
        with np.errstate(all="ignore"):
            for t, (mn, mx) in enumerate(self.bounds(x)):
                xrange = mx - mn
                factor = self.range / xrange
                add = self.ymin - mn * factor
                out[t] = (x[t].astype(f64) * factor + add).astype(f32)
        return out


# ---- ThresholdFeature / AmplificationFeature (feature.cc:1519-1560, 3927-3941) ----
def threshold(x, value=0.0, thresh=1.0, mode="upper"):
    compare = {"upper": 1, "lower": -1, "both": 0}[mode]
    v = np.asarray(x, f32).astype(f64)
    value, thresh = f64(value), f64(thresh)
    if compare > 0:
        v = np.where(v >= thresh, value, v)
    elif compare == 0:
        v = np.where(v >= thresh, value, np.where(v <= -thresh, -value, v))
    else:
        v = np.where(v <= thresh, value, v)
    return v.astype(f32)


def amplify(x, amplify=1.0):
    return (np.asarray(x, f32).astype(f64) * f64(amplify)).astype(f32)


# ---- SpectralResamplingFeature (feature.cc:1565-1602) ----
SAMPLE_RATIO = 16.0 / 22.05


def spectral_resample_table(srcN, ratio=SAMPLE_RATIO, length=0):
    """-> (low [outN] int, wgt [outN] float32); raises as the constructor does, and where a term past the source's end would carry weight"""
    outN = srcN if length == 0 else int(length)
    r = f64(ratio) * f64(f32(srcN)) / f64(f32(outN))
    if r > 1.0:
        raise ValueError("Must resample the spectrum to a higher rate (ratio = %10.4f < 1.0)." % r)
    low = np.zeros(outN, np.int64); wgt = np.zeros(outN, f32)
    for c in range(outN):
        exact = f32(f64(c) * r)
        lo = int(f64(c) * r)
        hi = lo + 1
        w = f32(f32(hi) - exact)
        if lo >= srcN or (hi >= srcN and (1.0 - float(w)) != 0.0):
            raise IndexError("coefficient %d reads source element %d of %d" % (c, hi, srcN))
        low[c], wgt[c] = lo, w
    return low, wgt


def spectral_resample(x, ratio=SAMPLE_RATIO, length=0):
    x = np.asarray(x, f64)
    T, srcN = x.shape
    low, wgt = spectral_resample_table(srcN, ratio, length)
    xp = np.concatenate([x, np.zeros((T, 1), f64)], axis=1)
    w = wgt.astype(f64)
    coeff = (w * xp[:, low] + (1.0 - w) * xp[:, low + 1]).astype(f32)
    return coeff.astype(f64)


# ---- SphinxMelFeature (feature.cc:2303-2385) ----
def sphinx_mel_filters(fftN=512, powerN=257, sampleRate=16000.0, lowerF=0.0, upperF=0.0, filterN=30):
    sampleRate = float(f32(sampleRate)); lowerF = float(f32(lowerF)); upperF = float(f32(upperF))
    A = np.zeros((filterN, powerN), f64)
    dfreq = sampleRate / fftN
    if upperF > sampleRate / 2:
        raise ValueError("Upper frequency %f exceeds Nyquist %f" % (upperF, sampleRate / 2.0))
    mel = lambda f: 2595.0 * math.log10(1.0 + (f / 700.0))
    inv = lambda m: 700.0 * (math.pow(10.0, m / 2595.0) - 1.0)
    melmax, melmin = mel(upperF), mel(lowerF)
    dmelbw = (melmax - melmin) / (filterN + 1)
    edges = [inv(melmin + dmelbw * n) for n in range(filterN + 2)]
    for fX in range(filterN):
        left, center, right = edges[fX], edges[fX + 1], edges[fX + 2]
        for k in range(1, powerN):
            hz = k * dfreq
            if hz < left:
                continue
            if hz > right:
                break
            with np.errstate(all="ignore"):
                lv = f64(hz - left) / f64(center - left)
                rv = f64(right - hz) / f64(right - center)
            A[fX, k] = rv if rv < lv else lv              # std::min(left_value, right_value)
    return A


def sphinx_mel_apply(A, x):
    """row-major dgemv: temp = 0; temp += x[k] * A[i][k], k ascending"""
    x = np.asarray(x, f64)
    out = np.zeros((x.shape[0], A.shape[0]), f64)
    for k in range(A.shape[1]):
        out = out + x[:, k, None] * A[None, :, k]
    return out
