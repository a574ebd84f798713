"""numpy restatement of btk/postfilter/spectralsubtraction.{h,cc} and binauralprocessing.{h,cc}: fp64 throughout, np.float32 where the
reference holds a `float`.  Written from the behaviour; the line numbers are those of the reference files.  Inputs are frames of
fftLen/2+1 bins (what the analysis banks leave in memory); outputs are fftLen/2+1 bins unless `full` asks for the fftLen-bin row with the
upper half as the reference leaves it."""
import numpy as np

f32 = np.float32


def abs2(x):
    x = np.asarray(x, np.complex128)
    return x.real * x.real + x.imag * x.imag                                  # gsl_complex_abs2


def upper_mirror(row, M, lo=1):
    """fftLen-bin row from bins 0..M/2: conj mirror for lo <= f < M/2, zero elsewhere in the upper half"""
    out = np.zeros(M, np.complex128); out[:M // 2 + 1] = row
    for f in range(lo, M // 2):
        out[M - f] = np.conj(row[f])
    return out


class AveragePSD:
    """averagePSDEstimator (spectralsubtraction.cc:52-129)"""

    def __init__(self, fftLen2, alpha=-1.0):
        self.est = np.zeros(fftLen2 + 1); self.alpha = float(alpha); self.seen = False; self.samples = []

    def addSample(self, x):
        p = abs2(x[:self.est.size])
        if self.alpha < 0:
            self.samples.append(p)                                            # :100-102
        elif not self.seen:
            self.est = p.copy(); self.seen = True                             # :104-107
        else:
            self.est = self.est * self.alpha + p * (1.0 - self.alpha)         # :108-112: two scalings, one addition

    def average(self):
        if self.alpha < 0:                                                    # :70-87
            s = np.zeros_like(self.est)
            for p in self.samples:
                s = s + p
            with np.errstate(all="ignore"):
                self.est = s * (np.float64(1.0) / np.float64(len(self.samples)))
        return self.est

    def clearSamples(self):
        self.samples = []

    def clear(self):
        self.seen = False; self.samples = []


class SpectralSubtractor:
    """SpectralSubtractor (spectralsubtraction.cc:141-267)"""

    def __init__(self, fftLen, ft=1.0, flooringV=0.001):
        self.M = fftLen; self.ft = f32(ft); self.floor = f32(flooringV); self.training = True; self.subtract = False; self.psd = []

    def setChannel(self, alpha=-1.0):
        self.psd.append(AveragePSD(self.M // 2, alpha))

    def stopTraining(self):
        self.training = False
        for p in self.psd:
            p.average()

    def next(self, frames):
        """frames [C][F] of one time step -> [F]"""
        F = self.M // 2 + 1; acc = np.zeros(F, np.complex128)
        for c, x in enumerate(frames):
            x = np.asarray(x, np.complex128)
            if self.training:
                self.psd[c].addSample(x)                                      # :209-212: the sample first
            if not self.subtract:
                acc = x + acc                                                 # :213-215
            else:
                N2 = self.psd[c].est
                th = np.arctan2(x.imag, x.real); S2 = abs2(x) - np.float64(self.ft) * N2
                S2 = np.where(S2 <= np.float64(self.floor), np.float64(self.floor), S2)          # :250-252
                r = np.sqrt(S2)
                acc = (r * np.cos(th) + 1j * (r * np.sin(th))) + acc          # gsl_complex_polar, then + tmp
        return acc * (1.0 / float(len(frames)))                               # :264

    def run(self, X, full=False):
        """X [C][T][F] -> [T][F] (or [T][M])"""
        out = [self.next(X[:, t]) for t in range(X.shape[1])]
        out = np.array(out).reshape(X.shape[1], self.M // 2 + 1)
        return np.array([upper_mirror(r, self.M) for r in out]).reshape(X.shape[1], self.M) if full else out


class WienerFilter:
    """WienerFilter (spectralsubtraction.cc:269-347); frames counts the object's life, reset() does not touch it"""

    def __init__(self, fftLen, alpha=0.0, flooringV=0.001, beta=1.0):
        self.M = fftLen; self.alpha = f32(alpha); self.floor = f32(flooringV); self.beta = f32(beta); self.update = True
        F = fftLen // 2 + 1; self.PSDs = np.zeros(F); self.PSDn = np.zeros(F); self.frames = 0

    def next(self, S, N):
        S = np.asarray(S, np.complex128); F = self.M // 2 + 1
        a = np.float64(self.alpha) if self.frames >= 2 else 0.0               # _frameX > 0 (:302-305)
        out = np.zeros(F, np.complex128); out[0] = S[0]
        PSDs = a * self.PSDs[1:] + (1 - a) * abs2(S[1:])
        if self.update:
            cur = abs2(np.asarray(N, np.complex128)[1:]); cur = np.where(cur < np.float64(self.floor), np.float64(self.floor), cur)
            PSDn = a * self.PSDn[1:] + (1 - a) * cur
            self.PSDn[1:] = PSDn
        else:
            PSDn = self.PSDn[1:]
        with np.errstate(all="ignore"):
            H = PSDs / (PSDs + np.float64(self.beta) * PSDn)
        out[1:] = S[1:].real * H + 1j * (S[1:].imag * H)
        out[F - 1] = np.conj(out[F - 1])                                      # :330-331: the mirror of M/2 is M/2
        self.PSDs[1:] = PSDs; self.frames += 1
        return out

    def run(self, S, N):
        return np.array([self.next(S[t], None if N is None else N[t]) for t in range(S.shape[0])]).reshape(S.shape[0], self.M // 2 + 1)


def calc_itd(M, L, R):
    """calcITDf (binauralprocessing.cc:12-33) for all bins of a frame (bin 0 divides by zero: IEEE)"""
    L = np.asarray(L, np.complex128); R = np.asarray(R, np.complex128)
    aL = np.arctan2(L.imag, L.real); aR = np.arctan2(R.imag, R.real)
    d1 = np.abs(aL - aR); d2 = np.abs(aL - aR - 2 * np.pi); d3 = np.abs(aL - aR + 2 * np.pi)
    d = np.where(d1 < d2, d1, d2); d = np.where(d3 < d, d3, d)
    with np.errstate(all="ignore"):
        return d / (2 * np.pi * np.arange(L.size) / M)


class MaskFilter:
    """kind 0 BinaryMaskFilter, 1 KimBinaryMaskFilter, 2 IIDBinaryMaskFilter (binauralprocessing.cc:47-211, 431-520)"""

    def __init__(self, kind, chanX, M, threshold, alpha, dEta=0.01):
        self.kind = kind; self.chanX = chanX; self.M = M; self.threshold = f32(threshold); self.alpha = f32(alpha); self.dEta = f32(dEta)
        self.prevMu = np.ones(M // 2 + 1, f32); self.thr = None

    def setThresholds(self, th):
        if self.thr is None:
            self.thr = np.zeros(self.M // 2 + 1)                              # :88-90 only allocates (zeros stand for the uninitialised memory)
        else:
            self.thr[1:] = np.asarray(th, np.float64)[1:self.M // 2 + 1]

    def next(self, L, R):
        """-> (out [F], mu [F] float32, sides (a, b) of the predicate a <= b per bin)"""
        F = self.M // 2 + 1; L = np.asarray(L, np.complex128); R = np.asarray(R, np.complex128)
        out = np.zeros(F, np.complex128); mu = np.zeros(F, f32); a = np.zeros(F); b = np.ones(F)
        if self.kind == 0:
            return out, mu, (a, b)
        out[0] = L[0]; mu[0] = self.prevMu[0]
        oma = f32(1) - self.alpha; omaEta = oma * self.dEta                   # float arithmetic (:152-161, :470-473)
        if self.kind == 1:
            a = calc_itd(self.M, L, R); b = np.full(F, np.float64(self.threshold))
            with np.errstate(all="ignore"):
                le = a <= b
            passing = le if self.chanX == 0 else ~le; X = L if self.chanX == 0 else R
        else:
            thr = np.full(F, self.threshold, f32) if self.thr is None else self.thr.astype(f32)   # :456-457 rounds to float
            X, I = (L, R) if self.chanX == 0 else (R, L)
            a = np.hypot(X.real, X.imag); b = np.hypot(I.real, I.imag) + thr.astype(np.float64)
            passing = ~(a <= b)
            if self.thr is not None:
                self.threshold = thr[F - 1]
        m = (self.alpha * self.prevMu).astype(f32) + np.where(passing, oma, omaEta).astype(f32)
        mu[1:] = m[1:].astype(f32); self.prevMu[1:] = mu[1:]
        out[1:] = X[1:].real * mu[1:].astype(np.float64) + 1j * (X[1:].imag * mu[1:].astype(np.float64))
        return out, mu, (a, b)

    def run(self, L, R, full=False):
        T = L.shape[0]; F = self.M // 2 + 1
        o = np.zeros((T, F), np.complex128); m = np.zeros((T, F), f32); A = np.zeros((T, F)); B = np.ones((T, F))
        for t in range(T):
            o[t], m[t], (A[t], B[t]) = self.next(L[t], R[t])
        if full:
            o = np.array([upper_mirror(r, self.M) for r in o]).reshape(T, self.M)
        return o, m, (A, B)


def candidates(kind, minTh, maxTh, width):
    """-> (table float32 [nLoop], nCand): the float loop of accumStats1 and the arrays' length (binauralprocessing.cc:251-269, 321, 721-731)"""
    minTh, maxTh, width = f32(minTh), f32(maxTh), f32(width)
    if minTh == maxTh:
        minTh, maxTh = (f32(-100000), f32(100000)) if kind == 2 else (f32(-0.2 * 16000 / 340), f32(0.2 * 16000 / 340))
    nCand = int(np.float64(f32(f32(maxTh - minTh) / width)) + 1.5)
    tab = []; th = minTh
    while th <= maxTh:
        tab.append(th); th = f32(th + width)
        if len(tab) > nCand:
            raise IndexError("the loop yields more than nCand = %d candidates" % nCand)
    return np.array(tab, f32), nCand


def bin_range(M, minFreq, maxFreq, sampleRate):
    if minFreq < 0 or maxFreq < 0 or sampleRate < 0:                          # :260-267
        return 1, M // 2 + 1
    return int(f32(f32(f32(M) * f32(minFreq)) / f32(sampleRate))), int(f32(f32(f32(M) * f32(maxFreq)) / f32(sampleRate)))


class ThresholdEstimator:
    """kind 0 KimITDThresholdEstimator, 1 IIDThresholdEstimator, 2 FDIIDThresholdEstimator (binauralprocessing.cc:232-426, 525-683, 702-928).
    Accumulator layout as in include/dsr.h (dsr_thest_acc_doubles)."""

    def __init__(self, kind, M, minTh=0.0, maxTh=0.0, width=0.02, minFreq=-1, maxFreq=-1, sampleRate=-1, dEta=0.01, dPowerCoeff=0.0):
        self.kind = kind; self.M = M; self.F = M // 2 + 1; self.cand, self.nCand = candidates(kind, minTh, maxTh, width)
        self.f0, self.f1 = (1, self.F) if kind == 2 else bin_range(M, minFreq, maxFreq, sampleRate)
        self.eta = np.float64(f32(dEta)); self.pc = np.float64(f32(dPowerCoeff)); self.beta = 3.0
        self.nacc = (5, 6, 3)[kind]
        self.acc = np.zeros((self.nacc, self.F, self.nCand) if kind == 2 else (self.nacc, self.nCand)); self.nSamples = 0

    def sides(self, L, R):
        """the two sides (a <= b) of every predicate of one frame: list of (a [bins], b [bins][nLoop])"""
        th = self.cand.astype(np.float64)[None, :]
        if self.kind == 0:
            itd = calc_itd(self.M, L, R)[self.f0:self.f1]
            return [(itd, np.broadcast_to(th, (itd.size, th.size)))]
        PT = np.hypot(L.real, L.imag)[self.f0:self.f1]; PI = np.hypot(R.real, R.imag)[self.f0:self.f1]
        return [(PT, PI[:, None] + th), (PI, PT[:, None] + th)]

    def accum(self, L, R):
        """the literal loops of accumStats1, vectorised over candidates only where the reference's order of additions is kept: the sums over
        bins run in bin order"""
        L = np.asarray(L, np.complex128); R = np.asarray(R, np.complex128); eta = self.eta; nL = self.cand.size
        th = self.cand.astype(np.float64)
        if self.kind == 0:
            itd = calc_itd(self.M, L, R); PT = np.zeros(nL); PI = np.zeros(nL)
            for f in range(self.f0, self.f1):
                with np.errstate(all="ignore"):
                    le = itd[f] <= th
                muT = np.where(le, 1.0, eta); muI = np.where(le, eta, 1.0)
                PT = PT + ((L[f].real * muT) ** 2 + (L[f].imag * muT) ** 2); PI = PI + ((R[f].real * muI) ** 2 + (R[f].imag * muI) ** 2)
            RT = np.power(PT, self.pc); RI = np.power(PI, self.pc)
            for q, v in enumerate((RT * RI, RT, RI, RT * RT, RI * RI)):
                self.acc[q, :nL] += v
        else:
            e2 = 2.0 * self.pc
            s = np.zeros((6, nL))
            for f in range(self.f0, self.f1):
                PT = np.hypot(L[f].real, L[f].imag); PI = np.hypot(R[f].real, R[f].imag)
                muT = np.where(PT <= (PI + th), eta, 1.0); muI = np.where(PI <= (PT + th), eta, 1.0)
                y1T = np.power(np.hypot(L[f].real * muT, L[f].imag * muT), e2); y1I = np.power(np.hypot(R[f].real * muI, R[f].imag * muI), e2)
                y2T = y1T * y1T; y2I = y1I * y1I
                if self.kind == 1:
                    for q, v in enumerate((y1T, y1I, y2T, y2I, y2T * y2T, y2I * y2I)):
                        s[q] = s[q] + v
                else:
                    self.acc[0, f, :nL] += y2T * y2T + y2I * y2I; self.acc[1, f, :nL] += y1T + y1I; self.acc[2, f, :nL] += y2T + y2I
            if self.kind == 1:
                self.acc[:, :nL] += s
        self.nSamples += 1

    def run(self, L, R):
        for t in range(L.shape[0]):
            self.accum(L[t], R[t])
        return self

    def flat(self):
        return np.concatenate([self.acc.ravel(), [float(self.nSamples)]])


def calc_threshold(kind, cand, nCand, F, flat, beta=3.0):
    """calcThreshold from the flat accumulators (pure) -> (threshold, index, cost, rho, thresholdsAtFreq or None)"""
    nL = cand.size; n = flat[-1]
    with np.errstate(all="ignore"):
        if kind == 0:
            a = flat[:-1].reshape(5, nCand)[:, :nL]
            mT = a[1] / n; mI = a[2] / n; sT = a[3] / n - mT * mT; sI = a[4] / n - mI * mI; c = a[0] / n
            rho = np.abs((c - mT * mI) / (np.sqrt(sT) * np.sqrt(sI)))
        elif kind == 1:
            a = flat[:-1].reshape(6, nCand)[:, :nL]
            sig2 = a[2] / n + a[3] / n; c = (a[4] / n + a[5] / n) - beta * sig2 * sig2; rho = -c
        else:
            a = flat[:-1].reshape(3, F, nCand)[:, :, :nL]
            sg = a[2] / n; c = a[0] / n - beta * sg * sg; rho = -c
    if kind < 2:
        best, arg, idx = 1000000, cand[0], 0
        for i in range(nL):
            if rho[i] < best:                                                 # the first minimum; a NaN never wins
                best, arg, idx = rho[i], cand[i], i
        cost = np.zeros(nCand); cost[:nL] = c
        return float(arg), idx, cost, rho, None
    best, arg, idx = 1000000, f32(0), 0; ths = np.zeros(F)
    for f in range(1, F):
        loc = 1000000
        for i in range(nL):
            if rho[f, i] <= best:                                             # the last minimum
                best, arg, idx = rho[f, i], cand[i], i
            if rho[f, i] <= loc:
                loc, ths[f] = rho[f, i], cand[i]
    cost = np.zeros((F, nCand)); cost[:, :nL] = c
    return float(arg), idx, cost, rho, ths
