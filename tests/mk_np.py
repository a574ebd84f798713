"""numpy restatements of maximum empirical kurtosis beamforming (MEKSubbandBeamformer_pr / _nrm), one (utterance, bin) problem at a time.

Two problem classes with one interface (f, df, fdf, finish, norm clipping):
  RefProblem  the reference's arithmetic in its order: complex numpy values, a Python loop over the frames, every term divided by N
              before it is added (btk/lib/mkBeamforming.py:410-484, 549-577)
  DevProblem  the device's order (csrc/k_mk.hip): y0 = wq^H X and Z = B^H X first (channels in increasing order), separate real and imaginary
              fp64 arrays so that no library complex product can fuse, 64 partial sums (partial p adds frames p, p + 64, ...), a fixed
              binary tree, one division by N after the sum
The two minimisers (conjugate_pr with its line search; steepest descent) and both driver loops are written once and run on either class."""
import math

import numpy as np

MAXIT, GRADIENT, DIFFERENCE, NO_PROGRESS, EVAL_CAP_HIT, SKIPPED = 0, 1, 2, 3, 4, 5
EVAL_CAP = 2048
P = 64
PR, NRM = 0, 1
DEFAULTS = {PR: dict(alpha=1.0e-2, beta=3.0, gamma=-1.0, MAXITNS=40, TOLERANCE=1.0e-3, STOPTOLERANCE=1.0e-2, DIFFSTOPTOLERANCE=1.0e-5, STEPSIZE=0.01),
            NRM: dict(alpha=0.1, beta=3.0, gamma=-1.0, MAXITNS=40, TOLERANCE=1.0e-3, STOPTOLERANCE=1.0e-2, DIFFSTOPTOLERANCE=1.0e-10, STEPSIZE=0.01)}


def bound_factor(T, C):
    """|ref - dev| <= 4 (T + 4 C) 2^-53 S: every addition of a sum of T terms rounds once, a term is a product of up to four values |Y| or |Z|,
    each a sum of C complex products that round a few times; S = the sum of the magnitudes of the summed terms (RefProblem.magnitudes)."""
    return 4.0 * (T + 4 * C) * 2.0 ** -53


def select_frames(sFrame, eFrame, R, nframes, Tmax):
    """accumObservations(sFrame, eFrame, R): the frame indices kept"""
    R = max(int(R), 1)
    return [s for s in range(max(sFrame, 0), min(eFrame, nframes, Tmax)) if s % R == 0]


def blocking_matrix(d):
    """_calcBlockingMatrix for NC = 1 in the order of csrc/gsc_weights.h: Gram-Schmidt on the first C-1 columns of I - conj(d) d^T / |d|^2"""
    C = len(d); bs = C - 1
    nrm = 0.0
    for i in range(C):
        nrm += d[i].real * d[i].real + d[i].imag * d[i].imag
    nrm = math.sqrt(nrm); nrm = nrm * nrm

    def mul(a, b):
        return complex(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)
    Pm = [[complex(1.0 if i == j else 0.0, 0.0) + mul(mul(complex(-1.0 / nrm, 0.0), d[i].conjugate()), d[j]) for j in range(C)] for i in range(C)]
    B = np.zeros((C, bs), np.complex128)
    for k in range(bs):
        vec = [Pm[i][k] for i in range(C)]
        for jd in range(k):
            ip = 0j
            for i in range(C):
                ip += mul(complex(B[i, jd]).conjugate(), vec[i])
            ip = complex(ip.real * -1.0, ip.imag * -1.0)
            for i in range(C):
                vec[i] += mul(ip, complex(B[i, jd]))
        nv = 0.0
        for i in range(C):
            nv += vec[i].real * vec[i].real + vec[i].imag * vec[i].imag
        nv = math.sqrt(nv)
        for i in range(C):
            B[i, k] = complex(vec[i].real * (1.0 / nv), vec[i].imag * (1.0 / nv))
    return B


def seq_norm(v):
    """|v|: the square root of the sequential sum of squares"""
    r = 0.0
    for a in v:
        r += float(a) * float(a)
    return math.sqrt(r)


def seq_dot(a, b):
    r = 0.0
    for x, y in zip(a, b):
        r += float(x) * float(y)
    return r


class _Problem:
    def __init__(self, kind, alpha, beta, gamma, prev):
        self.kind, self.alpha, self.beta, self.gamma = kind, float(alpha), float(beta), float(gamma)
        self.prev = [float(prev[0]), float(prev[1]), float(prev[2])]            # prevAvgY2, prevAvgY4, prevFrameN
        self.evals = 0; self.clipped = 0

    def f(self, x):
        self.evals += 1; return self._cost(x)

    def df(self, x):
        self.evals += 1; return self._grad(x)

    def fdf(self, x):
        self.evals += 1; return self._cost(x), self._grad(x)


class RefProblem(_Problem):
    """X [T][C] complex: the observations of one bin; wq [C], B [C][C-1]"""

    def __init__(self, kind, X, wq, B, alpha, beta, gamma=-1.0, prev=(0.0, 0.0, 0.0)):
        _Problem.__init__(self, kind, alpha, beta, gamma, prev)
        self.X = np.asarray(X, np.complex128); self.wq = np.asarray(wq, np.complex128); self.B = np.asarray(B, np.complex128)
        self.T, self.n = self.X.shape[0], self.B.shape[1]

    def normalize(self, wa):
        if self.kind != NRM:
            return wa
        nrm_wa = np.sqrt(np.inner(wa, np.conjugate(wa)).real)
        gamma = np.sqrt(np.inner(self.wq, np.conjugate(self.wq))) if self.gamma < 0 else self.gamma
        if nrm_wa > abs(gamma):
            self.clipped += 1
            wa = abs(gamma) * wa / nrm_wa
        return wa

    def entire(self, wa):
        return self.wq - np.dot(self.B, self.normalize(wa))

    @staticmethod
    def unpack(x):
        x = np.asarray(x, np.float64)
        return x[0::2] + 1j * x[1::2]

    def _cost(self, x):
        with np.errstate(all="ignore"):
            wa = self.normalize(self.unpack(x))
            N = self.prev[2] + self.T
            exY4 = (np.float64(self.prev[1]) / N) * self.prev[2]
            exY2 = (np.float64(self.prev[0]) / N) * self.prev[2]
            for t in range(self.T):
                Y = np.dot(np.conjugate(self.entire(wa)), self.X[t])
                Y2 = Y * np.conjugate(Y); Y4 = Y2 * Y2
                exY2 += Y2.real / N; exY4 += Y4.real / N
            kurt = exY4 - self.beta * exY2 * exY2
            return float(0.0 - kurt + (self.alpha * np.inner(wa, np.conjugate(wa))).real)

    def _grad(self, x):
        with np.errstate(all="ignore"):
            wa = self.normalize(self.unpack(x))
            N = self.prev[2] + self.T
            exY2 = (np.float64(self.prev[0]) / N) * self.prev[2]
            dexY2 = np.zeros(self.n, np.complex128); dexY4 = np.zeros(self.n, np.complex128)
            BH = np.transpose(np.conjugate(self.B))
            for t in range(self.T):
                Y = np.dot(np.conjugate(self.entire(wa)), self.X[t])
                BHX = -np.dot(BH, self.X[t])
                Y2 = Y * np.conjugate(Y)
                dexY4 += 2 * Y2 * BHX * np.conjugate(Y) / N
                dexY2 += BHX * np.conjugate(Y) / N
                exY2 += Y2.real / N
            d = -(dexY4 - 2 * self.beta * exY2 * dexY2) + self.alpha * wa
            g = np.zeros(2 * self.n); g[0::2] = d.real; g[1::2] = d.imag
            return g

    def finish(self, x):
        """_nrm after the loop (:646-654): normalise, storeStatistics with prevFrameN advanced first"""
        wa = self.normalize(self.unpack(x))
        self.prev[2] += self.T
        for t in range(self.T):
            Y = np.dot(np.conjugate(self.entire(wa)), self.X[t])
            Y2 = Y * np.conjugate(Y); Y4 = Y2 * Y2
            self.prev[0] += Y2.real / self.prev[2]; self.prev[1] += Y4.real / self.prev[2]
        out = np.zeros(2 * self.n); out[0::2] = wa.real; out[1::2] = wa.imag
        return out

    def magnitudes(self, x):
        """S of the error bound: what the cost and each gradient entry become when every summed term is replaced by its magnitude
        (products of magnitudes all the way down to |w_c| |x_c|) -> (S_cost, S_grad [n])"""
        wa = self.normalize(self.unpack(x)); self.clipped = 0
        N = self.prev[2] + self.T
        wom = np.abs(self.wq) + np.abs(self.B) @ np.abs(wa)
        Ym = np.abs(self.X) @ wom                                                # [T]
        Zm = np.abs(self.X) @ np.abs(self.B)                                     # [T][n]
        e2 = self.prev[0] * self.prev[2] / N + (Ym ** 2).sum() / N
        e4 = self.prev[1] * self.prev[2] / N + (Ym ** 4).sum() / N
        Sc = e4 + self.beta * e2 * e2 + self.alpha * (np.abs(wa) ** 2).sum()
        Sg = 2.0 * ((Ym ** 3)[:, None] * Zm).sum(0) / N + 2.0 * self.beta * e2 * (Ym[:, None] * Zm).sum(0) / N + self.alpha * np.abs(wa)
        return float(Sc), Sg


def _partials(term):
    """term [T] or [T][k] -> the 64 partial sums: partial p adds frames p, p + 64, ... in increasing order"""
    acc = np.zeros((P,) + term.shape[1:])
    for k in range(0, term.shape[0], P):
        seg = term[k:k + P]
        acc[:seg.shape[0]] = acc[:seg.shape[0]] + seg
    return acc


def _tree(a):
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def dev_prepare(X, wq, B):
    """X [T][C] complex64 -> (y0r, y0i [T], Zr, Zi [T][C-1]) in fp64, channels in increasing order"""
    X = np.asarray(X); xr = X.real.astype(np.float64); xi = X.imag.astype(np.float64)
    T, C = X.shape; n = C - 1
    wr, wi = np.asarray(wq).real, np.asarray(wq).imag; br, bi = np.asarray(B).real, np.asarray(B).imag
    y0r = np.zeros(T); y0i = np.zeros(T); Zr = np.zeros((T, n)); Zi = np.zeros((T, n))
    for c in range(C):
        y0r = y0r + (wr[c] * xr[:, c] + wi[c] * xi[:, c]); y0i = y0i + (wr[c] * xi[:, c] - wi[c] * xr[:, c])
        Zr = Zr + (br[c][None, :] * xr[:, c][:, None] + bi[c][None, :] * xi[:, c][:, None])
        Zi = Zi + (br[c][None, :] * xi[:, c][:, None] - bi[c][None, :] * xr[:, c][:, None])
    return y0r, y0i, Zr, Zi


def dev_gamma(wq, gamma):
    if gamma >= 0:
        return float(gamma)
    q = 0.0
    for w in wq:
        q += w.real * w.real + w.imag * w.imag
    return math.sqrt(q)


class DevProblem(_Problem):
    def __init__(self, kind, X, wq, B, alpha, beta, gamma=-1.0, prev=(0.0, 0.0, 0.0)):
        _Problem.__init__(self, kind, alpha, beta, gamma, prev)
        self.y0r, self.y0i, self.Zr, self.Zi = dev_prepare(X, wq, B)
        self.T, self.n = self.Zr.shape
        self.ag = abs(dev_gamma(np.asarray(wq, np.complex128), gamma))
        self.S2 = self.S4 = 0.0

    def _clip(self, x):
        x = np.asarray(x, np.float64)
        s = 0.0
        for k in range(self.n):
            s += x[2 * k] * x[2 * k] + x[2 * k + 1] * x[2 * k + 1]
        if self.kind == NRM:
            nr = math.sqrt(s)
            if nr > self.ag:
                self.clipped += 1
                return (self.ag * x) / nr
        return x.copy()

    def _eval(self, x, want_g):
        n, T = self.n, self.T
        if T == 0:
            return float("nan"), np.full(2 * n, np.nan)
        w = self._clip(x); wr = w[0::2]; wi = w[1::2]
        s2 = 0.0
        for k in range(n):
            s2 += w[2 * k] * w[2 * k] + w[2 * k + 1] * w[2 * k + 1]
        rterm = self.alpha * s2
        pY2, pY4, pN = self.prev; N = pN + float(T)
        sr = np.zeros(T); si = np.zeros(T)
        for j in range(n):
            sr = sr + (wr[j] * self.Zr[:, j] + wi[j] * self.Zi[:, j]); si = si + (wr[j] * self.Zi[:, j] - wi[j] * self.Zr[:, j])
        Yr = self.y0r - sr; Yi = self.y0i - si; y2 = Yr * Yr + Yi * Yi
        S2 = float(_tree(_partials(y2))); S4 = float(_tree(_partials(y2 * y2)))
        self.S2, self.S4 = S2, S4
        exY2 = (pY2 / N) * pN + S2 / N; exY4 = (pY4 / N) * pN + S4 / N
        kurt = exY4 - (self.beta * exY2) * exY2
        f = (0.0 - kurt) + rterm
        g = None
        if want_g:
            qr = self.Zr * Yr[:, None] + self.Zi * Yi[:, None]; qi = self.Zi * Yr[:, None] - self.Zr * Yi[:, None]
            A2r = _tree(_partials(qr)); A2i = _tree(_partials(qi)); A4r = _tree(_partials(y2[:, None] * qr)); A4i = _tree(_partials(y2[:, None] * qi))
            d4r = (-2.0 * A4r) / N; d4i = (-2.0 * A4i) / N; d2r = (-A2r) / N; d2i = (-A2i) / N
            cc = (2.0 * self.beta) * exY2
            g = np.zeros(2 * n)
            g[0::2] = (-(d4r - cc * d2r)) + self.alpha * wr; g[1::2] = (-(d4i - cc * d2i)) + self.alpha * wi
        return f, g

    def _cost(self, x):
        return self._eval(x, False)[0]

    def _grad(self, x):
        return self._eval(x, True)[1]

    def fdf(self, x):
        self.evals += 1; return self._eval(x, True)

    def finish(self, x):
        w = self._clip(x)
        self._eval(w, False)
        N = self.prev[2] + float(self.T)
        self.prev = [self.prev[0] + self.S2 / N, self.prev[1] + self.S4 / N, N]
        return w


def _step(x, p, a):
    dx = a * p
    return x + dx


def minimize(prob, x0, kind=None, MAXITNS=40, TOLERANCE=1.0e-3, STOPTOLERANCE=1.0e-2, DIFFSTOPTOLERANCE=None, STEPSIZE=0.01, store=True, **_unused):
    """the driver loops of estimateActiveWeights (:486-534 for _pr, :579-658 for _nrm) over the minimiser of that kind.
    -> dict(x, iters, evals, failed, reason, f, branches); branches: the names of the branches this run took"""
    kind = prob.kind if kind is None else kind
    if DIFFSTOPTOLERANCE is None:
        DIFFSTOPTOLERANCE = DEFAULTS[kind]["DIFFSTOPTOLERANCE"]
    x = np.array(x0, np.float64); n2 = len(x)
    br = set(); prob.evals = 0; prob.clipped = 0
    res = dict(x=x.copy(), iters=0, evals=0, failed=0, reason=SKIPPED, f=float("nan"), branches=br)
    if prob.T == 0:
        return res
    with np.errstate(all="ignore"):
        f, g = prob.fdf(x)
    if not math.isfinite(f):
        res.update(evals=prob.evals, f=f)
        return res
    iters = failed = 0; reason = MAXIT; preMi = 10000.0
    if kind == PR:
        p = g.copy(); g0 = g.copy(); pnorm = g0norm = seq_norm(g); step = STEPSIZE; cg = 0
        for itera in range(MAXITNS):
            it_evals = prob.evals
            if pnorm == 0.0 or g0norm == 0.0:
                reason = NO_PROGRESS; break
            fa, stepa, stepc = f, 0.0, step
            pg = seq_dot(p, g)
            lam = (1.0 if pg >= 0.0 else -1.0) / pnorm
            x1 = _step(x, p, -stepc * lam); fc = prob.f(x1)
            ic, ifc, capped = stepc, fc, False
            while True:                                           # intermediate_point
                u = abs(pg * lam * ic)
                with np.errstate(all="ignore"):
                    stepb = float(np.float64(0.5 * ic * u) / np.float64((ifc - fa) + u))
                if prob.evals - it_evals >= EVAL_CAP:
                    capped = True; break
                x1 = _step(x, p, -stepb * lam); fb = prob.f(x1)
                if fb >= fa and stepb > 0.0:
                    ifc, ic = fb, stepb; failed += 1; br.add("intermediate_retry"); continue
                break
            if capped:
                reason = EVAL_CAP_HIT; break
            g = prob.df(x1)
            if stepb == 0.0:
                reason = NO_PROGRESS; break
            uS, vS, wS, fu, fv, fw = stepb, stepa, stepc, fb, fa, fc
            old2, old1 = abs(wS - vS), abs(vS - uS)
            x2 = x1.copy(); fnew, stepnew, g1norm = fb, stepb, seq_norm(g)
            for _li in range(10):                                 # minimize
                dw, dv, du = wS - uS, vS - uS, 0.0
                e1 = ((fv - fu) * dw * dw + (fu - fw) * dv * dv)
                e2 = 2.0 * ((fv - fu) * dw + (fu - fw) * dv)
                if e2 != 0.0:
                    du = e1 / e2
                if du > 0.0 and du < (stepc - stepb) and abs(du) < 0.5 * old2:
                    stepm = uS + du
                elif du < 0.0 and du > (stepa - stepb) and abs(du) < 0.5 * old2:
                    stepm = uS + du
                elif (stepc - stepb) > (stepb - stepa):
                    stepm = 0.38 * (stepc - stepb) + stepb
                else:
                    stepm = stepb - 0.38 * (stepb - stepa)
                x1 = _step(x, p, -stepm * lam); fm = prob.f(x1)
                if fm > fb:
                    if fm < fv:
                        wS, vS, fw, fv = vS, stepm, fv, fm
                    elif fm < fw:
                        wS, fw = stepm, fm
                    if stepm < stepb:
                        stepa, fa = stepm, fm
                    else:
                        stepc, fc = stepm, fm
                elif fm <= fb:
                    old2 = old1; old1 = abs(uS - stepm)
                    wS, vS, uS, fw, fv, fu = vS, uS, stepm, fv, fu, fm
                    x2 = x1.copy(); g = prob.df(x1)
                    pg = seq_dot(p, g); gnorm1 = seq_norm(g)
                    fnew, stepnew, g1norm = fm, stepm, gnorm1
                    with np.errstate(all="ignore"):
                        ok = abs(np.float64(pg * lam) / np.float64(gnorm1)) < TOLERANCE
                    if ok:
                        break
                    if stepm < stepb:
                        stepc, fc, stepb, fb = stepb, fb, stepm, fm
                    else:
                        stepa, fa, stepb, fb = stepb, fb, stepm, fm
                else:
                    break
            f, step, x = fnew, stepnew, x2
            cg = (cg + 1) % n2
            if cg == 0:
                p = g.copy(); pnorm = g1norm; br.add("restart")
            else:
                g0 = g0 + (-1.0) * g
                with np.errstate(all="ignore"):
                    beta = float(np.float64(seq_dot(g0, g)) / np.float64(g0norm * g0norm))
                q = (-beta) * p; p = q + g; pnorm = seq_norm(p)
            g0norm = g1norm; g0 = g.copy()
            iters += 1
            if seq_norm(g) < STOPTOLERANCE:
                reason = GRADIENT; break
            if abs(preMi - f) < DIFFSTOPTOLERANCE:
                reason = DIFFERENCE; break
            preMi = f
    else:
        step = STEPSIZE
        for itera in range(MAXITNS):
            it_evals = prob.evals
            f0, fail, stop = f, False, None
            gnorm = seq_norm(g)
            if gnorm == 0.0:
                reason = NO_PROGRESS; break
            while True:
                x1 = _step(x, g, (-step) / gnorm)
                if np.array_equal(x1, x):
                    stop = NO_PROGRESS; break
                if prob.evals - it_evals >= EVAL_CAP:
                    stop = EVAL_CAP_HIT; break
                f1, g1 = prob.fdf(x1)
                if f1 > f0:
                    fail = True; failed += 1; step *= TOLERANCE; br.add("failed_trial"); continue
                break
            if stop is not None:
                reason = stop; break
            step *= TOLERANCE if fail else 2.0
            x, g, f = x1, g1, f1
            iters += 1
            if seq_norm(g) < STOPTOLERANCE and itera > 2:
                reason = GRADIENT; break
            if abs(preMi - f) < DIFFSTOPTOLERANCE and itera > 2:
                reason = DIFFERENCE; break
            preMi = f
    evals = prob.evals
    if prob.clipped:
        br.add("clip")
    if kind == NRM and store:
        x = prob.finish(x)
    res.update(x=np.array(x, np.float64), iters=iters, evals=evals, failed=failed, reason=reason, f=float(f))
    return res
