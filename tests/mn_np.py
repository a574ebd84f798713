"""numpy restatements of maximum negentropy beamforming under a generalised Gaussian (GG) model (MNSubbandBeamformerGGDc_pr / _nrm) and of the GG
model's training (MLE4CGGaussianD), written from the formulas of include/dsr.h section 2a'.

  det_log, det_exp, det_pow, det_psi   csrc/det_math.h operation for operation (frexp / ldexp are exact, so they stand for the exponent-field moves)
  RefProblem   the reference's arithmetic in its order: complex numpy values, np.power / np.log, a Python loop over the frames
  DevProblem   the device's order (csrc/mn_kernels.hip) on mk_np.dev_prepare, _partials and _tree
Both plug into mk_np.minimize(kind=PR): the two reference classes run conjugate_pr and differ in the default beta only.
  ggd_acc_ref, ggd_acc_dev, ggd_update, ggd_constants   the training statistics in the reference's and in the device's order, the update, fixConst"""
import math

import numpy as np

from tests import mk_np

U53 = 2.0 ** -53
LN2_HI = float.fromhex("0x1.62e42fefp-1")                # the leading 33 bits of ln 2
LN2_LO = float.fromhex("0x1.473de6af278edp-34")
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
SQRT_HALF = 0.70710678118654757
LOG_PI = 1.1447298858494002
DEFAULTS = dict(alpha=1.0e-2, beta=0.5, gamma=-1.0, MAXITNS=40, TOLERANCE=1.0e-3, STOPTOLERANCE=1.0e-2, DIFFSTOPTOLERANCE=1.0e-5, STEPSIZE=0.2)


def det_log(x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        m, e = np.frexp(x)                                # x = 2^e m, m in [1/2, 1); exact, subnormals included
        low = m < SQRT_HALF
        m = np.where(low, m * 2.0, m); e = np.where(low, e - 1, e)
        s = (m - 1.0) / (m + 1.0); z = s * s
        p = np.full(x.shape, 1.0 / 23.0)
        for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            p = 1.0 / d + z * p
        s2 = 2.0 * s; r = s2 + s2 * (z * p); de = e.astype(np.float64)
        out = (de * LN2_HI + r) + de * LN2_LO
        out = np.where(x == 0.0, -np.inf, out)
        out = np.where(np.isposinf(x), np.inf, out)
        out = np.where((x < 0.0) | np.isnan(x), np.nan, out)
    return out if out.ndim else float(out)


_INV_FACT = [1.0 / float(math.factorial(j)) for j in range(15)]


def det_exp(x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        xc = np.where((x >= -708.0) & (x <= 709.0), x, 0.0)
        k = np.floor(xc * INV_LN2 + 0.5)
        r = (xc - k * LN2_HI) - k * LN2_LO
        p = np.full(x.shape, _INV_FACT[14])
        for j in range(13, 1, -1):
            p = _INV_FACT[j] + r * p
        y = 1.0 + (r + (r * r) * p)
        out = np.ldexp(y, k.astype(np.int64))
        out = np.where(x < -708.0, 0.0, out)
        out = np.where(x > 709.0, np.inf, out)
        out = np.where(np.isnan(x), np.nan, out)
    return out if out.ndim else float(out)


def det_pow(x, f):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        out = np.where(x > 0.0, det_exp(f * det_log(np.where(x > 0.0, x, 1.0))), np.where(x == 0.0, 0.0, np.nan))
    return out if out.ndim else float(out)


def det_psi(x):
    """digamma of one positive value"""
    x = float(x); r = 0.0
    while x < 6.0:
        r -= 1.0 / x; x += 1.0
    v = 1.0 / x; w = v * v
    t = 854513.0 / 3036.0
    for c in (174611.0 / 6600.0, 43867.0 / 14364.0, 3617.0 / 8160.0, 1.0 / 12.0, 691.0 / 32760.0, 1.0 / 132.0, 1.0 / 240.0, 1.0 / 252.0, 1.0 / 120.0, 1.0 / 12.0):
        t = c - w * t
    return r + ((det_log(x) - 0.5 * v) - w * t)


def eps_pow(f, x):
    """the relative error bound of det_pow(x, f) that tests/test_mn_np_cpu.py asserts"""
    with np.errstate(all="ignore"):
        return 4.0 * (np.abs(f * np.log(x)) + 2.0) * U53


def ggd_constants(p):
    """fixConst for one shape parameter in the order of csrc/ggd.h -> dict(Bc, lNF, NgConst, LlConst, logBc)"""
    lg1 = math.lgamma(1.0 / p); lg2 = math.lgamma(2.0 / p); lB = lg1 - lg2
    Bc = det_exp(lB); lNF = (LOG_PI + lg1) + lB
    return dict(Bc=Bc, lNF=lNF, NgConst=(lNF - det_log(p)) + 1.0 / p, LlConst=det_log(p) - lNF, logBc=det_log(Bc))


class _MnProblem(mk_np._Problem):
    def __init__(self, alpha, beta, shape, Bc, NgConst):
        mk_np._Problem.__init__(self, mk_np.PR, alpha, beta, -1.0, (0.0, 0.0, 0.0))
        self.shape, self.Bc, self.NgConst = float(shape), float(Bc), float(NgConst)


class RefProblem(_MnProblem):
    """X [T][C] complex: the observations of one bin; wq [C], B [C][C-1]; Bc, NgConst: the model's constants of this bin"""

    def __init__(self, X, wq, B, alpha, beta, shape, Bc, NgConst):
        _MnProblem.__init__(self, alpha, beta, shape, Bc, NgConst)
        self.X = np.asarray(X, np.complex128); self.wq = np.asarray(wq, np.complex128); self.B = np.asarray(B, np.complex128)
        self.T, self.n = self.X.shape[0], self.B.shape[1]

    unpack = staticmethod(mk_np.RefProblem.unpack)

    def _outputs(self, wa):
        """calcCovarOutputs_f -> (Y [T], SigmaY, SigmaYf)"""
        wo = self.wq - np.dot(self.B, wa); f = self.shape
        Y = np.zeros(self.T, np.complex128); SigmaY = 0j; SigmaYf = 0.0
        for t in range(self.T):
            Y[t] = np.inner(np.conjugate(wo), self.X[t])
            s = Y[t] * np.conjugate(Y[t])
            SigmaY += s; SigmaYf += np.power(s.real, f)
        return Y, SigmaY / self.T, SigmaYf / self.T

    def _cost(self, x):
        with np.errstate(all="ignore"):
            wa = self.unpack(x); f = self.shape
            _, SigmaY, SigmaYf = self._outputs(wa)
            scaling = np.power(f * SigmaYf, 1 / f) / self.Bc
            JY = (np.log(SigmaY) + (1 + np.log(np.pi))) - self.beta * (self.NgConst + np.log(scaling))
            return float((-JY + (self.alpha * np.inner(wa, np.conjugate(wa))).real).real)

    def _grad(self, x):
        with np.errstate(all="ignore"):
            wa = self.unpack(x); f = self.shape
            Y, SigmaY, SigmaYf = self._outputs(wa)
            BH = np.conjugate(self.B).transpose()
            dJ = np.zeros(self.n, np.complex128); cnt = 0
            for t in range(self.T):
                absY = abs(Y[t])
                q = np.dot(BH, self.X[t]) * np.conjugate(Y[t])
                if absY > 0.0:
                    val = np.power(absY, 2 * f - 2) / SigmaYf
                    dJ += (-(1 / SigmaY) + self.beta * val) * q
                    cnt += 1
            d = -(dJ / cnt) + self.alpha * wa
            g = np.zeros(2 * self.n); g[0::2] = d.real; g[1::2] = d.imag
            return g

    def bound(self, x, C):
        """-> (bound of |ref - dev| for the cost, for each gradient entry [n]).  u = 2^-53, b = mk_np.bound_factor(T, C) (a sum of T terms, each
        from sums of C complex products).  Magnitude sums: Ym_t = sum_c |wo_c| |x_tc| >= |Y_t|, Zm_tj = sum_c |B_cj| |x_tc|.
          Y_t is off by at most bC Ym_t, bC = bound_factor(0, C); so y2_t = |Y_t|^2 is off by the relative r_t = 2 rho + rho^2, rho = bC Ym_t / |Y_t|.
          sigma2: relative rs = b sum Ym^2 / sum y2.   log sigma2: rs + 5 u |log sigma2| (det_log 4 u, the library's log 1 u).
          p_t = y2_t^f: relative d_t = EPS_POW(f, y2_t) + f r_t, so Sf is off by the relative rf = sum p_t d_t / sum p_t + b,
          and log(f Sf) / f by rf / f + 6 u |log(f Sf)| / f.
          cost: rs + 5 u |log sigma2| + beta (rf / f + 6 u |log(f Sf)| / f + 2 u (|NgConst| + |log Bc|)) + b alpha |wa|^2 + 4 u |cost|.
          gradient entry j = G1_j - G2_j + alpha wa_j with G1_j = sum' q_tj / (sigma2 T'), G2_j = beta sum' y2_t^(f-1) q_tj / (Sf T'):
          |q_tj| <= Ym_t Zm_tj with relative error 2 b; y2^(f-1) is off by the relative e_t = EPS_POW(f, y2_t) + (|f - 1| + f + 1) r_t + 4 u, so
          bound_j = (b + rs) sum' Ym Zm_j / (sigma2 T') + beta sum' y2^(f-1) Ym Zm_j (2 b + rf + e_t) / (Sf T') + b alpha |wa_j|."""
        with np.errstate(all="ignore"):
            wa = self.unpack(x); f = self.shape; u = U53; T = self.T
            b = mk_np.bound_factor(T, C); bC = mk_np.bound_factor(0, C)
            Y, SigmaY, Sf = self._outputs(wa); sig2 = SigmaY.real
            y2 = np.abs(Y) ** 2; pos = y2 > 0.0
            Ym = np.abs(self.X) @ (np.abs(self.wq) + np.abs(self.B) @ np.abs(wa)); Zm = np.abs(self.X) @ np.abs(self.B)
            rho = np.where(pos, bC * Ym / np.where(pos, np.abs(Y), 1.0), 0.0); r = 2 * rho + rho * rho
            rs = b * (Ym ** 2).sum() / y2.sum()
            p = np.where(pos, np.power(y2, f), 0.0)
            ep = np.where(pos, eps_pow(f, np.where(pos, y2, 1.0)), 0.0)
            rf = (p * (ep + f * r)).sum() / p.sum() + b
            cost = self._cost(x)
            lB = abs(math.log(self.Bc))
            bc = (rs + 5 * u * abs(np.log(sig2)) + self.beta * (rf / f + 6 * u * abs(np.log(f * Sf)) / f + 2 * u * (abs(self.NgConst) + lB))
                  + b * self.alpha * (np.abs(wa) ** 2).sum() + 4 * u * abs(cost))
            Tp = max(int(pos.sum()), 1)
            e = ep + (abs(f - 1) + f + 1) * r + 4 * u
            pm1 = np.where(pos, p / np.where(pos, y2, 1.0), 0.0)
            g1 = (b + rs) * ((Ym * pos)[:, None] * Zm).sum(0) / (sig2 * Tp)
            g2 = self.beta * ((pm1 * Ym * (2 * b + rf + e))[:, None] * Zm).sum(0) / (Sf * Tp)
            return float(bc), g1 + g2 + b * self.alpha * np.abs(wa)


class DevProblem(_MnProblem):
    def __init__(self, X, wq, B, alpha, beta, shape, Bc, NgConst, logBc):
        _MnProblem.__init__(self, alpha, beta, shape, Bc, NgConst)
        self.logBc = float(logBc)
        self.y0r, self.y0i, self.Zr, self.Zi = mk_np.dev_prepare(X, wq, B)
        self.T, self.n = self.Zr.shape

    def _eval(self, x, want_g):
        n, T = self.n, self.T
        if T == 0:
            return float("nan"), np.full(2 * n, np.nan)
        with np.errstate(all="ignore"):
            w = np.asarray(x, np.float64); wr = w[0::2]; wi = w[1::2]; f = self.shape
            s2 = 0.0
            for k in range(n):
                s2 += w[2 * k] * w[2 * k] + w[2 * k + 1] * w[2 * k + 1]
            rterm = self.alpha * s2
            sr = np.zeros(T); si = np.zeros(T)
            for j in range(n):
                sr = sr + (wr[j] * self.Zr[:, j] + wi[j] * self.Zi[:, j]); si = si + (wr[j] * self.Zi[:, j] - wi[j] * self.Zr[:, j])
            Yr = self.y0r - sr; Yi = self.y0i - si; y2 = Yr * Yr + Yi * Yi
            pt = det_pow(y2, f); pos = y2 > 0.0
            S2 = float(mk_np._tree(mk_np._partials(y2))); Sp = float(mk_np._tree(mk_np._partials(pt))); Tp = float(pos.sum())
            if not S2 > 0.0:
                return float("nan"), np.full(2 * n, np.nan)
            Tn = float(T); sig2 = S2 / Tn; Sf = Sp / Tn
            hg = det_log(sig2) + (1.0 + LOG_PI)
            hgg = (self.NgConst + det_log(f * Sf) / f) - self.logBc
            cost = (0.0 - (hg - self.beta * hgg)) + rterm
            g = None
            if want_g:
                ratio = np.where(pos, pt / np.where(pos, y2, 1.0), 0.0)
                qr = self.Zr * Yr[:, None] + self.Zi * Yi[:, None]; qi = self.Zi * Yr[:, None] - self.Zr * Yi[:, None]
                m = pos[:, None]
                A1r = mk_np._tree(mk_np._partials(np.where(m, qr, 0.0))); A1i = mk_np._tree(mk_np._partials(np.where(m, qi, 0.0)))
                Apr = mk_np._tree(mk_np._partials(np.where(m, ratio[:, None] * qr, 0.0))); Api = mk_np._tree(mk_np._partials(np.where(m, ratio[:, None] * qi, 0.0)))
                dJr = ((-A1r) / sig2 + (self.beta * Apr) / Sf) / Tp; dJi = ((-A1i) / sig2 + (self.beta * Api) / Sf) / Tp
                g = np.zeros(2 * n)
                g[0::2] = (-dJr) + self.alpha * wr; g[1::2] = (-dJi) + self.alpha * wi
        return float(cost), g

    def _cost(self, x):
        return self._eval(x, False)[0]

    def _grad(self, x):
        return self._eval(x, True)[1]

    def fdf(self, x):
        self.evals += 1; return self._eval(x, True)


def minimize(prob, x0, **over):
    kw = dict(DEFAULTS); kw.update(over)
    return mk_np.minimize(prob, x0, kind=mk_np.PR, **{k: kw[k] for k in ("MAXITNS", "TOLERANCE", "STOPTOLERANCE", "DIFFSTOPTOLERANCE", "STEPSIZE")})


# ---- GG model training
ACC_TINY2 = 1.0e-22                                       # (10e-12)^2: acc1P takes a sample only where |X| > 10e-12


def ggd_acc_ref(X, nframes, p, sa):
    """MLE4CGGaussianD.acc sample by sample in the reference's arithmetic.  X [U][T][F] complex -> acc [5][F]"""
    U, T, F = X.shape; acc = np.zeros((5, F))
    with np.errstate(all="ignore"):
        for f in range(F):
            c = ggd_constants(p[f]); B = c["Bc"]; Ll = c["LlConst"]
            for uu in range(U):
                for t in range(min(int(nframes[uu]), T)):
                    val = abs(complex(X[uu, t, f])); X2 = val * val
                    acc[0, f] += np.power(X2, p[f])
                    argE = X2 / (B * sa[f]); tmp = np.power(argE, p[f])
                    if val > 10e-12:
                        acc[1, f] += tmp * np.log(argE)
                    acc[2, f] += tmp
                    acc[3, f] += 1
                    acc[4, f] += Ll - np.log(sa[f]) - tmp
    return acc


def ggd_acc_dev(X, nframes, p, sa, acc_in=None, constants=ggd_constants):
    """the device's order: v2 from the fp32 parts in fp64, det functions, per (utterance, bin) 64 partial sums and a tree, then acc_in and the
    utterances in increasing order.  constants(p) -> dict(Bc, LlConst, ...): the library's lgamma is the C library's, math.lgamma is Python's
    own, so a bit-for-bit comparison hands in the library's constants (dsr_ggd_constants)."""
    X = np.asarray(X, np.complex64); U, T, F = X.shape
    p = np.asarray(p, np.float64); sa = np.asarray(sa, np.float64)
    cs = [constants(float(v)) for v in p]
    Bc = np.array([c["Bc"] for c in cs]); Ll = np.array([c["LlConst"] for c in cs])
    la0 = det_log(Bc * sa); ll0 = Ll - det_log(sa)
    acc = np.zeros((5, F)) if acc_in is None else np.array(acc_in, np.float64)
    with np.errstate(all="ignore"):
        for uu in range(U):
            nf = max(min(int(nframes[uu]), T), 0)
            re = X[uu, :nf].real.astype(np.float64); im = X[uu, :nf].imag.astype(np.float64); v2 = re * re + im * im
            pos = v2 > 0.0; v2s = np.where(pos, v2, 1.0)
            l = det_log(v2s); la = l - la0[None, :]
            t1S = np.where(pos, det_exp(p[None, :] * l), 0.0)
            tmp = np.where(pos, det_exp(p[None, :] * la), 0.0)
            t1P = np.where(v2 > ACC_TINY2, tmp * la, 0.0)
            tL = ll0[None, :] - tmp
            for row, term in ((0, t1S), (1, t1P), (2, tmp), (4, tL)):
                acc[row] = acc[row] + mk_np._tree(mk_np._partials(term))
            acc[3] = acc[3] + float(nf)
    return acc


def ggd_update(acc, p, sa, nItr=0, alpha=0.05, thresh=0.00001, floorV=10e-8, floorP=0.07, sigmaOnly=False, constants=ggd_constants):
    """MLE4CGGaussianD.update in the order of csrc/ggd.cpp -> (newSa [F], newP [F], converged [F])"""
    F = len(p); ns = np.array(sa, np.float64); npp = np.array(p, np.float64); cv = np.zeros(F, bool)
    for f in range(F):
        a1S, a1P, a2P, nS, pf = float(acc[0][f]), float(acc[1][f]), float(acc[2][f]), float(acc[3][f]), float(p[f])
        if not nS > 0.0:
            continue
        B = constants(pf)["Bc"]
        val = det_pow((pf * a1S) / nS, 1.0 / pf)
        sigma = (1.0 / B) * val
        newp = pf
        if not sigmaOnly:
            dg1 = det_psi(1.0 / pf); dg2 = det_psi(2.0 / pf)
            dLp1 = (nS / (pf * pf)) * ((pf + 2.0 * dg1) - 2.0 * dg2)
            dLp2 = a1P + (a2P * (dg1 - 2.0 * dg2)) / pf
            dLp = dLp1 - dLp2
            newp = pf + dLp * (alpha / float(1 + nItr))
            cv[f] = abs(newp - pf) < thresh
        ns[f] = floorV if sigma < floorV else sigma
        if not sigmaOnly:
            npp[f] = floorP if newp < floorP else newp
    return ns, npp, cv


def acc_bound(X, nframes, p, sa):
    """|ggd_acc_ref - device| <= bound [5][F].  Every term is a det_pow-like value tmp = exp(p la) (relative error EPS_POW(p, argE) + 8 u: v2 from
    fp32 parts in fp64 rounds three times, the division or subtraction of logs once more) times, for acc1P, la (absolute error 6 u (|l| + |log(Bc sa)|));
    both orders add the N samples and U utterance sums with at most N + U roundings of a running sum each: 2 (N + U) u times the sum of the
    terms' magnitudes.  nSample is exact."""
    X = np.asarray(X, np.complex64); U, T, F = X.shape; u = U53; out = np.zeros((5, F))
    with np.errstate(all="ignore"):
        for f in range(F):
            c = ggd_constants(p[f]); N = 0; mags = np.zeros(5)
            for uu in range(U):
                nf = max(min(int(nframes[uu]), T), 0); N += nf
                x = X[uu, :nf, f].astype(np.complex128); v2 = np.abs(x) ** 2; pos = v2 > 0
                v2s = np.where(pos, v2, 1.0)
                l = np.log(v2s); l0 = math.log(c["Bc"] * sa[f]); la = l - l0
                t1 = np.where(pos, np.power(v2s, p[f]), 0.0); tmp = np.where(pos, np.exp(p[f] * la), 0.0)
                e1 = eps_pow(p[f], v2s) + 8 * u; e2 = 4.0 * (np.abs(p[f] * la) + 2.0) * u + 8 * u + p[f] * 6 * u * (np.abs(l) + abs(l0))
                dla = 6 * u * (np.abs(l) + abs(l0))
                out[0, f] += (t1 * e1).sum(); out[1, f] += (tmp * (np.abs(la) * e2 + dla)).sum(); out[2, f] += (tmp * e2).sum()
                out[4, f] += (tmp * e2).sum() + nf * 6 * u * (abs(c["LlConst"]) + abs(math.log(sa[f])))
                for row, mag in ((0, t1), (1, tmp * np.abs(la)), (2, tmp), (4, tmp + abs(c["LlConst"]) + abs(math.log(sa[f])))):
                    mags[row] += np.sum(mag)
            out[:, f] += 2 * (N + U) * u * mags
    return out
