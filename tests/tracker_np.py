"""Numpy restatement of the spherical-array speaker trackers (btk/beamformer/tracker.{h,cc}): BaseDecomposition / ModalDecomposition /
SpatialDecomposition (:90-870), BaseSphericalArrayTracker and its two subclasses (:881-1436) and PlaneWaveSimulator (:1444-1488), written from
the reference line by line.  `dtype` runs every operation in float64 or np.longdouble; `reverse` sums every dot product from the last term
to the first (the second opinion where long double is no wider than double).  Every printf / cout of the reference is dropped.  Ties of |B| in
the subband sort (std::sort leaves them unspecified) go to the lower bin.  Each next() appends to `log` the selected bins in order, the local
iterations used, the clamp flag, the sorted |B| and the convergence ratios."""
import math

import numpy as np

from tests import sph_np as S

SSPEED = 343740.0
CHAN = 32
EPSILON = 0.01
TOLERANCE = 1.0e-4
M_PI = math.pi


def types(dtype):
    rt = np.dtype(dtype).type
    return rt, (np.clongdouble if rt is np.longdouble else np.complex128)


def cx(re, im, ct):
    z = np.zeros((), ct)
    z.real = re
    z.imag = im
    return z[()]


def seq(x, reverse=False):
    """the sum of x as a C loop accumulates it, from the first term (or from the last)"""
    x = np.asarray(x)
    return np.cumsum(x[::-1] if reverse else x)[-1]


def gmul(a, b, ct):
    return cx(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real, ct)


def gdiv(a, b, ct):
    s = 1.0 / np.hypot(b.real, b.imag)
    sbr, sbi = s * b.real, s * b.imag
    return cx((a.real * sbr + a.imag * sbi) * s, (a.imag * sbr - a.real * sbi) * s, ct)


def eigenmike(rt=np.float64):
    """_setEigenMikeGeometry (:195-297): degrees * M_PI / 180.0"""
    return (np.array([rt(t) * rt(M_PI) / rt(180.0) for t in S.EM_THETA], rt), np.array([rt(p) * rt(M_PI) / rt(180.0) for p in S.EM_PHI], rt))


def sph_plm(l, m, x, rt):
    """gsl_sf_legendre_sphPlm, the recurrence of tests/sph_np.py in rt"""
    pmm = rt(1.0) / np.sqrt(rt(4.0) * rt(M_PI))
    u = np.sqrt((rt(1.0) - x) * (rt(1.0) + x))
    for i in range(1, m + 1):
        pmm = pmm * (-u * np.sqrt(rt(2.0 * i + 1.0) / rt(2.0 * i)))
    if l == m:
        return pmm
    p1 = x * np.sqrt(rt(2.0 * m + 3.0)) * pmm
    if l == m + 1:
        return p1
    p0 = pmm
    for n in range(m + 2, l + 1):
        a = np.sqrt(rt(4.0 * n * n - 1.0) / rt(n * n - m * m))
        b = np.sqrt(rt((n - 1.0) ** 2 - m * m) / rt(4.0 * (n - 1.0) ** 2 - 1.0))
        p0, p1 = p1, a * (x * p1 - b * p0)
    return p1


def legendre_plm(l, m, x, rt):
    """gsl_sf_legendre_Plm(l, m, x), m >= 0: the unnormalised P_l^m with the Condon-Shortley phase, upward in l from P_m^m"""
    pmm = rt(1.0)
    if m > 0:
        root = np.sqrt(rt(1.0) - x) * np.sqrt(rt(1.0) + x)
        fact = rt(1.0)
        for _ in range(m):
            pmm = pmm * (-fact * root)
            fact = fact + rt(2.0)
    if l == m:
        return pmm
    pmmp1 = x * rt(2 * m + 1) * pmm
    if l == m + 1:
        return pmmp1
    p = rt(0.0)
    for ell in range(m + 2, l + 1):
        p = (x * rt(2 * ell - 1) * pmmp1 - rt(ell + m - 1) * pmm) / rt(ell - m)
        pmm, pmmp1 = pmmp1, p
    return p


def harmonic(order, degree, theta, phi, rt=np.float64):
    """BaseDecomposition::harmonic (:319-339): sphPlm(n, |m|, cos theta), the sign flipped for odd negative m, times e^{-i m phi}"""
    ct = types(rt)[1]
    theta, phi = rt(theta), rt(phi)
    p = sph_plm(order, abs(degree), np.cos(theta), rt)
    if degree < 0 and (-degree) % 2 == 1:
        p = -p
    a = rt(-degree) * phi
    return cx(np.cos(a) * p, np.sin(a) * p, ct)


def calculate_normalization(order, degree, rt=np.float64):
    """_calculateNormalization (:381-403)"""
    norm = np.sqrt(rt(2 * order + 1) / (rt(4.0) * rt(M_PI)))
    factor = rt(1.0)
    if degree >= 0:
        m = degree
        while m > -degree:
            factor = factor * rt(order + m)
            m -= 1
        norm = norm / np.sqrt(factor)
    else:
        m = -degree
        while m > degree:
            factor = factor * rt(order + m)
            m -= 1
        norm = norm * np.sqrt(factor)
    return norm


def calculate_pnm(order, degree, theta, rt=np.float64):
    """_calculatePnm (:421-437): the unnormalised Legendre function with the negative-degree scaling loop"""
    result = legendre_plm(order, abs(degree), np.cos(rt(theta)), rt)
    if degree < 0:
        m = -degree
        factor = rt(1.0)
        while m > degree:
            factor = factor * rt(order + m)
            m -= 1
        result = result / factor
        if (-degree) % 2 == 1:
            result = result * rt(-1)
    return result


def calculate_dpnm_dtheta(order, degree, theta, rt=np.float64):
    """_calculate_dPnm_dtheta (:440-449): d P / d x in fact; the (degree - order - 1) factor is kept for negative degree"""
    c = np.cos(rt(theta))
    c2 = c * c
    return (rt(degree - order - 1) * calculate_pnm(order + 1, degree, theta, rt) + rt(order + 1) * c * calculate_pnm(order, degree, theta, rt)) / (rt(1.0) - c2)


def harmonic_deriv_polar(order, degree, theta, phi, rt=np.float64):
    """harmonicDerivPolarAngle (:452-460)"""
    ct = types(rt)[1]
    theta, phi = rt(theta), rt(phi)
    factor = -calculate_normalization(order, degree, rt) * calculate_dpnm_dtheta(order, degree, theta, rt) * np.sin(theta)
    a = rt(-degree) * phi
    return cx(np.cos(a) * factor, np.sin(a) * factor, ct)


def harmonic_deriv_azimuth(order, degree, theta, phi, rt=np.float64):
    """harmonicDerivAzimuth (:463-472): (Y * (0 - i)) * degree"""
    ct = types(rt)[1]
    y = gmul(harmonic(order, degree, theta, phi, rt), cx(rt(0.0), rt(-1.0), ct), ct)
    return cx(y.real * rt(degree), y.imag * rt(degree), ct)


def modal_coefficient(order, ka, rt=np.float64):
    """BaseDecomposition::modalCoefficient(order, ka) (:474-628): its own closed forms for orders 0-8 in its order of operations, the Bessel
    branch above"""
    ct = types(rt)[1]
    ka = rt(ka)
    if ka == 0.0:
        return cx(rt(1.0), rt(0.0), ct)
    c, s = np.cos(ka), np.sin(ka)
    ka2 = ka * ka
    ka3 = ka2 * ka
    ka4 = ka2 * ka2
    ka5 = ka4 * ka
    ka6 = ka5 * ka
    ka7 = ka6 * ka
    ka8 = ka7 * ka
    ka9 = ka8 * ka

    def mul_real(z, x):
        return cx(z.real * x, z.imag * x, ct)

    def mul_imag(z, y):
        return cx(-y * z.imag, y * z.real, ct)

    if order == 0:
        y = rt(M_PI) * (ka / rt(M_PI))
        j0 = np.sin(y) / y if abs(ka / rt(M_PI)) >= 1e-8 else rt(1.0) - y * y / rt(6.0)
        h0 = cx(j0, -c / ka, ct)
        val1 = ka * c - s
        val2 = gmul(cx(ka, rt(1.0), ct), cx(c, s, ct), ct)
        grad = gdiv(cx(val1, rt(0.0), ct), val2, ct)
        g = gmul(grad, h0, ct)
        return cx(j0 - g.real, rt(0.0) - g.imag, ct)
    if order == 1:
        return mul_real(gdiv(cx(-c, s, ct), cx(ka2 - 2, 2 * ka, ct), ct), ka)
    if order == 2:
        return mul_imag(gdiv(cx(c, -s, ct), cx(ka3 - 9 * ka, 4 * ka2 - 9, ct), ct), ka2)
    if order == 3:
        return mul_real(gdiv(cx(c, -s, ct), cx(ka4 - 27 * ka2 + 60, 7 * ka3 - 60 * ka, ct), ct), ka3)
    if order == 4:
        return mul_real(gdiv(cx(s, c, ct), cx(ka5 - 65 * ka3 + 525 * ka, 11 * ka4 - 240 * ka2 + 525, ct), ct), ka4)
    if order == 5:
        return mul_real(gdiv(cx(c, -s, ct), cx(ka6 - 135 * ka4 + 2625 * ka2 - 5670, 16 * ka5 - 735 * ka3 + 5670 * ka, ct), ct), ka5)
    if order == 6:
        return mul_imag(gdiv(cx(c, -s, ct), cx(ka7 - 252 * ka5 + 9765 * ka3 - 72765 * ka, 22 * ka6 - 1890 * ka4 + 34020 * ka2 - 72765, ct), ct), ka6)
    if order == 7:
        return mul_real(gdiv(cx(c, -s, ct), cx(1081080 - 509355 * ka2 + 29925 * ka4 - 434 * ka6 + ka8,
                                               -1081080 * ka + 148995 * ka3 - 4284 * ka5 + 29 * ka7, ct), ct), ka7)
    if order == 8:
        return mul_real(gdiv(cx(s, c, ct), cx(18243225 * ka - 2567565 * ka3 + 79695 * ka5 - 702 * ka7 + ka9,
                                              18243225 - 8648640 * ka2 + 530145 * ka4 - 8820 * ka6 + 37 * ka8, ct), ct), ka8)
    # the Bessel branch (:590-624), double only: tests/sph_np.py's j_l / y_l
    x = float(ka)
    jn, yn = S.jl(order, x), S.yl(order, x)
    jp, jnn, yp, ynn = S.jl(order - 1, x), S.jl(order + 1, x), S.yl(order - 1, x), S.yl(order + 1, x)
    djn = (jp - jnn) / 2
    hn, hp, hnn = cx(jn, yn, ct), cx(jp, yp, ct), cx(jnn, ynn, ct)
    val = cx((hn.real + hnn.real * ka) / ka, (hn.imag + hnn.imag * ka) / ka, ct)
    dhn = cx((hp.real - val.real) * rt(0.5), (hp.imag - val.imag) * rt(0.5), ct)
    grad = gdiv(cx(rt(djn), rt(0.0), ct), dhn, ct)
    g = gmul(grad, hn, ct)
    return cx(-g.real + rt(jn), -g.imag, ct)


IN =[(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]                 # _calc_in (:299-312)


class Decomposition:
    """BaseDecomposition with spatial = False (ModalDecomposition) or True (SpatialDecomposition)"""

    def __init__(self, spatial, orderN, subbandsN, a, sampleRate, useSubbandsN=0, dtype=np.float64, reverse=False):
        self.rt, self.ct = types(dtype)
        rt, ct = self.rt, self.ct
        self.reverse = reverse
        self.spatial, self.orderN, self.modesN = bool(spatial), orderN, (orderN + 1) * (orderN + 1)
        self.subbandsN, self.subbandsN2 = subbandsN, subbandsN // 2
        self.F = self.subbandsN2 + 1
        self.useSubbandsN = self.F if useSubbandsN == 0 else useSubbandsN
        self.L = CHAN if spatial else self.modesN
        self.theta_s, self.phi_s = eigenmike(rt)
        self.modes = [(n, m) for n in range(orderN + 1) for m in range(-n, n + 1)]
        self.bn = np.zeros((self.F, orderN + 1), ct)
        for f in range(self.F):
            ka = rt(2.0) * rt(M_PI) * rt(f) * rt(a) * rt(sampleRate) / (rt(subbandsN) * rt(SSPEED))
            for n in range(orderN + 1):
                i_n = cx(rt(IN[n % 4][0]), rt(IN[n % 4][1]), ct)
                self.bn[f, n] = gmul(gmul(cx(rt(4.0) * rt(M_PI), rt(0.0), ct), i_n, ct), modal_coefficient(n, ka, rt), ct)
        self.sc = np.zeros((self.modesN, CHAN), ct)                      # _sphericalComponent: conj(Y) at the sensors
        for idx, (n, m) in enumerate(self.modes):
            for s in range(CHAN):
                self.sc[idx, s] = np.conj(harmonic(n, m, self.theta_s[s], self.phi_s[s], rt))
        self.norm = np.array([calculate_normalization(n, m, rt) for n, m in self.modes], rt)
        self.bkl = np.zeros(self.F, ct)
        self.dbt = np.zeros(self.F, ct)
        self.dbp = np.zeros(self.F, ct)
        self.g = np.zeros((self.F, self.L), ct)
        self.dgt = np.zeros((self.F, self.L), ct)
        self.dgp = np.zeros((self.F, self.L), ct)
        self.sel = []
        self.sortedAbs = None
        self._cache = (None, None)

    def dotc(self, a, b):
        """gsl_blas_zdotc: sum conj(a) b"""
        return seq(np.conj(a) * b, self.reverse)

    def at(self, theta, phi):
        """the harmonics and their derivatives of every mode at (theta, phi), and P, dP of the ddelta sum"""
        key = (theta, phi)
        if self._cache[0] != key:
            rt = self.rt
            Y = np.array([harmonic(n, m, theta, phi, rt) for n, m in self.modes], self.ct)
            Yt = np.array([harmonic_deriv_polar(n, m, theta, phi, rt) for n, m in self.modes], self.ct)
            Yp = np.array([harmonic_deriv_azimuth(n, m, theta, phi, rt) for n, m in self.modes], self.ct)
            P = np.array([calculate_pnm(n, m, theta, rt) for n, m in self.modes], rt)
            dP = np.array([calculate_dpnm_dtheta(n, m, theta, rt) for n, m in self.modes], rt)
            self._cache = (key, (Y, Yt, Yp, P, dP))
        return self._cache[1]

    def transform(self, snapshot):
        """ModalDecomposition::transform (:680-691)"""
        return np.array([self.dotc(self.sc[idx], snapshot) for idx in range(self.modesN)], self.ct)

    def calculate_gkl(self, theta, phi, f):
        Y, Yt, Yp, _, _ = self.at(theta, phi)
        order = np.array([n for n, _ in self.modes])
        if not self.spatial:                                            # :750-767
            b = self.bn[f][order]
            self.g[f], self.dgt[f], self.dgp[f] = b * Y, b * Yt, b * Yp
            return
        for s in range(CHAN):                                           # :838-870
            sums = []
            for T in (Y, Yt, Yp):
                sum_n = self.ct(0)
                for n in range(self.orderN + 1):
                    lo = n * n
                    sum_m = seq(self.sc[lo:lo + 2 * n + 1, s] * T[lo:lo + 2 * n + 1], self.reverse)
                    sum_n = sum_n + self.bn[f, n] * sum_m
                sums.append(sum_n)
            self.g[f, s], self.dgt[f, s], self.dgp[f, s] = sums

    def vkl(self, snapshot):
        return np.asarray(snapshot, self.ct) if self.spatial else self.transform(np.asarray(snapshot, self.ct))

    def estimateBkl(self, theta, phi, snapshot, f):
        """:636-678 / :775-791"""
        rt = self.rt
        self.calculate_gkl(theta, phi, f)
        v = self.vkl(snapshot)
        eta = self.dotc(self.g[f], v)
        delta = self.dotc(self.g[f], self.g[f]).real
        self.bkl[f] = eta / delta
        if not self.spatial:
            deta_dtheta = self.dotc(self.dgt[f], v)
            deta_dphi = self.dotc(self.dgp[f], v)
            _, _, _, P, dP = self.at(theta, phi)
            terms = []
            for idx, (n, m) in enumerate(self.modes):
                norm2 = rt(M_PI) * self.norm[idx] * np.hypot(self.bn[f, n].real, self.bn[f, n].imag)
                terms.append(rt(-32.0) * norm2 * norm2 * P[idx] * dP[idx] * np.sin(rt(theta)))
            ddelta = seq(np.array(terms, rt), self.reverse)
            self.dbt[f] = (deta_dtheta * delta - eta * ddelta) / (delta * delta)
            self.dbp[f] = deta_dphi / delta
        if f == self.subbandsN2:                                        # SubbandList (:52-70): |B| descending, ties to the lower bin
            ab = np.hypot(self.bkl.real, self.bkl.imag)
            order = sorted(range(self.F), key=lambda k: (-ab[k], k))
            self.sortedAbs = ab[order]
            self.sel = [(k, self.bkl[k]) for k in order[:self.useSubbandsN]]

    def linearize(self):
        """:693-723 / :793-815 -> Hbar [N][2]"""
        H = np.zeros((self.useSubbandsN * self.L, 2), self.ct)
        for x, (f, B) in enumerate(self.sel):
            r = slice(x * self.L, (x + 1) * self.L)
            if self.spatial:
                H[r, 0], H[r, 1] = B * self.dgt[f], B * self.dgp[f]
            else:
                H[r, 0] = B * self.dgt[f] + self.g[f] * self.dbt[f]
                H[r, 1] = B * self.dgp[f] + self.g[f] * self.dbp[f]
        return H

    def predictedObservation(self, theta, phi):
        """:725-747 (the harmonics at the angles given, the B of the list) / :817-836 (the stored g)"""
        y = np.zeros(self.useSubbandsN * self.L, self.ct)
        for x, (f, B) in enumerate(self.sel):
            r = slice(x * self.L, (x + 1) * self.L)
            if self.spatial:
                y[r] = self.g[f] * B
            else:
                Y = self.at(theta, phi)[0]
                y[r] = (self.bn[f][np.array([n for n, _ in self.modes])] * Y) * B
        return y


def calc_givens(v1, v2):
    norm = np.sqrt(v1 * v1 + v2 * v2)
    if norm == 0.0:
        raise ArithmeticError("calcGivensRotation: Norm is zero.")
    return norm, v1 / norm, v2 / norm


def _rotate_a22(P, n2, S_):
    """the second and third loops of _lowerTriangularize (:1206-1250) on the A22 | A23 blocks"""
    A22 = P[n2:n2 + S_, n2:n2 + S_]
    A23 = P[n2:n2 + S_, n2 + S_:n2 + 2 * S_]

    def rot(blk, rowX, colX):
        norm, c, s = calc_givens(A22[rowX, rowX], blk[rowX, colX])
        A22[rowX, rowX] = norm
        blk[rowX, colX] = 0.0
        v1, v2 = A22[rowX + 1:, rowX].copy(), blk[rowX + 1:, colX].copy()
        A22[rowX + 1:, rowX] = c * v1 + s * v2
        blk[rowX + 1:, colX] = c * v2 - s * v1

    for rowX in range(S_):
        for colX in range(rowX + 1, S_):
            rot(A22, rowX, colX)
    for rowX in range(S_):
        for colX in range(S_):
            rot(A23, rowX, colX)


def lower_triangularize(P, n2, S_=2):
    """_lowerTriangularize (:1179-1251) on the dense prearray, in place"""
    for rowX in range(n2):
        for colX in range(S_):
            norm, c, s = calc_givens(P[rowX, rowX], P[rowX, n2 + colX])
            P[rowX, rowX] = norm
            P[rowX, n2 + colX] = 0.0
            v1, v2 = P[rowX + 1:, rowX].copy(), P[rowX + 1:, n2 + colX].copy()
            P[rowX + 1:, rowX] = c * v1 + s * v2
            P[rowX + 1:, n2 + colX] = c * v2 - s * v1
    _rotate_a22(P, n2, S_)


def trsv_lower(A, x):
    """gsl_blas_dtrsv(CblasLower, CblasNoTrans, CblasNonUnit): row by row, the subtractions in column order"""
    x = x.copy()
    for i in range(len(x)):
        x[i] = np.cumsum(np.concatenate([x[i:i + 1], -(A[i, :i] * x[:i])]))[-1] / A[i, i]
    return x


def dense_update(P, n2, r):
    """the postarray, A11^-1 r and the correction B21 (A11^-1 r) of _update (:1133-1150) on a dense prearray"""
    P = P.copy()
    lower_triangularize(P, n2)
    x = trsv_lower(P[:n2, :n2], r)
    corr = np.array([seq(P[n2 + i, :n2] * x) for i in range(2)], P.dtype)
    return P, corr


def streaming_update(colfn, a0, a1, A23, r):
    """The same sweep one A11 column at a time: column j is touched only at step j, where it mixes with the two A12 columns over the rows
    >= j; it is then final and the column-oriented forward substitution consumes it at once.  colfn(j) -> rows j.. of column j of the
    prearray's first block column (length n2 + 2 - j); a0, a1: the two A12 | A22 columns (length n2 + 2).  -> (correction, A22)"""
    a0, a1, r = a0.copy(), a1.copy(), r.copy()
    n2 = len(r)
    corr = np.zeros(2, r.dtype)
    for j in range(n2):
        w = colfn(j).copy()
        for a in (a0, a1):
            norm, c, s = calc_givens(w[0], a[j])
            w[0] = norm
            a[j] = 0.0
            v1, v2 = w[1:].copy(), a[j + 1:].copy()
            w[1:] = c * v1 + s * v2
            a[j + 1:] = c * v2 - s * v1
        x = r[j] / w[0]
        r[j + 1:] = r[j + 1:] - w[1:n2 - j] * x
        corr = corr + w[n2 - j:] * x
    P = np.zeros((2, 4), r.dtype)
    P[:, 0], P[:, 1], P[:, 2:] = a0[n2:], a1[n2:], A23
    _rotate_a22(P, 0, 2)
    return corr, P[:, :2].copy()


class Tracker:
    """BaseSphericalArrayTracker + ModalSphericalArrayTracker::next (:1280-1345) / SpatialSphericalArrayTracker::next (:1356-1436)"""

    def __init__(self, dec, sigma2_u=10.0, sigma2_v=10.0, sigma2_init=10.0, maxLocalN=1):
        rt = dec.rt
        self.dec, self.rt, self.ct = dec, rt, dec.ct
        self.L, self.F, self.K_ = dec.L, dec.F, dec.useSubbandsN
        self.N = self.K_ * self.L
        self.maxLocalN = maxLocalN
        self.sigma_init = np.sqrt(rt(sigma2_init))                        # :890
        self.U = np.eye(2, dtype=rt) * np.sqrt(rt(sigma2_u))
        self.V = np.zeros((self.F, 2 * self.L, 2 * self.L), rt)            # the diagonal blocks of _V
        for f in range(self.F):
            self.V[f] = np.eye(2 * self.L, dtype=rt) * np.sqrt(rt(sigma2_v))
        self.position = np.zeros(2, rt)
        self.log = []
        self.post = None
        self.nextSpeaker()

    def nextSpeaker(self):
        self.position = np.array([0.5, 0.0], self.rt)
        self.K = np.eye(2, dtype=self.rt) * np.sqrt(self.sigma_init)      # the root taken twice (:890, :908, :928)

    def setInitialPosition(self, theta, phi):
        self.position = np.array([theta, phi], self.rt)

    def setV(self, Vk, f):
        """:961-981: the lower triangle only; the lower-left block's entries with n > m keep their previous contents"""
        L = self.L
        B = self.V[f].copy()
        Vk = np.asarray(Vk)
        for m in range(L):
            for n in range(m + 1):
                B[m, n] = B[m + L, n + L] = self.rt(Vk[m, n].real)
                B[m + L, n] = self.rt(Vk[m, n].imag)
        self.V[f] = cholesky_lower(B)

    def residual(self, vk, theta, phi):
        d = vk - self.dec.predictedObservation(theta, phi)
        return seq(d.real * d.real + d.imag * d.imag, self.dec.reverse) / self.rt(self.N)

    def realify(self, x):
        """_realify / _realifyResidual (:1077-1101): per selected bin the L real parts, then the L imaginary parts"""
        x = x.reshape((self.K_, self.L) + x.shape[1:])
        return np.concatenate([x.real, x.imag], axis=1).reshape((2 * self.N,) + x.shape[2:])

    def prearray(self, Hre):
        n2 = 2 * self.N
        P = np.zeros((n2 + 2, n2 + 4), self.rt)
        for x, (f, _) in enumerate(self.dec.sel):
            r = slice(2 * x * self.L, 2 * (x + 1) * self.L)
            P[r, r] = self.V[f]
        for i in range(2):
            for j in range(2):                                            # dgemm, beta = 0: (0 + h0 K0j) + h1 K1j
                P[:n2, n2 + j] = P[:n2, n2 + j] + Hre[:, i] * self.K[i, j]
        P[n2:, n2:n2 + 2] = self.K
        P[n2:, n2 + 2:] = self.U
        return P

    def innovation(self, vk, H, yhat, eta):
        Hre = self.realify(H)
        r = self.realify(vk) - self.realify(yhat)
        delta = self.position - eta
        r = r - (Hre[:, 0] * delta[0] + Hre[:, 1] * delta[1])
        return Hre, r

    def update(self, vk, H, yhat, eta):
        """_update (:1103-1156) + _checkPhysicalConstraints -> (eta, clamped)"""
        Hre, r = self.innovation(vk, H, yhat, eta)
        self.post, corr = dense_update(self.prearray(Hre), 2 * self.N, r)
        eta = eta + corr
        clamped = False
        if eta[0] < EPSILON:
            eta[0] = self.rt(EPSILON); clamped = True
        elif eta[0] > self.rt(M_PI) - self.rt(EPSILON):
            eta[0] = self.rt(M_PI) - self.rt(EPSILON); clamped = True
        return eta, clamped

    def next(self, snapshots):
        """snapshots [F][32] (SnapShotArray::getSnapShot per bin) -> float32 (theta, phi)"""
        dec = self.dec
        X = np.asarray(snapshots).astype(self.ct)
        eta = self.position.copy()
        rec = dict(sel=None, iters=0, clamp=False, ratios=[], sortedAbs=[])
        for localX in range(self.maxLocalN):
            theta, phi = eta[0], eta[1]
            for f in range(self.F):
                dec.estimateBkl(theta, phi, X[f], f)
            vk = np.concatenate([dec.vkl(X[f]) for f, _ in dec.sel])
            rec["sel"] = [f for f, _ in dec.sel] if rec["sel"] is None else rec["sel"]
            rec.setdefault("sels", []).append([f for f, _ in dec.sel])
            rec["sortedAbs"].append(dec.sortedAbs.copy())
            if dec.spatial:
                before = self.residual(vk, theta, phi)
                H, yhat = dec.linearize(), dec.predictedObservation(theta, phi)
                eta, cl = self.update(vk, H, yhat, eta)
                for f, _ in dec.sel:
                    dec.calculate_gkl(eta[0], eta[1], f)
            else:
                H, yhat = dec.linearize(), dec.predictedObservation(theta, phi)
                before = self.residual(vk, theta, phi)
                eta, cl = self.update(vk, H, yhat, eta)
            after = self.residual(vk, eta[0], eta[1])
            rec["clamp"] = rec["clamp"] or cl
            rec["iters"] = localX + 1
            ratio = (before - after) / (before + after)
            rec["ratios"].append(ratio)
            if ratio < TOLERANCE:
                break
        self.position = eta.copy()
        n2 = 2 * self.N
        self.K = self.post[n2:, n2:n2 + 2].copy()
        rec["pos64"] = self.position.copy()
        self.log.append(rec)
        return self.position.astype(np.float32)


def cholesky_lower(A):
    """the Cholesky factor of the symmetric matrix the lower triangle of A stands for, row by row, the strict upper part zero;
    ArithmeticError where it is not positive definite"""
    n = A.shape[0]
    Lm = np.zeros_like(A)
    for i in range(n):
        for j in range(i):
            Lm[i, j] = (A[i, j] - (seq(Lm[i, :j] * Lm[j, :j]) if j else 0)) / Lm[j, j]
        d = A[i, i] - (seq(Lm[i, :i] * Lm[i, :i]) if i else 0)
        if not d > 0:
            raise ArithmeticError("setV: the block is not positive definite")
        Lm[i, i] = np.sqrt(d)
    return Lm


def info_word(rec, error=False):
    """the packing of the device's info: bits 0-7 the local iterations used, bit 8 the clamp flag, bit 9 the error flag"""
    return rec["iters"] | (int(rec["clamp"]) << 8) | (int(error) << 9)


class PlaneWaveSimulator:
    """PlaneWaveSimulator (:1444-1488) over a ModalDecomposition"""

    def __init__(self, dec, channelX, theta, phi):
        self.dec = dec
        rt, ct = dec.rt, dec.ct
        self.coef = np.zeros(dec.F, ct)
        for f in range(dec.F):
            coefficient = ct(0)
            for n in range(dec.orderN + 1):
                coeff_n = ct(0)
                for m in range(-n, n + 1):
                    coeff_n = coeff_n + dec.sc[n * n + n + m, channelX] * harmonic(n, m, theta, phi, rt)
                coefficient = coefficient + dec.bn[f, n] * coeff_n
            self.coef[f] = coefficient

    def next(self, block):
        """block [>= M/2+1] -> [M]: bins 0..M/2 and the conjugate mirror (:1479-1484)"""
        M, M2 = self.dec.subbandsN, self.dec.subbandsN2
        out = np.zeros(M, self.dec.ct)
        for k in range(M2 + 1):
            out[k] = self.coef[k] * block[k]
            if k != 0 and k != M2:
                out[M - k] = np.conj(out[k])
        return out


def plane_wave_coefficients(dec, theta, phi):
    """[32][M/2+1]: every channel's coefficients"""
    return np.stack([PlaneWaveSimulator(dec, c, theta, phi).coef for c in range(CHAN)])
