"""Numpy fp64 restatement of the spherical-array family (btk/beamformer/modalBeamformer.{h,cc}): EigenBeamformer, SphericalDSBeamformer,
DOAEstimatorSRPEB and DOAEstimatorSRPSphDSB over whole utterances.  The spherical Bessel functions, the normalised associated Legendre
functions, the mode amplitudes (modeAmplitude :37-170), the harmonics at the sensors (:189-217, :566-601), the weights of both kinds
(:304-345, :1022-1058), the (theta, phi) grid and steering table (:793-858), the eigenbeam transform, SRP, gate, N-best and accumulators
(:860-950).  No scipy: the GPU machines may lack it.  The GPU tests check the device against it."""
import math

import numpy as np

from tests import doa_srp_np as D

SSPEED = 343740.0
EM_THETA = [69, 90, 111, 90, 32, 55, 90, 125, 148, 125, 90, 55, 21, 58, 121, 159, 69, 90, 111, 90, 32, 55, 90, 125, 148, 125, 90, 55, 21, 58, 122, 159]
EM_PHI = [0, 32, 0, 328, 0, 45, 69, 45, 0, 315, 291, 315, 91, 90, 90, 89, 180, 212, 180, 148, 180, 225, 249, 225, 180, 135, 111, 135, 269, 270, 270, 271]


def eigenmike():
    """setEigenMikeGeometry (:414-536): (a = 42 mm, theta_s [32], phi_s [32])"""
    return 42.0, np.array(EM_THETA) * np.pi / 180, np.array(EM_PHI) * np.pi / 180


def jl(l, x):
    """spherical Bessel j_l: power series below x = l + 1, upward recurrence from j_0, j_1 above"""
    if x == 0.0:
        return 1.0 if l == 0 else 0.0
    if l == 0:
        return math.sin(x) / x
    if x < l + 1.0:
        lead = 1.0
        for i in range(1, l + 1):
            lead *= x / (2.0 * i + 1.0)
        h, term, s = -0.5 * x * x, 1.0, 1.0
        for k in range(1, 200):
            term *= h / (k * (2.0 * l + 2.0 * k + 1.0))
            s += term
            if abs(term) < 1e-17 * abs(s):
                break
        return lead * s
    jm, j = math.sin(x) / x, math.sin(x) / (x * x) - math.cos(x) / x
    for n in range(1, l):
        jm, j = j, (2.0 * n + 1.0) / x * j - jm
    return j


def yl(l, x):
    """spherical Bessel y_l, x > 0: upward recurrence"""
    ym = -math.cos(x) / x
    if l == 0:
        return ym
    y = -math.cos(x) / (x * x) - math.sin(x) / x
    for n in range(1, l):
        ym, y = y, (2.0 * n + 1.0) / x * y - ym
    return y


def sph_plm(l, m, x):
    """gsl_sf_legendre_sphPlm: sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) P_l^m(x), Condon-Shortley phase included"""
    pmm = 1.0 / math.sqrt(4.0 * math.pi)
    u = math.sqrt((1.0 - x) * (1.0 + x))
    for i in range(1, m + 1):
        pmm *= -u * math.sqrt((2.0 * i + 1.0) / (2.0 * i))
    if l == m:
        return pmm
    p1 = x * math.sqrt(2.0 * m + 3.0) * pmm
    if l == m + 1:
        return p1
    p0 = pmm
    for n in range(m + 2, l + 1):
        a = math.sqrt((4.0 * n * n - 1.0) / (n * n - m * m))
        b = math.sqrt(((n - 1.0) ** 2 - m * m) / (4.0 * (n - 1.0) ** 2 - 1.0))
        p0, p1 = p1, a * (x * p1 - b * p0)
    return p1


def Y(m, n, theta, phi):
    """sphericalHarmonic(degree m, order n) (:189-217)"""
    p = sph_plm(n, abs(m), math.cos(theta))
    if m < 0 and (-m) % 2:
        p = -p
    return complex(math.cos(m * phi), math.sin(m * phi)) * p


def _gdiv(a, b):
    """gsl_complex_div"""
    s = 1.0 / math.hypot(b.real, b.imag); sbr, sbi = s * b.real, s * b.imag
    return complex((a.real * sbr + a.imag * sbi) * s, (a.imag * sbr - a.real * sbi) * s)


def _closed(n, ka):
    """orders 0-3: the reference's closed forms in its order of operations (:40-130); they cancel badly at small ka, a quirk kept"""
    s, c = math.sin(ka), math.cos(ka)
    ka2 = ka * ka; ka3 = ka2 * ka; ka4 = ka3 * ka if n != 3 else ka2 * ka2; ka5 = ka4 * ka
    j0 = math.sin(ka) / ka if abs(ka) >= 1e-8 * math.pi else 1.0 - ka * ka / 6.0
    y0 = -c / ka
    j1, y1 = (s / ka2) - (c / ka), -(c / ka2) - (s / ka)
    j2, y2 = (3 / ka3 - 1 / ka) * s - (3 / ka2) * c, -(3 / ka3 - 1 / ka) * c - (3 / ka2) * s
    if n >= 2:
        j2, y2 = (3 / ka3 - 1 / ka) * s - (3 * c / ka2), -(3 / ka3 - 1 / ka) * c - (3 * s / ka2)
    j3, y3 = (-15 + ka2) * c / ka3 - (-15 + 6 * ka2) * s / ka4, (-15 + ka2) * s / ka3 + (-15 + 6 * ka2) * c / ka4
    if n == 0:
        val1 = c / ka - s / ka2
        eika = complex(math.cos(ka), math.sin(ka))
        e = complex(ka, 1) * eika
        val2 = complex(e.real / ka2, e.imag / ka2)
        return complex(j0, 0) - _gdiv(complex(val1, 0), val2) * complex(j0, y0)
    if n == 1:
        val1 = (-0.5 / ka) * (-c / ka + s / ka2) + 0.5 * (3 * c / ka2 + s / ka - (3 - ka2) * s / ka3)
        h1 = complex(j1, y1); hd = complex(j0, y0) - complex(j2, y2) - complex(h1.real / ka, h1.imag / ka)
        return complex(j1, 0) - _gdiv(complex(val1, 0), complex(hd.real / 2, hd.imag / 2)) * h1
    if n == 2:
        val1 = 0.5 * (-c / ka + s / ka2 + (18 - ka2) * c / ka3 + (-18 + 7 * ka2) * s / ka4)
        h2 = complex(j2, y2); hd = complex(j1, y1) - complex(j3, y3) - complex(h2.real / ka, h2.imag / ka)
        return complex(j2, 0) - _gdiv(complex(val1, 0), complex(hd.real / 2, hd.imag / 2)) * h2
    val1 = 0.5 * (-3 * c / ka2 + (3 - ka2) * s / ka3 + (120 - 11 * ka2) * c / ka4 + (-120 + 51 * ka2 - ka4) * s / ka5)
    j4 = (-105 + 10 * ka2) * c / ka4 + (105 - 45 * ka2 + ka4) * s / ka5
    y4 = (-105 + 10 * ka2) * s / ka4 - (105 - 45 * ka2 + ka4) * c / ka5
    h3 = complex(j3, y3); hd = complex(j2, y2) - complex(j4, y4) - complex(h3.real / ka, h3.imag / ka)
    return complex(j3, 0) - _gdiv(complex(val1, 0), complex(hd.real / 2, hd.imag / 2)) * h3


def mode_amplitude(n, ka, closed=True):
    """b_n(ka) of a rigid sphere, j_n - (j_n' / h_n') h_n (:37-170); ka = 0 gives 1.  closed=False: the j_l / y_l formula for every order"""
    if ka == 0:
        return 1.0 + 0j
    if closed and n <= 3:
        return _closed(n, ka)
    j = lambda l: jl(l, ka) if l >= 0 else math.cos(ka) / ka           # j_{-1}(x) = cos x / x, y_{-1}(x) = sin x / x
    y = lambda l: yl(l, ka) if l >= 0 else math.sin(ka) / ka
    hn, hp, hm = complex(j(n), y(n)), complex(j(n - 1), y(n - 1)), complex(j(n + 1), y(n + 1))
    djn = (j(n - 1) - j(n) / ka - j(n + 1)) / 2
    dhn = ((hp - hm) - complex(hn.real / ka, hn.imag / ka)) / 2
    g = _gdiv(complex(djn, 0), dhn) * hn
    return complex(-g.real + j(n), -g.imag)


def mode_amplitudes(a, fs, M, maxOrder):
    """_calcModeAmplitudes: [M/2+1][maxOrder]"""
    B = np.zeros((M // 2 + 1, maxOrder), np.complex128)
    for f in range(M // 2 + 1):
        ka = 2.0 * np.pi * f * a * fs / (M * SSPEED)
        for n in range(maxOrder):
            B[f, n] = mode_amplitude(n, ka)
    return B


def harmonics_at(maxOrder, theta, phi):
    return np.array([Y(m, n, theta, phi) for n in range(maxOrder) for m in range(-n, n + 1)])


def sensor_harmonics(maxOrder, theta_s, phi_s):
    """_sh_s [dim][C] = conj Y at every sensor"""
    return np.conj(np.stack([harmonics_at(maxOrder, t, p) for t, p in zip(theta_s, phi_s)], axis=1))


def weights(kind, B_f, Yd, maxOrder, C, sigma2=0.0, normalize=False, wgain=1.0):
    """_calcWeights of one bin: kind "EB" (:304-345) or "DS" (:1022-1058); Yd = the harmonics at the direction [dim]"""
    dim = maxOrder * maxOrder
    w = np.zeros(dim, np.complex128)
    idx = 0
    for n in range(maxOrder):
        inn = [1, 1j, -1, -1j][n % 4]
        for m in range(-n, n + 1):
            if kind == "EB":
                w[idx] = np.conj(Yd[idx]) * 4 * np.pi * (inn * B_f[n]) / (dim * C * (abs(B_f[n]) ** 2 + float(np.float32(sigma2))))
            else:
                w[idx] = np.conj(Yd[idx]) * (inn * B_f[n]) * 4 * np.pi
            idx += 1
    if normalize:
        w = w * (float(np.float32(wgain)) / np.sqrt((np.abs(w) ** 2).sum()))
    return w


def look_weights(kind, B, maxOrder, C, theta, phi, **kw):
    """[M/2+1][dim]: bin 0 the DC weights (1 for n = 0), bins 1.. _calcWeights"""
    F = B.shape[0]
    Yd = harmonics_at(maxOrder, theta, phi)
    W = np.zeros((F, maxOrder * maxOrder), np.complex128)
    W[0, 0] = 1.0
    for f in range(1, F):
        W[f] = weights(kind, B[f], Yd, maxOrder, C, **kw)
    return W


def grid(minTheta, maxTheta, minPhi, maxPhi, widthTheta, widthPhi):
    """(:803-832) -> (theta [units], phi [units], nTheta, nPhi): theta-major, both accumulated by repeated addition, no swap"""
    nT = int((maxTheta - minTheta) / widthTheta + 0.5) if (maxTheta - minTheta) / widthTheta + 0.5 >= 1 else 0
    nP = int((maxPhi - minPhi) / widthPhi + 0.5) if (maxPhi - minPhi) / widthPhi + 0.5 >= 1 else 0
    th, ph = [], []
    t = float(minTheta)
    for _ in range(nT):
        p = float(minPhi)
        for _ in range(nP):
            th.append(t); ph.append(p); p += widthPhi
        t += widthTheta
    return np.array(th), np.array(ph), nT, nP


def steering_table(kind, B, maxOrder, C, thetas, phis, fbinMin, fbinMax, **kw):
    """[fbinMax+1][units][dim]: bin 0 = 1, then _calcWeights for fbinMin..fbinMax (overwrites bin 0 when fbinMin = 0)"""
    W = np.zeros((fbinMax + 1, len(thetas), maxOrder * maxOrder), np.complex128)
    for k, (t, p) in enumerate(zip(thetas, phis)):
        Yd = harmonics_at(maxOrder, t, p)
        W[0, k] = 1.0
        for f in range(fbinMin, fbinMax + 1):
            W[f, k] = weights(kind, B[f], Yd, maxOrder, C, **kw)
    return W


def transform(X, S):
    """F = S X per bin and frame (sphericalHarmonicsTransformation, zdotu): X [C][T][F] -> [T][F][dim]"""
    return np.einsum("dc,ctf->tfd", S, X.astype(np.complex128))


def apply(X, nframes, S, Wl):
    """the beamformer over a batch: X [U][C][T][F] -> (y [U][T][F], F [U][T][F][dim]); frames past nframes stay 0"""
    U, C, T, F = X.shape
    y = np.zeros((U, T, F), np.complex128); Fo = np.zeros((U, T, F, S.shape[0]), np.complex128)
    for u in range(U):
        N = min(int(nframes[u]), T)
        Fu = transform(X[u, :, :N], S)
        Fo[u, :N] = Fu
        y[u, :N] = np.einsum("fd,tfd->tf", np.conj(Wl), Fu)
    return y, Fo


def response_power(X, S, W, fbinMin, fbinMax, M):
    """(:874-889) -> (rp [T][units], the last unit's values [T][fbinMax+1])"""
    Fu = transform(X[:, :, :fbinMax + 1], S)                             # [T][f][dim]
    T, nU = X.shape[1], W.shape[1]
    rp = np.zeros((T, nU)); last = np.zeros((T, fbinMax + 1), np.complex128)
    for f in range(fbinMin, fbinMax + 1):
        v = Fu[:, f] @ np.conj(W[f]).T                                     # [T][units]
        last[:, f] = v[:, -1]
        rp += (2.0 if f < M // 2 else 1.0) * (v.real ** 2 + v.imag ** 2)
    return rp / (fbinMax - fbinMin + 1), last


def run(X, nframes, S, W, M, nBest, fbinMin, fbinMax, threshold, acc=None):
    """X [U][C][T][M/2+1] complex64 -> dict as doa_srp_np.run, units in place of theta"""
    U, C, T, F = X.shape
    nU = W.shape[1]
    out = dict(energy=np.zeros((U, T), np.float32), rp=np.zeros((U, T, nU)), gated=np.zeros((U, T), np.int32),
               nbest_rp=np.zeros((U, T, nBest)), nbest_idx=np.zeros((U, T, nBest), np.int64),
               acc=np.zeros((U, nU)) if acc is None else np.array(acc, np.float64), y=np.zeros((U, T, F), np.complex128))
    for u in range(U):
        N = min(int(nframes[u]), T)
        if N == 0:
            continue
        Xu = X[u, :, :N]
        e = D.energy(Xu, fbinMin, fbinMax, M)
        rp, last = response_power(Xu, S, W, fbinMin, fbinMax, M)
        out["energy"][u, :N] = e; out["rp"][u, :N] = rp
        out["y"][u, :N, fbinMin:fbinMax + 1] = last[:, fbinMin:fbinMax + 1]
        for t in range(N):
            R, I = np.full(nBest, -10e10), np.full(nBest, -1)
            if e[t] < np.float32(threshold):
                out["gated"][u, t] = 1
            else:
                R, I = D.nbest(rp[t], nBest)
                out["acc"][u] += rp[t]
            out["nbest_rp"][u, t] = R; out["nbest_idx"][u, t] = I
    return out


def plane_wave(B, S_unused, theta_s, phi_s, theta0, phi0, maxOrder, T, seed=5):
    """snapshots [C][T][F] of a rigid-sphere plane wave from (theta0, phi0): p_c(f) = s_t(f) 4 pi sum_n i^n b_n(f) sum_m conj(Y_n^m(theta0, phi0))
    Y_n^m(theta_c, phi_c), the same b_n the handle uses, a random source spectrum per frame"""
    rng = np.random.default_rng(seed)
    F = B.shape[0]
    Y0 = np.conj(harmonics_at(maxOrder, theta0, phi0))
    Ys = np.stack([harmonics_at(maxOrder, t, p) for t, p in zip(theta_s, phi_s)])   # [C][dim]
    nidx = np.array([n for n in range(maxOrder) for m in range(-n, n + 1)])
    resp = np.zeros((len(theta_s), F), np.complex128)
    for f in range(F):
        g = 4 * np.pi * np.array([1, 1j, -1, -1j])[nidx % 4] * B[f, nidx]
        resp[:, f] = Ys @ (g * Y0)
    s = rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))
    return (resp[:, None, :] * s[None]).astype(np.complex64)
