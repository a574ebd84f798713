"""Numpy fp64 restatement of the further spherical-array beamformers (btk/beamformer/modalBeamformer.cc): SphericalHWNCBeamformer (:1387-1478),
SphericalGSCBeamformer / SphericalHWNCGSCBeamformer (:1483-1713, calcOutputOfGSC beamformer.cc:1251-1287, _calcBlockingMatrix :398-479,
calcSidelobeCancellerP_f :761-783), SphericalMOENBeamformer (:1804-2099), SphericalSpatialDSBeamformer (:2106-2270), both getBeamPattern
(:756-787, :2068-2099), the fold v = S^H w and the multi-beam apply.  Written from the reference line by line on top of tests/sph_np.py (mode
amplitudes and harmonics).  MOEN's inverse is the library's dsr_pseudoinverse: the reference's single-precision LINPACK SVD, pinned by
tests/test_oracle_cpu.py::test_pseudoinverse_pinned_by_linpack."""
import ctypes as C

import numpy as np

from tests import sph_np as S

IN = [1, 1j, -1, -1j]


def f32(x):
    return float(np.float32(x))


def hwnc_wng(B, Cn, ratio):
    """SphericalHWNCBeamformer::calcWNG (:1397-1418): [M/2+1], n < maxOrder"""
    n = np.arange(B.shape[1])
    return Cn / (16 * np.pi * np.pi) * ((2 * n + 1) * np.abs(B) ** 2).sum(axis=1) * f32(ratio)


def hwnc_weights(B_f, Yd, maxOrder, Cn, ratio, sigma2=0.0):
    """SphericalHWNCBeamformer::_calcWeights (:1426-1478): the HMDI weights, then the gain rule (normalizeWeights takes its gain as a float)"""
    w = S.weights("EB", B_f, Yd, maxOrder, Cn, sigma2=sigma2)
    if f32(ratio) > 0.0:
        wng = hwnc_wng(B_f[None], Cn, ratio)[0]
        return w * (f32(2 * np.sqrt(np.pi / (Cn * wng))) / np.sqrt((np.abs(w) ** 2).sum()))
    return w * ((16 * np.pi * np.pi) / (Cn * maxOrder * maxOrder))


def modal_look(kind, B, maxOrder, Cn, theta, phi, ratio=1.0, sigma2=0.0, normalize=False, wgain=1.0):
    """[M/2+1][dim] of kind "HWNC" / "HWNCGSC" (HWNC weights) or "DS" / "GSC" (SphericalDSBeamformer weights): bin 0 the DC weights"""
    if kind in ("DS", "GSC"):
        return S.look_weights("DS", B, maxOrder, Cn, theta, phi, normalize=normalize, wgain=wgain)
    Yd = S.harmonics_at(maxOrder, theta, phi)
    W = np.zeros((B.shape[0], maxOrder * maxOrder), np.complex128)
    W[0, 0] = 1.0
    for f in range(1, B.shape[0]):
        W[f] = hwnc_weights(B[f], Yd, maxOrder, Cn, ratio, sigma2)
    return W


def _gmul(ar, ai, br, bi):
    """gsl_complex_mul on (re, im) arrays"""
    return ar * br - ai * bi, ar * bi + ai * br


def _seq(x):
    """the sum of x in index order, as a C loop accumulates it (numpy's own sum is pairwise)"""
    return np.cumsum(x)[-1]


def blocking_matrix(d, NC):
    """_calcBlockingMatrix (beamformer.cc:398-479): I - conj(d) d^T / ||d||^2, its first len(d) - NC columns orthonormalised by classical
    Gram-Schmidt.  Over the 63 columns of an order-8 quiescent vector that recursion amplifies a last-bit difference to 1e-5, so this is
    written operation by operation (real arithmetic, sums in index order) and agrees with a C loop bit for bit rather than to rounding."""
    d = np.asarray(d, np.complex128)
    n = len(d); bs = n - NC
    dr, di = d.real.copy(), d.imag.copy()
    nrm = np.sqrt(_seq(dr * dr + di * di)); nrm = nrm * nrm
    x = -1.0 / nrm
    cr, ci = x * dr, x * -di                                             # alpha conj(d)
    Pr, Pi = _gmul(cr[:, None], ci[:, None], dr[None, :], di[None, :])
    Pr = np.eye(n) + Pr; Pi = 0.0 + Pi
    Br, Bi = np.zeros((n, bs)), np.zeros((n, bs))
    for i in range(bs):
        vr, vi = Pr[:, i].copy(), Pi[:, i].copy()
        for j in range(i):
            tr, ti = _gmul(Br[:, j], -Bi[:, j], vr, vi)                  # zdotc(B_j, vec)
            ipr, ipi = (0.0 + _seq(tr)) * -1.0, (0.0 + _seq(ti)) * -1.0
            ar, ai = _gmul(ipr, ipi, Br[:, j], Bi[:, j])
            vr, vi = vr + ar, vi + ai
        nv = np.sqrt(_seq(vr * vr + vi * vi))
        Br[:, i], Bi[:, i] = vr * (1.0 / nv), vi * (1.0 / nv)
    return Br + 1j * Bi


def gsc_blocking_matrix(wq, NC):
    """the spherical GSC kinds' B for a quiescent vector wq: _calcBlockingMatrix of conj(wq) (the routine blocks the conjugate of its
    argument), then every column projected once against wq (classical Gram-Schmidt loses that orthogonality over many columns)"""
    wq = np.asarray(wq, np.complex128)
    Bm = blocking_matrix(np.conj(wq), NC)
    return Bm - np.outer(wq, (np.conj(wq) @ Bm) / (np.abs(wq) ** 2).sum())


def sidelobe_wl(Bm, packed):
    """calcSidelobeCancellerP_f (beamformer.cc:761-783): wl = B wa, wa from (re, im) pairs"""
    p = np.asarray(packed, np.float64)
    return Bm @ (p[0::2] + 1j * p[1::2])


def gsc_effective(wq, wl, normalize):
    """what calcOutputOfGSC applies (beamformer.cc:1251-1287) at bins >= 1, bin 0 wq alone (:1508-1516): [M/2+1][dim]"""
    e = np.array(wq, np.complex128)
    for f in range(1, e.shape[0]):
        e[f] = wq[f] - wl[f]
        if normalize:
            e[f] = e[f] / (np.sqrt((np.abs(e[f]) ** 2).sum()) * e.shape[1])
    return e


def spatial_ds(B, Sh, maxOrder, theta, phi):
    """SphericalSpatialDSBeamformer::_calcWeights for bins 0..M/2 (:2119-2172, :2258): [M/2+1][C]"""
    Cn = Sh.shape[1]
    Yd = S.harmonics_at(maxOrder, theta, phi)
    nidx = np.array([n for n in range(maxOrder) for m in range(-n, n + 1)])
    W = np.zeros((B.shape[0], Cn), np.complex128)
    for f in range(B.shape[0]):
        inbn = np.array([IN[n % 4] * B[f, n] for n in range(maxOrder)])
        t = np.conj(Sh) * np.conj(Yd)[:, None]                       # [dim][C]
        per_n = np.stack([t[nidx == n].sum(axis=0) for n in range(maxOrder)])
        W[f] = (inbn[:, None] * per_n).sum(axis=0) * (4 * np.pi / Cn)
    return W


def pinv_linpack(dsr, A, thr=1e-8):
    n, p = A.shape
    A = np.ascontiguousarray(A, np.complex128); out = np.zeros((p, n), np.complex128); ok = C.c_int(0)
    dsr.check(dsr.load().dsr_pseudoinverse(A.ctypes.data_as(C.c_void_p), n, p, C.c_float(thr), out.ctypes.data_as(C.c_void_p), C.byref(ok), None))
    return out


def moen(dsr, B, Sh, maxOrder, theta, phi, diag=None, fixed=False, normalize=False, wgain=1.0):
    """SphericalMOENBeamformer (:1937-2040): [M/2+1][C]; bin 0 calcDCWeights into the C-long, zeroed vector.  The normal matrix goes through a
    single-precision SVD whose small singular values are noise, and the products after it cancel by several digits: a last-bit difference in
    its input moves the weights by 1e-8 and more.  So the products are written operation by operation (gsl_complex_mul, sums in index order),
    as blocking_matrix is, and agree with a C loop bit for bit."""
    F, Cn, dim = B.shape[0], Sh.shape[1], Sh.shape[0]
    Yd = S.harmonics_at(maxOrder, theta, phi)
    nidx = np.array([n for n in range(maxOrder) for m in range(-n, n + 1)])
    CN = 2.0 / (maxOrder * maxOrder)
    BNr, BNi = Yd.real * (2 * np.pi), -Yd.imag * (2 * np.pi)
    W = np.zeros((F, Cn), np.complex128)
    W[0, 0] = 1.0
    for f in range(1, F):
        if fixed:
            w = np.zeros(Cn, np.complex128)                          # _fixedW freed and zeroed before use (:1993-1996, :2031-2034)
        else:
            inbn = np.array([IN[n % 4] * B[f, n] for n in nidx])
            Ar, Ai = _gmul(Sh.real, Sh.imag, inbn.real[:, None], inbn.imag[:, None])
            Ar, Ai = Ar * (4 * np.pi), Ai * (4 * np.pi)              # _A [dim][C] (:1969-1972)
            lam = 0.0 if diag is None else f32(diag[f])
            tr, ti = _gmul(Ar[:, :, None], -Ai[:, :, None], Ar[:, None, :], Ai[:, None, :])   # conj(A[d][i]) A[d][j]
            Gr, Gi = np.cumsum(tr, axis=0)[-1], np.cumsum(ti, axis=0)[-1]
            iu = np.triu_indices(Cn, 1)                              # zherk's upper triangle, mirrored (:2009-2013)
            Gr[iu[1], iu[0]] = Gr[iu]; Gi[iu[1], iu[0]] = -Gi[iu]
            Gr[np.diag_indices(Cn)] += lam; Gi[np.diag_indices(Cn)] = 0.0
            P = pinv_linpack(dsr, Gr + 1j * Gi)
            tr, ti = _gmul(P.real[:, None, :], P.imag[:, None, :], Ar[None, :, :], -Ai[None, :, :])   # _fixedW [C][dim] = P A^H (:2027)
            Wr, Wi = np.cumsum(tr, axis=2)[:, :, -1], np.cumsum(ti, axis=2)[:, :, -1]
            tr, ti = _gmul(Wr, Wi, BNr[None, :], BNi[None, :])
            w = (np.cumsum(tr, axis=1)[:, -1] * CN) + 1j * (np.cumsum(ti, axis=1)[:, -1] * CN)
        if normalize:
            with np.errstate(divide="ignore", invalid="ignore"):
                w = w * (f32(wgain) / np.sqrt((np.abs(w) ** 2).sum()))
        W[f] = w
    return W


def plane_wave_on_sphere(ka, theta, phi, theta_s, phi_s):
    """planeWaveOnSphericalAperture (:737-747)"""
    return np.exp(1j * ka * (np.sin(theta_s) * np.sin(theta) * np.cos(phi_s - phi) + np.cos(theta_s) * np.cos(theta)))


def pattern_grid(minTheta, maxTheta, minPhi, maxPhi, widthTheta, widthPhi):
    """(:759-772): sizes through a float, theta and phi accumulated by addition"""
    nT = int(np.float32((maxTheta - minTheta) / widthTheta + 0.5 + 1)); nP = int(np.float32((maxPhi - minPhi) / widthPhi + 0.5 + 1))
    th, t = [], float(minTheta)
    for _ in range(nT):
        th.append(t); t += widthTheta
    ph, p = [], float(minPhi)
    for _ in range(nP):
        ph.append(p); p += widthPhi
    return np.array(th), np.array(ph)


def beam_pattern(mode, w, fbinX, a, fs, M, theta_s, phi_s, Sh, grid):
    """mode "modal": |w^H (S p)| (:756-787); "moen": |sum w p| (zdotu, :2068-2099); "sensor": |w^H p| (SpatialDS)"""
    th, ph = pattern_grid(*grid)
    ka = 2.0 * np.pi * fbinX * a * fs / (M * S.SSPEED)
    out = np.zeros((len(th), len(ph)))
    for i, t in enumerate(th):
        for j, p_ in enumerate(ph):
            p = plane_wave_on_sphere(ka, t, p_, theta_s, phi_s)
            out[i, j] = abs(np.vdot(w, Sh @ p)) if mode == "modal" else abs((w * p).sum()) if mode == "moen" else abs(np.vdot(w, p))
    return out


def fold(w, Sh):
    """v [F][C] = S^H w per bin: v^H x = w^H (S x)"""
    return w @ np.conj(Sh)


def beams(X, nframes, V):
    """X [U][C][T][F], V [NB][F][C] -> Y [U][NB][T][F] = v^H x, rows past nframes zero"""
    U, Cn, T, F = X.shape
    Y = np.zeros((U, V.shape[0], T, F), np.complex128)
    for u in range(U):
        N = min(int(nframes[u]), T)
        Y[u, :, :N] = np.einsum("bfc,ctf->btf", np.conj(V), X[u, :, :N].astype(np.complex128))
    return Y
