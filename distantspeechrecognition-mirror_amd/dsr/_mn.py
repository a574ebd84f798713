"""btk/lib/mnBeamforming.py and btk/lib/GGDcEst.py through the C-ABI (include/dsr.h section 2a'): maximum negentropy beamforming under a generalised
Gaussian model for a batch, the model's training statistics on the device, its constants and update on the host, and the deterministic fp64
log / exp / digamma of csrc/det_math.h.  Built on dsr._capi._core; importing this module imports neither torch nor the library."""
import ctypes as C

import numpy as np

from ._capi import _core
from ._capi._core import DsrError, Handle, check, cur_stream, load, torch, _np, _ptr, _dev

MN_BETA_PR, MN_BETA_NRM = 0.5, 1.0


def _det(name, x):
    L = load()
    a = _np(x, np.float64); y = np.empty_like(a)
    check(getattr(L, name)(_ptr(a), _ptr(y), a.size))
    return y if y.ndim else float(y)


def det_log(x):
    return _det("dsr_det_log", x)


def det_exp(x):
    return _det("dsr_det_exp", x)


def det_psi(x):
    return _det("dsr_det_psi", x)


def ggd_constants(p):
    """fixConst for an array of shape parameters -> (Bc, lNF, NgConst, LlConst), each shaped like p"""
    L = load()
    a = _np(p, np.float64); out = [np.empty_like(a) for _ in range(4)]
    check(L.dsr_ggd_constants(_ptr(a), a.size, *[_ptr(o) for o in out]))
    return tuple(out)


def ggd_accumulate(X, p, sa, nframes=None, acc_in=None):
    """X: cuda complex64 [U][T][F]; p, sa [F]; nframes: cuda int32 [U]; acc_in [5][F] -> acc [5][F] fp64 (numpy): acc_in + acc1S, acc1P, acc2P,
    nSample, totalL of MLE4CGGaussianD.acc over every sample"""
    L = load()
    if X.dim() != 3 or X.dtype != torch.complex64:
        raise DsrError(5, "X must be complex64 [U][T][F]")
    U, T, F = X.shape
    pa, s = _np(p, np.float64), _np(sa, np.float64)
    if pa.shape != (F,) or s.shape != (F,):
        raise DsrError(5, "p and sa must have %d entries" % F)
    a_in = None
    if acc_in is not None:
        a_in = _np(acc_in, np.float64)
        if a_in.shape != (5, F):
            raise DsrError(5, "acc_in must be 5 x %d" % F)
    Xr = torch.view_as_real(X.contiguous()); acc = np.zeros((5, F))
    check(L.dsr_ggd_accumulate(_dev(Xr), _dev(nframes) if nframes is not None else None, U, T, F, _ptr(pa), _ptr(s), _ptr(a_in) if a_in is not None else None,
                               _ptr(acc), cur_stream()))
    return acc


def ggd_update(acc, p, sa, nItr=0, alpha=0.05, thresh=0.00001, floorV=10e-8, floorP=0.07, sigmaOnly=False):
    """MLE4CGGaussianD.update for F bins -> (newSa [F], newP [F], converged [F] bool)"""
    L = load()
    pa, s = _np(p, np.float64), _np(sa, np.float64); F = pa.size
    a = _np(acc, np.float64)
    if a.shape != (5, F) or s.size != F:
        raise DsrError(5, "acc must be 5 x %d" % F)
    ns, npp, cv = np.empty(F), np.empty(F), np.zeros(F, np.int32)
    check(L.dsr_ggd_update(_ptr(a), F, _ptr(pa), _ptr(s), int(nItr), alpha, thresh, floorV, floorP, int(bool(sigmaOnly)), _ptr(ns), _ptr(npp), _ptr(cv)))
    return ns, npp, cv.astype(bool)


def ggd_write_param(filename, sa, p, mean=0.0):
    check(load().dsr_ggd_write_param(str(filename).encode(), float(sa), float(p), float(mean)))


def ggd_read_param(filename):
    """-> (sa, p, mean, B, lNF)"""
    out = np.zeros(5)
    check(load().dsr_ggd_read_param(str(filename).encode(), _ptr(out)))
    return tuple(float(v) for v in out)


def ggd_write_accs(filename, acc, alpha, nItr, thresh, floorV, floorP):
    a = _np(acc, np.float64)
    check(load().dsr_ggd_write_accs(str(filename).encode(), _ptr(a), alpha, int(nItr), thresh, floorV, floorP))


def ggd_read_accs(filename, acc):
    """adds the file's statistics to acc [5] in place -> whether the file was used (its nItr is 1)"""
    used = C.c_int(0)
    assert acc.dtype == np.float64 and acc.shape == (5,) and acc.flags.c_contiguous
    check(load().dsr_ggd_read_accs(str(filename).encode(), _ptr(acc), C.byref(used)))
    return bool(used.value)


class MnBeamformer(Handle):
    """Maximum negentropy beamforming with the generalised Gaussian model (MNSubbandBeamformerGGDc_pr / _nrm) for a batch: every (utterance, bin) is one
    problem, all of them minimised by conjugate_pr in one launch.  shape [F]: the model's shape parameter per bin.  The two reference classes differ
    in the default beta only (0.5, 1.0); gamma is accepted and has no effect, as there."""

    _destroy = "dsr_mn_destroy"

    def __init__(self, fftLen, chanN, shape=None, alpha=1.0e-2, beta=MN_BETA_PR, gamma=-1.0, NC=1, nSource=1, halfBandShift=False):
        L = load()
        self.M, self.C, self.F = fftLen, chanN, fftLen // 2 + 1
        self._create(L.dsr_mn_create, fftLen, chanN, int(NC), int(nSource), int(bool(halfBandShift)))
        self.config(alpha, beta, gamma)
        self.minimizer()
        if shape is not None:
            self.setGGD(shape)

    def config(self, alpha=1.0e-2, beta=MN_BETA_PR, gamma=-1.0):
        check(_core._lib.dsr_mn_config(self.h, alpha, beta, gamma)); self.alpha, self.beta, self.gamma = alpha, beta, gamma

    def minimizer(self, MAXITNS=40, TOLERANCE=1.0e-3, STOPTOLERANCE=1.0e-2, DIFFSTOPTOLERANCE=1.0e-5, STEPSIZE=0.2):
        check(_core._lib.dsr_mn_minimizer(self.h, int(MAXITNS), TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE))

    def setGGD(self, shape):
        s = _np(shape, np.float64)
        if s.shape != (self.F,):
            raise DsrError(5, "the shape parameters must have %d entries" % self.F)
        check(_core._lib.dsr_mn_set_ggd(self.h, _ptr(s)))

    def getConstants(self):
        """-> (Bc, NgConst, log Bc), [F] each"""
        out = [np.zeros(self.F) for _ in range(3)]
        check(_core._lib.dsr_mn_get_constants(self.h, *[_ptr(o) for o in out]))
        return tuple(out)

    def setFixedWeightsFromBeamformer(self, bf):
        """the quiescent vectors and blocking matrices of a Beamformer after calcGSCWeights"""
        check(_core._lib.dsr_mn_set_fixed_weights_from_bf(self.h, bf.h))

    def setFixedWeights(self, wq, B=None):
        """wq [F][C]; B [F][C][C-1] or None for the blocking matrices of wq"""
        w = _np(wq, np.complex128)
        if w.shape != (self.F, self.C):
            raise DsrError(5, "wq must be %d x %d" % (self.F, self.C))
        b = None
        if B is not None:
            b = _np(B, np.complex128)
            if b.shape != (self.F, self.C, self.C - 1):
                raise DsrError(5, "B must be %d x %d x %d" % (self.F, self.C, self.C - 1))
        check(_core._lib.dsr_mn_set_fixed_weights(self.h, _ptr(w), _ptr(b) if b is not None else None))

    def getFixedWeights(self):
        wq = np.zeros((self.F, self.C), np.complex128); B = np.zeros((self.F, self.C, self.C - 1), np.complex128)
        check(_core._lib.dsr_mn_get_fixed_weights(self.h, _ptr(wq), _ptr(B)))
        return wq, B

    def forceStreamed(self, on=True):
        check(_core._lib.dsr_mn_force_streamed(self.h, int(bool(on))))

    def _args(self, X, nframes, sFrame, eFrame, R, fbinX):
        U, Cn, T, F = X.shape
        if Cn != self.C or F != self.F or X.dtype != torch.complex64:
            raise DsrError(5, "X must be complex64 [U][%d][T][%d]" % (self.C, self.F))
        self._keep = (torch.view_as_real(X.contiguous()), nframes)
        return (_dev(self._keep[0]), _dev(nframes) if nframes is not None else None, U, T, int(sFrame), int(T if eFrame is None else eFrame), int(R), int(fbinX))

    def _wa(self, wa, X):
        U, n = X.shape[0], self.C - 1
        if wa is None:
            return torch.zeros((U, self.F, n), dtype=torch.complex128, device=X.device)
        wa = torch.as_tensor(wa).to(device=X.device, dtype=torch.complex128)
        if tuple(wa.shape) != (U, self.F, n):
            raise DsrError(5, "the active weights must be %d x %d x %d" % (U, self.F, n))
        return wa.contiguous().clone()

    def eval(self, X, wa, nframes=None, sFrame=0, eFrame=None, R=1, fbinX=-1):
        """X: cuda complex64 [U][C][T][F]; wa [U][F][C-1] complex128; nframes: cuda int32 [U]
        -> (cost [U][F], packed gradient [U][F][2 (C-1)]) fp64"""
        a = self._args(X, nframes, sFrame, eFrame, R, fbinX); w = self._wa(wa, X); U = X.shape[0]
        cost = torch.zeros((U, self.F), dtype=torch.float64, device=X.device)
        grad = torch.zeros((U, self.F, 2 * (self.C - 1)), dtype=torch.float64, device=X.device)
        check(_core._lib.dsr_mn_eval(self.h, *a, _dev(torch.view_as_real(w)), _dev(cost), _dev(grad), cur_stream()))
        return cost, grad

    def estimate(self, X, wa=None, nframes=None, sFrame=0, eFrame=None, R=1, fbinX=-1):
        """-> (wa [U][F][C-1] complex128, info [U][F][4] int32: iterations, evaluations, failed trials, exit reason, final cost [U][F]).  wa: the
        starting point (None: zero)."""
        a = self._args(X, nframes, sFrame, eFrame, R, fbinX); w = self._wa(wa, X); U = X.shape[0]
        info = torch.zeros((U, self.F, 4), dtype=torch.int32, device=X.device)
        cost = torch.zeros((U, self.F), dtype=torch.float64, device=X.device)
        check(_core._lib.dsr_mn_estimate(self.h, *a, _dev(torch.view_as_real(w)), _dev(info), _dev(cost), cur_stream()))
        return w, info, cost

    def apply(self, X, wa):
        """Y [U][T][F] = (wq - B wa[u][f])^H X, per-utterance active weights"""
        U, Cn, T, F = X.shape
        w = self._wa(wa, X)
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        check(_core._lib.dsr_mn_apply(self.h, _dev(torch.view_as_real(X.contiguous())), U, T, _dev(torch.view_as_real(w)), _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)
