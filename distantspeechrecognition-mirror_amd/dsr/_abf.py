"""btk/lib/subbandBeamforming.py through the C-ABI (include/dsr.h section 2a''): the fixed-weight and the data-adaptive subband beamformers for a
batch -- delay-and-sum, static GSC, Griffiths-Jim, sample-matrix-inversion MVDR and MPDR -- and the host helpers they are set up with.  Built on
dsr._capi._core (the common handle base); dsr._capi re-exports AdaptiveBeamformer.  Importing this module imports neither torch nor the library."""
import ctypes as C

import numpy as np

from ._capi import _core
from ._capi._core import DsrError, Handle, check, cur_stream, load, torch, _np, _ptr, _dev, E_CONSISTENCY

ABF_DS, ABF_GSC, ABF_GJ, ABF_MVDR, ABF_MPDR = 0, 1, 2, 3, 4
ABF_STATE_REGS, ABF_STATE_LDS, ABF_STATE_MEM = 0, 1, 2
ABF_KINDS = {"ds": ABF_DS, "gsc": ABF_GSC, "gj": ABF_GJ, "mvdr": ABF_MVDR, "mpdr": ABF_MPDR}


def abf_path(kind, chanN):
    """-> ((CT, CAP, residence), (bytes of the 64 lanes' state and factor, dynamic LDS of the launch)): the kernel dsr_abf_run launches for an
    adaptive kind and chanN channels; needs no device"""
    L = load()
    out = (C.c_int * 3)(); lds = (C.c_int64 * 2)()
    check(L.dsr_abf_path(int(ABF_KINDS.get(kind, kind)), int(chanN), out, lds))
    return tuple(out), tuple(lds)


def blocking_matrix(vs, NC=1):
    """calcBlockingMatrix(vs, NC) -> B [C][C - NC]"""
    v = _np(vs, np.complex128); B = np.zeros((v.size, max(v.size - NC, 0)), np.complex128)
    check(load().dsr_abf_blocking_matrix(_ptr(v), v.size, int(NC), _ptr(B)))
    return B


def null_beamformer(w_t, w_j, NC=2):
    """calcNullBeamformer(w_t, w_j, NC) -> wq [C]"""
    a, b = _np(w_t, np.complex128), _np(w_j, np.complex128); wq = np.zeros(a.size, np.complex128)
    if a.size != b.size:
        raise DsrError(5, "w_t and w_j differ in length")
    check(load().dsr_abf_null_beamformer(_ptr(a), _ptr(b), a.size, int(NC), _ptr(wq)))
    return wq


def manifold(fbinX, fftLen, chanN, sampleRate, delays, halfBandShift=False, normalize=True):
    """calcArrayManifold_f (normalize) / calcArrayManifoldWoNorm_f -> vs [chanN]"""
    d = _np(delays, np.float64); vs = np.zeros(int(chanN), np.complex128)
    if d.size != chanN:
        raise DsrError(5, "%d delays for %d channels" % (d.size, chanN))
    check(load().dsr_abf_manifold(int(fbinX), int(fftLen), int(chanN), float(sampleRate), _ptr(d), int(bool(halfBandShift)), int(bool(normalize)), _ptr(vs)))
    return vs


class AdaptiveBeamformer(Handle):
    """One beamformer of btk/lib/subbandBeamforming.py for a batch of utterances.  kind: "ds", "gsc", "gj", "mvdr", "mpdr" (or ABF_*).  The keyword
    parameters are the reference constructors'.  Every run starts new streams unless carry(True); reset() is nextSpkr()."""

    _destroy = "dsr_abf_destroy"

    def __init__(self, kind, fftLen, chanN, NC=1, halfBandShift=False, **params):
        L = load()
        self.kind = int(ABF_KINDS.get(kind, kind)); self.M, self.C, self.F, self.NC = fftLen, chanN, fftLen // 2 + 1, NC
        self._create(L.dsr_abf_create, self.kind, fftLen, chanN, int(NC), int(bool(halfBandShift)))
        self.params = dict(beta=0.999, gamma=0.0005, initDiagLoad=1.0e10, floorSubBandSigmaK=2.0e7, silThresh=1.0e10, alpha2=0.001, staticAfter=1000,
                           diagLoad=0.001, forgetFactor=0.99, end=20)
        self.config(**params)

    def config(self, **params):
        unknown = set(params) - set(self.params)
        if unknown:
            raise TypeError("unknown parameter(s) %s" % sorted(unknown))
        p = dict(self.params); p.update(params)
        check(_core._lib.dsr_abf_config(self.h, p["beta"], p["gamma"], p["initDiagLoad"], p["floorSubBandSigmaK"], p["silThresh"], p["alpha2"],
                                        int(p["staticAfter"]), p["diagLoad"], p["forgetFactor"], int(p["end"])))
        self.params = p

    @property
    def outN(self):
        """length of a final weight vector: C for MVDR (w), C - 1 for Griffiths-Jim and MPDR (wa)"""
        return self.C if self.kind == ABF_MVDR else self.C - 1

    def setFixedWeights(self, wq, B=None):
        """wq [F][C]; B [F][C][C-NC] or None for calcBlockingMatrix(wq[f], NC)"""
        w = _np(wq, np.complex128); nb = self.C - self.NC
        if w.shape != (self.F, self.C):
            raise DsrError(5, "wq must be %d x %d" % (self.F, self.C))
        b = None
        if B is not None:
            b = _np(B, np.complex128)
            if b.shape != (self.F, self.C, nb):
                raise DsrError(5, "B must be %d x %d x %d" % (self.F, self.C, nb))
        check(_core._lib.dsr_abf_set_fixed_weights(self.h, _ptr(w), _ptr(b) if b is not None else None))

    def getFixedWeights(self):
        wq = np.zeros((self.F, self.C), np.complex128); B = np.zeros((self.F, self.C, self.C - self.NC), np.complex128)
        check(_core._lib.dsr_abf_get_fixed_weights(self.h, _ptr(wq), _ptr(B)))
        return wq, B

    def setActiveWeights(self, wa):
        """setWa of the static GSC: wa [F][C-NC]"""
        w = _np(wa, np.complex128)
        if w.shape != (self.F, self.C - self.NC):
            raise DsrError(5, "wa must be %d x %d" % (self.F, self.C - self.NC))
        check(_core._lib.dsr_abf_set_active_weights(self.h, _ptr(w)))

    def carry(self, on=True):
        check(_core._lib.dsr_abf_set_carry(self.h, int(bool(on))))

    def reset(self):
        check(_core._lib.dsr_abf_reset(self.h))

    def path(self):
        return abf_path(self.kind, self.C)

    def run(self, X, nframes=None, wp=None, wpFrames=None, want_weights=True, Y=None):
        """X: cuda complex64 [U][C][T][F]; nframes, wpFrames: cuda int32 [U]; wp: cuda float32 [U][T][F] (row t scales frame t while t < wpFrames[u])
        -> (Y [U][T][F] complex64, final weights [U][F][outN] complex128 or None).  Y: an output tensor to fill."""
        if X.dim() != 4 or X.shape[1] != self.C or X.shape[3] != self.F or X.dtype != torch.complex64:
            raise DsrError(5, "X must be complex64 [U][%d][T][%d]" % (self.C, self.F))
        U, _, T, F = X.shape
        Xr = torch.view_as_real(X.contiguous())
        if wp is not None and (tuple(wp.shape) != (U, T, F) or wp.dtype != torch.float32):
            raise DsrError(5, "wp must be float32 [%d][%d][%d]" % (U, T, F))
        if wp is not None:
            wp = wp.contiguous()
        if Y is None:
            Y = torch.empty((U, T, F), dtype=torch.complex64, device=X.device)
        Yr = torch.view_as_real(Y)
        w = torch.zeros((U, F, self.outN), dtype=torch.complex128, device=X.device) if (want_weights and self.kind >= ABF_GJ) else None
        check(_core._lib.dsr_abf_run(self.h, _dev(Xr), _dev(nframes) if nframes is not None else None, U, T, _dev(wp) if wp is not None else None,
                                     _dev(wpFrames) if wpFrames is not None else None, _dev(Yr), _dev(torch.view_as_real(w)) if w is not None else None,
                                     cur_stream()))
        return Y, w
