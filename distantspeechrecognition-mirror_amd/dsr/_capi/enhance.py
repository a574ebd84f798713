"""btk/dereverberation and btk/cancelVP: WPE and the subband echo cancellers."""

import numpy as np

from . import _core
from ._core import (Handle, check, cur_stream, load, torch, _ptr, _dev, _counts)


def wpe_single(Y, fftLen, lowerN, upperN, iterationsN=2, loadDb=-20.0, bandWidth=0.0, sampleRate=16000.0, nframes=None, want_filters=False, gn=None):
    """Single-channel WPE (dereverberation.cc:28-300): Y cuda complex64 [U][N][M/2+1] -> out (and the filters [U][M/2+1][P] complex128).
    gn: the filters of the utterance / block before (reset() keeps them in the reference): used as the start and overwritten."""
    load()
    U, N, F = Y.shape
    nframes = _counts(nframes, U, N, Y.device)
    out = torch.zeros((U, N, F), dtype=torch.complex64, device=Y.device)
    if gn is not None:
        check(_core._lib.dsr_wpe_single_continue(_dev(Y.contiguous()), _dev(nframes), U, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, _dev(out),
                                           _dev(gn), cur_stream()))
        return out, gn
    gn = torch.zeros((U, F, upperN - lowerN + 1), dtype=torch.complex128, device=Y.device) if want_filters else None
    check(_core._lib.dsr_wpe_single(_dev(Y.contiguous()), _dev(nframes), U, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, _dev(out),
                              _dev(gn) if want_filters else None, cur_stream()))
    return (out, gn) if want_filters else out


def wpe_multi(Y, fftLen, lowerN, upperN, iterationsN=2, loadDb=-20.0, bandWidth=0.0, sampleRate=16000.0, nframes=None, filterChan=-1, gn=None):
    """Multi-channel WPE (dereverberation.cc:281-620): Y cuda complex64 [U][C][N][M/2+1] -> (out, filters [U][C][M/2+1][C*P] complex128).
    filterChan >= 0: all channels through that channel's filter (the reference's getOutput when that channel's feature pulls first).
    gn: the filters of the utterance / block before (reset() keeps them in the reference): used as the start and overwritten."""
    load()
    U, Cn, N, F = Y.shape
    nframes = _counts(nframes, U, N, Y.device)
    out = torch.zeros((U, Cn, N, F), dtype=torch.complex64, device=Y.device)
    if gn is not None:
        if tuple(gn.shape) != (U, Cn, F, Cn * (upperN - lowerN + 1)) or gn.dtype != torch.complex128 or not gn.is_contiguous():
            raise ValueError("gn: contiguous complex128 [U][C][M/2+1][C*P] expected")
        check(_core._lib.dsr_wpe_multi_continue(_dev(Y.contiguous()), _dev(nframes), U, Cn, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate,
                                          int(filterChan), _dev(out), _dev(gn), cur_stream()))
        return out, gn
    gn = torch.zeros((U, Cn, F, Cn * (upperN - lowerN + 1)), dtype=torch.complex128, device=Y.device)
    check(_core._lib.dsr_wpe_multi(_dev(Y.contiguous()), _dev(nframes), U, Cn, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, int(filterChan),
                             _dev(out), _dev(gn), cur_stream()))
    return out, gn


class Aec(Handle):
    """Subband echo cancellers of btk/cancelVP (include/dsr.h section 2d): kind "nlms", "kalman", "block", "dtd", "info" (the information filter)
    or "sqrtinfo" (its square-root form).  The handle holds the
    parameters (SWIG defaults of cancelVP.i unless given); the adaptive state is a device buffer of the caller (newState) that apply()
    continues from and leaves behind.  played, recorded: cuda complex64 [U][T][M/2+1]."""
    KINDS = {"nlms": 0, "kalman": 1, "block": 2, "dtd": 3, "info": 8, "sqrtinfo": 9}
    FILTER, K, SIGMA2V, DTD, HISTORY, BAND, INFO, SKIPPED, RESETS = 0, 1, 2, 3, 4, 5, 6, 7, 8

    _destroy = "dsr_aec_destroy"

    def __init__(self, kind, fftLen, sampleN=1, delta=100.0, epsilon=1.0e-4, threshold=100.0, beta=0.95, sigma2=5.0, sigmau2=10e-4, sigmak2=5.0,
                 amp4play=1.0, snrTh=2.0, engTh=100.0, smooth=0.9, frameMode=0, loading=1.0e-2):
        L = load(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind); self.M = int(fftLen)
        if self.kind in (8, 9):
            self._create(L.dsr_aec_create_info, int(self.kind == 9), int(fftLen), int(sampleN))
        else:
            self._create(L.dsr_aec_create, self.kind, int(fftLen), int(sampleN))
        self.L = L.dsr_aec_sample_n(self.h); self.F = self.M // 2 + 1
        if self.kind == 0:
            check(L.dsr_aec_set_nlms(self.h, float(delta), float(epsilon), float(threshold)))
        elif self.kind == 1:
            check(L.dsr_aec_set_kalman(self.h, float(beta), float(sigma2), float(threshold)))
        else:
            check(L.dsr_aec_set_block(self.h, float(beta), float(sigmau2), float(sigmak2), float(threshold), float(amp4play)))
        if self.kind == 3:
            check(L.dsr_aec_set_dtd(self.h, float(snrTh), float(engTh), float(smooth)))
            check(L.dsr_aec_set_frame_mode(self.h, int(frameMode)))
        if self.kind in (8, 9):
            check(L.dsr_aec_set_info(self.h, float(snrTh), float(engTh), float(smooth), float(loading)))
            check(L.dsr_aec_set_frame_mode(self.h, int(frameMode)))

    def setFrameMode(self, mode):
        check(_core._lib.dsr_aec_set_frame_mode(self.h, int(mode)))

    def stateBytes(self, U):
        return int(_core._lib.dsr_aec_state_bytes(self.h, int(U)))

    def newState(self, U, device="cuda:0"):
        st = torch.zeros((self.stateBytes(U) + 7) // 8, dtype=torch.float64, device=device)
        check(_core._lib.dsr_aec_state_init(self.h, _dev(st), int(U), cur_stream()))
        return st

    def apply(self, played, recorded, nframes=None, state=None, frame0=0):
        """-> the residual E [U][T][M/2+1] complex64; frames from nframes[u] on are zero and leave the state alone.  state None: a fresh one, discarded."""
        U, T, F = played.shape
        if F != self.F or tuple(recorded.shape) != (U, T, F) or played.dtype != torch.complex64 or recorded.dtype != torch.complex64:
            raise ValueError("played, recorded: complex64 [U][T][%d] expected" % self.F)
        out = torch.zeros((U, T, F), dtype=torch.complex64, device=played.device)
        check(_core._lib.dsr_aec_apply(self.h, _dev(played.contiguous()), _dev(recorded.contiguous()), _dev(nframes) if nframes is not None else None, U, T,
                                 int(frame0), _dev(out), _dev(state) if state is not None else None, cur_stream()))
        return out

    def read(self, state, U, what):
        F, L = self.F, self.L
        shape = {0: (U, F, L), 1: (U, F, L, L), 2: (U, F), 3: (U, 3), 4: (U, F, L), 5: (U, F, 3), 6: (U, F, L), 7: (U,), 8: (U,)}[what]
        real = what in (2, 3, 5, 7, 8)
        out = np.zeros(shape, np.float64 if real else np.complex128)
        check(_core._lib.dsr_aec_state_read(self.h, _dev(state), int(U), int(what), _ptr(out), out.size * (1 if real else 2)))
        return out

    def resetFilter(self, state, U):
        check(_core._lib.dsr_aec_reset_filter(self.h, _dev(state), int(U), cur_stream()))
