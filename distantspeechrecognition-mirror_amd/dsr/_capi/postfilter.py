"""btk/postfilter: the array post-filters, spectral subtraction, Wiener and binaural mask filters."""
import ctypes as C

import numpy as np

from . import _core
from ._core import (Handle, check, cur_stream, load, torch, _np, _ptr, _dev, _nf, _counts, _state)


PF_ZEL_REG, PF_ZEL_SUM, PF_ZEL_SUM_BF, PF_MCCOWAN_REG, PF_MCCOWAN_MEM, PF_WAVE = 0, 1, 2, 3, 4, 5


def zelinski_path(kind, chanN, bf=None):
    """-> (cell, template argument): the kernels a post-filter of that kind (0 Zelinski, 1 McCowan, 2 Lefkimmiatis) launches, behind the beamformer bf
    (apply_bf) or on its own (apply); PF_*; follows DSR_PF_SUM / DSR_PF_NOFUSE / DSR_PF_WAVE / DSR_PF_MEMSTATE; needs no device"""
    L = load()
    out = (C.c_int * 2)()
    check(L.dsr_zelinski_path(int(kind), int(chanN), bf.h if bf is not None else None, out))
    return tuple(out)


class ZelinskiPostFilter(Handle):
    kind = 0
    """Zelinski post-filter (postfilter.cc:8-221,350-493); manifold [M/2+1][C] complex = arrayManifold() (or wq() with type | 8)."""

    _destroy = "dsr_zelinski_destroy"

    def __init__(self, fftLen, chanN, manifold, alpha=0.6, type=2, minFrames=0):
        L = load(); self.M, self.C = fftLen, chanN
        self._create(L.dsr_zelinski_create, fftLen, chanN, alpha, type, minFrames)
        m = np.ascontiguousarray(manifold, np.complex128)
        for f in range(fftLen // 2 + 1):
            check(L.dsr_zelinski_set_manifold(self.h, f, _ptr(m[f])))

    def apply(self, X, Y, nframes=None, want_weights=False):
        """X: cuda complex64 [U][C][T][F], Y: [U][T][F] -> out [U][T][F] (and the weights [U][T][F] fp32)"""
        U, Cn, T, F = X.shape
        nframes = _counts(nframes, U, T, X.device)
        out = torch.zeros((U, T, F), dtype=torch.complex64, device=X.device)
        w = torch.zeros((U, T, F), dtype=torch.float32, device=X.device) if want_weights else None
        check(_core._lib.dsr_zelinski_apply(self.h, _dev(X.contiguous()), _dev(Y.contiguous()), _dev(nframes), U, T, _dev(out), _dev(w) if want_weights else None, cur_stream()))
        return (out, w) if want_weights else out

    def apply_bf(self, bf, X, nframes=None, want_weights=False, want_bf_output=False):
        """The post-filter behind its beamformer (setBeamformer, postfilter.cc:376): out = postfilter(X, bf(X)); the beamformer's sum is formed in the filter's own
        pass over the snapshots where it streams them.  X: cuda complex64 [U][C][T][F] -> out [U][T][F] (+ the weights, + bf(X))"""
        U, Cn, T, F = X.shape
        nframes = _counts(nframes, U, T, X.device)
        out = torch.zeros((U, T, F), dtype=torch.complex64, device=X.device)
        w = torch.zeros((U, T, F), dtype=torch.float32, device=X.device) if want_weights else None
        Y = torch.zeros((U, T, F), dtype=torch.complex64, device=X.device) if want_bf_output else None
        check(_core._lib.dsr_zelinski_apply_bf(self.h, bf.h, _dev(X.contiguous()), _dev(nframes), U, T, _dev(out), _dev(w) if want_weights else None,
                                         _dev(Y) if want_bf_output else None, cur_stream()))
        r = (out,) + ((w,) if want_weights else ()) + ((Y,) if want_bf_output else ())
        return r if len(r) > 1 else out

    def carry(self, on=True):
        """keep the spectral densities from call to call (block streaming)"""
        check(_core._lib.dsr_zelinski_carry(self.h, int(bool(on))))

    def resetState(self):
        check(_core._lib.dsr_zelinski_reset_state(self.h))

    def path(self, bf=None):
        """zelinski_path of this filter: what apply (bf None) / apply_bf(bf) launches"""
        return zelinski_path(self.kind, self.C, bf)


class McCowanPostFilter(ZelinskiPostFilter):
    """McCowan post-filter (postfilter.cc:502-945): Zelinski's recursions + a noise coherence matrix per bin."""
    kind = 1

    def __init__(self, fftLen, chanN, manifold, alpha=0.6, type=2, minFrames=0, threshold=0.99):
        L = load(); self.M, self.C = fftLen, chanN
        self._create(L.dsr_mccowan_create, fftLen, chanN, alpha, type, minFrames, threshold)
        m = np.ascontiguousarray(manifold, np.complex128)
        for f in range(fftLen // 2 + 1):
            check(L.dsr_zelinski_set_manifold(self.h, f, _ptr(m[f])))

    def setDiffuseNoiseModel(self, micPositions, sampleRate, sspeed=343740.0):
        mp = _np(micPositions, np.float64); check(_core._lib.dsr_mccowan_set_diffuse_noise_model(self.h, _ptr(mp), sampleRate, sspeed)); return True

    def setNoiseSpatialSpectralMatrix(self, fbinX, Rnn):
        r = np.ascontiguousarray(Rnn, np.complex128); check(_core._lib.dsr_mccowan_set_noise_matrix(self.h, fbinX, _ptr(r))); return True

    def setAllLevelsOfDiagonalLoading(self, w):
        check(_core._lib.dsr_mccowan_diagonal_loading(self.h, -1, w))

    def setLevelOfDiagonalLoading(self, fbinX, w):
        check(_core._lib.dsr_mccowan_diagonal_loading(self.h, fbinX, w))

    def divideAllNonDiagonalElements(self, myu):
        check(_core._lib.dsr_mccowan_divide_nondiagonal(self.h, myu))


class LefkimmiatisPostFilter(McCowanPostFilter):
    """Lefkimmiatis post-filter (postfilter.cc:948-1210): McCowan's clean-signal estimate against the coherence-based noise estimate,
    divided by d^H pinv(R) d from bin fbinX1 on."""
    kind = 2

    def __init__(self, fftLen, chanN, manifold, minSV=1e-8, fbinX1=0, alpha=0.6, type=2, minFrames=0, threshold=0.99):
        L = load(); self.M, self.C = fftLen, chanN
        self._create(L.dsr_lefkimmiatis_create, fftLen, chanN, minSV, fbinX1, alpha, type, minFrames, threshold)
        m = np.ascontiguousarray(manifold, np.complex128)
        for f in range(fftLen // 2 + 1):
            check(L.dsr_zelinski_set_manifold(self.h, f, _ptr(m[f])))


class SpectralSubtractor(Handle):
    """SpectralSubtractor with its averagePSDEstimators (spectralsubtraction.cc:52-267) over dsr_specsub_* (include/dsr.h 6a-2).  The noise
    estimates are a device buffer of the caller (newState), as with Gcc."""

    _destroy = "dsr_specsub_destroy"

    def __init__(self, fftLen, halfBandShift=False, ft=1.0, flooringV=0.001):
        L = load(); self.M = int(fftLen); self.F = self.M // 2 + 1
        self._create(L.dsr_specsub_create, self.M, int(bool(halfBandShift)), float(ft), float(flooringV))

    def setChannel(self, alpha=-1.0):
        check(_core._lib.dsr_specsub_set_channel(self.h, float(alpha)))

    def chanN(self):
        return int(_core._lib.dsr_specsub_chan_n(self.h))

    def newState(self, U, device="cuda:0"):
        st = _state(_core._lib.dsr_specsub_state_bytes(self.h, int(U)), device); st.U = int(U)
        check(_core._lib.dsr_specsub_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def setNoiseOverEstimationFactor(self, ft):
        check(_core._lib.dsr_specsub_set_noise_over_estimation_factor(self.h, float(ft)))

    def startTraining(self):
        check(_core._lib.dsr_specsub_start_training(self.h))

    def stopTraining(self, state=None):
        check(_core._lib.dsr_specsub_stop_training(self.h, _dev(state) if state is not None else None, state.U if state is not None else 0, cur_stream() if state is not None else None))

    def startNoiseSubtraction(self):
        check(_core._lib.dsr_specsub_set_noise_subtraction(self.h, 1))

    def stopNoiseSubtraction(self):
        check(_core._lib.dsr_specsub_set_noise_subtraction(self.h, 0))

    def clear(self, state):
        check(_core._lib.dsr_specsub_clear(self.h, _dev(state), state.U, cur_stream()))

    def clearNoiseSamples(self, state):
        check(_core._lib.dsr_specsub_clear_noise_samples(self.h, _dev(state), state.U, cur_stream()))

    def readNoiseFile(self, fn, state, idx=0):
        check(_core._lib.dsr_specsub_read_noise_file(self.h, str(fn).encode(), int(idx), _dev(state), state.U)); return True

    def writeNoiseFile(self, fn, state, idx=0, u=0):
        check(_core._lib.dsr_specsub_write_noise_file(self.h, str(fn).encode(), int(idx), _dev(state), state.U, int(u))); return True

    def apply(self, X, state, nframes=None, full=False, train_only=False):
        """X cuda complex64 [U][C][T][F] -> [U][T][F] complex64 ([U][T][fftLen] with full); train_only: addSample alone, no output"""
        U, Cn, T, F = X.shape
        if Cn != self.chanN() or F != self.F or X.dtype != torch.complex64:
            raise ValueError("X: complex64 [U][%d][T][%d] expected" % (self.chanN(), self.F))
        nb = self.M if full else self.F
        out = None if train_only else torch.zeros((U, T, nb), dtype=torch.complex64, device=X.device)
        check(_core._lib.dsr_specsub_apply(self.h, _dev(X.contiguous()), _nf(nframes), U, T, _dev(out) if out is not None else None, nb, 0, _dev(state), cur_stream()))
        return out

    def read(self, state, what, u, chan):
        out = np.zeros(2 if what == 2 else self.F); check(_core._lib.dsr_specsub_state_read(self.h, _dev(state), state.U, int(what), int(u), int(chan), _ptr(out), out.size))
        return out


class WienerFilter(Handle):
    """WienerFilter (spectralsubtraction.cc:269-347) over dsr_wiener_*"""

    _destroy = "dsr_wiener_destroy"

    def __init__(self, fftLen, halfBandShift=False, alpha=0.0, flooringV=0.001, beta=1.0, noiseLen=None):
        L = load(); self.M = int(fftLen); self.F = self.M // 2 + 1
        self._create(L.dsr_wiener_create, self.M, int(self.M if noiseLen is None else noiseLen), int(bool(halfBandShift)), float(alpha), float(flooringV), float(beta))

    def setNoiseAmplificationFactor(self, beta):
        check(_core._lib.dsr_wiener_set_noise_amplification_factor(self.h, float(beta)))

    def startUpdatingNoisePSD(self):
        check(_core._lib.dsr_wiener_set_updating_noise_psd(self.h, 1))

    def stopUpdatingNoisePSD(self):
        check(_core._lib.dsr_wiener_set_updating_noise_psd(self.h, 0))

    def carry(self, on=True):
        check(_core._lib.dsr_wiener_carry(self.h, int(bool(on))))

    def newState(self, U, device="cuda:0"):
        st = _state(_core._lib.dsr_wiener_state_bytes(self.h, int(U)), device); st.U = int(U)
        check(_core._lib.dsr_wiener_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def resetState(self, state):
        check(_core._lib.dsr_wiener_reset_state(self.h, _dev(state), state.U, cur_stream()))

    def apply(self, S, N, state, nframes=None, full=False):
        """S, N cuda complex64 [U][T][F] -> [U][T][F] (or [U][T][fftLen])"""
        U, T, F = S.shape; nb = self.M if full else self.F
        out = torch.zeros((U, T, nb), dtype=torch.complex64, device=S.device)
        check(_core._lib.dsr_wiener_apply(self.h, _dev(S.contiguous()), _dev(N.contiguous()) if N is not None else None, _nf(nframes), U, T, _dev(out), nb, 0, _dev(state), cur_stream()))
        return out

    def read(self, state, what, u):
        out = np.zeros(1 if what == 2 else self.F); check(_core._lib.dsr_wiener_state_read(self.h, _dev(state), state.U, int(what), int(u), _ptr(out), out.size)); return out


class BinaryMask(Handle):
    """BinaryMaskFilter ("base"), KimBinaryMaskFilter ("kim"), IIDBinaryMaskFilter ("iid") (binauralprocessing.cc:47-211, 431-520) over dsr_binmask_*"""
    KINDS = {"base": 0, "kim": 1, "iid": 2}

    _destroy = "dsr_binmask_destroy"

    def __init__(self, kind, chanX, fftLen, threshold, alpha, dEta=0.01, dPowerCoeff=0.0):
        L = load(); self.M = int(fftLen); self.F = self.M // 2 + 1; self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self._create(L.dsr_binmask_create, self.kind, int(chanX), self.M, float(threshold), float(alpha), float(dEta), float(dPowerCoeff))

    def setThreshold(self, threshold):
        check(_core._lib.dsr_binmask_set_threshold(self.h, float(threshold)))

    def getThreshold(self):
        return float(_core._lib.dsr_binmask_threshold(self.h))

    def setThresholds(self, thresholds):
        t = _np(thresholds, np.float64); check(_core._lib.dsr_binmask_set_thresholds(self.h, _ptr(t), t.size))

    def getThresholds(self):
        out = np.zeros(self.F); ex = C.c_int32(0); check(_core._lib.dsr_binmask_thresholds(self.h, _ptr(out), out.size, C.byref(ex)))
        return out if ex.value else None

    def carry(self, on=True):
        check(_core._lib.dsr_binmask_carry(self.h, int(bool(on))))

    def newState(self, U, device="cuda:0"):
        st = torch.zeros((int(U), self.F), dtype=torch.float32, device=device); st.U = int(U)
        check(_core._lib.dsr_binmask_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def resetState(self, state):
        check(_core._lib.dsr_binmask_reset_state(self.h, _dev(state), state.U, cur_stream()))

    def apply(self, L, R, state, nframes=None, full=False, want_mu=False, want_itd=False):
        """L, R cuda complex64 [U][T][F] -> dict(out [U][T][F] or [U][T][fftLen], mu float32 [U][T][F], itd float64 [U][T][F])"""
        U, T, F = L.shape; nb = self.M if full else self.F; dev = L.device
        r = dict(out=torch.zeros((U, T, nb), dtype=torch.complex64, device=dev), mu=torch.zeros((U, T, F), dtype=torch.float32, device=dev) if want_mu else None,
                 itd=torch.zeros((U, T, F), dtype=torch.float64, device=dev) if want_itd else None)
        check(_core._lib.dsr_binmask_apply(self.h, _dev(L.contiguous()), _dev(R.contiguous()), _nf(nframes), U, T, _dev(r["out"]), nb, 0,
                                     _dev(r["mu"]) if want_mu else None, _dev(r["itd"]) if want_itd else None, _dev(state), cur_stream()))
        return r

    def read(self, state, u):
        out = np.zeros(self.F, np.float32); check(_core._lib.dsr_binmask_state_read(self.h, _dev(state), state.U, int(u), _ptr(out), out.size)); return out


class ThresholdEstimator(Handle):
    """KimITDThresholdEstimator ("kim"), IIDThresholdEstimator ("iid"), FDIIDThresholdEstimator ("fdiid") (binauralprocessing.cc:232-426, 525-683,
    702-928) over dsr_thest_*: run() adds to the caller's accumulators (newState), calcThreshold() finalises one utterance's on the host."""
    KINDS = {"kim": 0, "iid": 1, "fdiid": 2}

    _destroy = "dsr_thest_destroy"

    def __init__(self, kind, fftLen, minThreshold=0.0, maxThreshold=0.0, width=0.02, minFreq=-1.0, maxFreq=-1.0, sampleRate=-1, dEta=0.01, dPowerCoeff=0.0):
        L = load(); self.M = int(fftLen); self.F = self.M // 2 + 1; self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self._create(L.dsr_thest_create, self.kind, self.M, float(minThreshold), float(maxThreshold), float(width), float(minFreq), float(maxFreq), int(sampleRate),
                     float(dEta), float(dPowerCoeff))
        self.nCand = int(L.dsr_thest_n_cand(self.h)); self.nLoop = int(L.dsr_thest_n_loop(self.h)); self.accDoubles = int(L.dsr_thest_acc_doubles(self.h))

    def candidates(self):
        out = np.zeros(self.nLoop, np.float32); check(_core._lib.dsr_thest_candidates(self.h, _ptr(out), out.size)); return out

    def binRange(self):
        out = np.zeros(2, np.int32); check(_core._lib.dsr_thest_bin_range(self.h, _ptr(out))); return int(out[0]), int(out[1])

    def newState(self, U, device="cuda:0"):
        st = _state(_core._lib.dsr_thest_state_bytes(self.h, int(U)), device); st.U = int(U)
        check(_core._lib.dsr_thest_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def resetState(self, state):
        check(_core._lib.dsr_thest_reset_state(self.h, _dev(state), state.U, cur_stream()))

    def run(self, L, R, state, nframes=None):
        U, T, F = L.shape
        check(_core._lib.dsr_thest_run(self.h, _dev(L.contiguous()), _dev(R.contiguous()), _nf(nframes), U, T, _dev(state), cur_stream()))

    def read(self, state, u):
        out = np.zeros(self.accDoubles); check(_core._lib.dsr_thest_state_read(self.h, _dev(state), state.U, int(u), _ptr(out), out.size)); return out

    def calcThreshold(self, acc, inPlace=False):
        """-> dict(threshold, index, cost [nCand] or [F][nCand], thresholds [F] (FDIID)) from one utterance's accumulators (numpy, host side)"""
        a = acc if inPlace else _np(acc, np.float64).copy()
        th = C.c_double(0.0); ix = C.c_int32(0); cost = np.zeros((self.F, self.nCand) if self.kind == 2 else self.nCand); ths = np.zeros(self.F)
        check(_core._lib.dsr_thest_calc_threshold(self.h, _ptr(a), a.size, int(bool(inPlace)), C.byref(th), C.byref(ix), _ptr(cost), cost.size, _ptr(ths), ths.size))
        return dict(threshold=th.value, index=ix.value, cost=cost, thresholds=ths if self.kind == 2 else None)


def psdFileWrite(fn, est):
    e = _np(est, np.float64); load(); check(_core._lib.dsr_psd_file_write(str(fn).encode(), _ptr(e), e.size))


def psdFileRead(fn, n):
    out = np.zeros(int(n)); load(); check(_core._lib.dsr_psd_file_read(str(fn).encode(), _ptr(out), out.size)); return out
