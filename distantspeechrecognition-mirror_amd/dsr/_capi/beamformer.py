"""btk/beamformer: subband, spherical-array and maximum-kurtosis beamformers, SRP direction finding, the trackers."""
import ctypes as C

import numpy as np

from . import _core
from ._core import (DsrError, Handle, check, cur_stream, load, torch, E_DIMENSION, E_PARAMETER, _np, _ptr, _dev, _counts)


class Beamformer(Handle):
    """beamformerWeights + SubbandDS/GSC/MVDR weight design and apply (btk/beamformer/beamformer.h)."""

    _destroy = "dsr_bf_destroy"

    def __init__(self, fftLen, chanN, halfBandShift=False):
        L = load()
        self.M, self.C = fftLen, chanN
        self._create(L.dsr_bf_create, fftLen, chanN, int(halfBandShift))

    def calcArrayManifoldVectors(self, sampleRate, delays):
        d = _np(delays, np.float64)
        if d.size != self.C:
            raise DsrError(5, "Number of delays does not match number of channels (%d vs. %d)." % (d.size, self.C))
        check(_core._lib.dsr_bf_calc_array_manifold(self.h, sampleRate, _ptr(d)))

    def setDiffuseNoiseModel(self, micPositions, sampleRate, sspeed=343740.0):
        mp = _np(micPositions, np.float64)
        check(_core._lib.dsr_bf_set_diffuse_noise_model(self.h, _ptr(mp), sampleRate, sspeed))

    def divideAllNonDiagonalElements(self, myu):
        check(_core._lib.dsr_bf_divide_nondiagonal(self.h, myu))

    def setAllLevelsOfDiagonalLoading(self, w):
        check(_core._lib.dsr_bf_diagonal_loading(self.h, w))

    def setNoiseSpatialSpectralMatrix(self, fbinX, Rnn):
        R = _np(Rnn, np.complex128)
        check(_core._lib.dsr_bf_set_noise_matrix(self.h, fbinX, _ptr(R)))

    def calcMVDRWeights(self, sampleRate, dThreshold=1.0e-8):
        check(_core._lib.dsr_bf_calc_mvdr_weights(self.h, sampleRate, dThreshold))

    def calcGSCWeights(self, sampleRate, delays):
        d = _np(delays, np.float64)
        check(_core._lib.dsr_bf_calc_gsc_weights(self.h, sampleRate, _ptr(d)))

    def setActiveWeights_f(self, fbinX, packedWeight):
        w = _np(packedWeight, np.float64)
        if w.size != 2 * (self.C - 1):
            raise DsrError(5, "the size of an active weight vector must be %d but it is %d" % (2 * (self.C - 1), w.size))
        check(_core._lib.dsr_bf_set_active_weights(self.h, fbinX, _ptr(w)))

    def zeroActiveWeights(self):
        check(_core._lib.dsr_bf_zero_active_weights(self.h))

    def select(self, mode):
        check(_core._lib.dsr_bf_select(self.h, {"ds": 0, "mvdr": 1, "gsc": 2, "gsc_norm": 3, "mvdr_gsc": 4}.get(mode, mode)))

    def get(self, kind):
        F = self.M // 2 + 1
        shape = {0: (self.M, self.C), 1: (F, self.C), 2: (F, self.C, self.C), 3: (self.M, self.C, self.C - 1), 4: (_core._lib.dsr_bf_bins(self.h), self.C)}[kind]
        out = np.zeros(shape, np.complex128)
        check(_core._lib.dsr_bf_get(self.h, kind, _ptr(out), out.size * 2))
        return out

    # SubbandMVDRGSC (beamformer.h:394-425): the MVDR vector as quiescent weight, active weights from outside (select("mvdr_gsc"))
    def calcBlockingMatrix1(self, sampleRate, delaysT):
        self.calcGSCWeights(sampleRate, delaysT); return True

    def calcBlockingMatrix2(self):
        try:
            check(_core._lib.dsr_bf_calc_blocking_matrix2(self.h)); return True
        except DsrError:
            return False                                       # "You have to call calcMVDRWeights() first": the reference returns false

    def upgradeBlockingMatrix(self):
        check(_core._lib.dsr_bf_upgrade_blocking_matrix(self.h))

    def blockingMatrixOutput(self, X, outChanX=0):
        """X: cuda complex64 [U][C][T][F] -> B[:, outChanX]^H X, [U][T][F]"""
        U, Cn, T, F = X.shape
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        check(_core._lib.dsr_bf_blocking_matrix_output(self.h, _dev(torch.view_as_real(X.contiguous())), U, T, int(outChanX), _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)

    # SubbandGSCRLS (beamformer.h:213-262): recursive-least-squares adaptation of the active weights
    def rlsConfig(self, myu=0.9, sigma2=0.0):
        check(_core._lib.dsr_bf_rls_config(self.h, myu, sigma2))

    def initPrecisionMatrix(self, sigma2=0.01):
        check(_core._lib.dsr_bf_rls_init_precision(self.h, sigma2))

    def setPrecisionMatrix(self, fbinX, Pz):
        p = np.ascontiguousarray(Pz, np.complex128)
        if p.shape != (self.C - 1, self.C - 1):
            raise DsrError(5, "the precision matrix must be %d x %d" % (self.C - 1, self.C - 1))
        check(_core._lib.dsr_bf_rls_set_precision(self.h, fbinX, _ptr(p)))

    def setQuadraticConstraint(self, alpha, qctype=1):
        check(_core._lib.dsr_bf_rls_quadratic_constraint(self.h, alpha, qctype))

    def updateActiveWeightVecotrs(self, flag):
        check(_core._lib.dsr_bf_rls_adapt(self.h, int(bool(flag))))

    def gsc_rls(self, X, nframes=None):
        """X: cuda complex64 [U][C][T][F] -> (Y [U][T][F], final active weights [U][F][C-1] complex128); nframes: cuda int32 [U] valid frames"""
        U, Cn, T, F = X.shape
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        wa = torch.zeros((U, F, Cn - 1), dtype=torch.complex128, device=X.device)
        check(_core._lib.dsr_bf_gsc_rls(self.h, _dev(torch.view_as_real(X.contiguous())), _dev(nframes) if nframes is not None else None, U, T, _dev(Y), _dev(wa), cur_stream()))
        return torch.view_as_complex(Y), wa

    def rlsCarry(self, on=True):
        """keep adapting from call to call (block streaming; the reference's behaviour across reset())"""
        check(_core._lib.dsr_bf_rls_carry(self.h, int(bool(on))))

    def rlsResetState(self):
        check(_core._lib.dsr_bf_rls_reset_state(self.h))

    def rls_path(self):
        """bf_rls_path(chanN) of this object: the kernel gsc_rls launches and where its adaptation state lives"""
        return bf_rls_path(self.C)

    def bins(self):
        """bins per frame of apply(): fftLen/2+1, or fftLen with halfBandShift"""
        return _core._lib.dsr_bf_bins(self.h)

    def apply(self, X):
        """X: cuda complex64 [U][C][T][F] -> [U][T][F]"""
        U, Cn, T, F = X.shape
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        check(_core._lib.dsr_bf_apply(self.h, _dev(torch.view_as_real(X.contiguous())), U, T, _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)


def calcDelaysPolar2(azimuth, elevation, micPositions):
    load()
    mp = _np(micPositions, np.float64); d = np.zeros(mp.shape[0], np.float64)
    check(_core._lib.dsr_calc_delays_polar2(azimuth, elevation, _ptr(mp), mp.shape[0], _ptr(d)))
    return d


RLS_STATE_REGS, RLS_STATE_LDS, RLS_STATE_MEM = 0, 1, 2


def bf_rls_path(chanN):
    """-> ((CT, CAP, residence), (bytes of the 64 lanes' state, dynamic LDS of the launch)): the k_gsc_rls<CT, REG, CAP> dsr_bf_gsc_rls launches for
    chanN channels, REG = residence == RLS_STATE_REGS; follows DSR_RLS_NOREGS / DSR_RLS_MEMSTATE; needs no device"""
    L = load()
    out = (C.c_int * 3)(); lds = (C.c_int64 * 2)()
    check(L.dsr_bf_rls_path(int(chanN), out, lds))
    return tuple(out), tuple(lds)


class SubbandMMI(Handle):
    """SubbandMMI (beamformer.h:264-312, beamformer.cc:1753-2319) over dsr_mmi_*; the reference's method names."""

    _destroy = "dsr_mmi_destroy"

    def __init__(self, fftLen=512, chanN=2, halfBandShift=False, targetSourceX=0, nSource=2, pfType=0, alpha=0.9):
        L = load(); self.M, self.C, self.nSource, self.NC = fftLen, chanN, nSource, 1
        self._create(L.dsr_mmi_create, fftLen, chanN, int(bool(halfBandShift)), targetSourceX, nSource, pfType, alpha)

    def bins(self):
        return _core._lib.dsr_mmi_bins(self.h)

    def outBins(self):
        """bins per output frame: bins(), or fftLen with the APAB post-filter (whose frames are not conjugate-symmetric)"""
        return _core._lib.dsr_mmi_out_bins(self.h)

    def useBinaryMask(self, avgFactor=-1.0, fwidth=1, type=0):
        check(_core._lib.dsr_mmi_use_binary_mask(self.h, avgFactor, fwidth, type))

    def calcWeights(self, sampleRate, delays):
        d = np.ascontiguousarray(delays, np.float64)
        if d.shape != (self.nSource, self.C):
            raise DsrError(5, "delays must be [%d][%d]" % (self.nSource, self.C))
        check(_core._lib.dsr_mmi_calc_weights(self.h, sampleRate, _ptr(d))); self.NC = 1

    def calcWeightsN(self, sampleRate, delays, NC=2):
        d = np.ascontiguousarray(delays, np.float64)
        if d.shape != (self.nSource, self.C):
            raise DsrError(5, "delays must be [%d][%d]" % (self.nSource, self.C))
        check(_core._lib.dsr_mmi_calc_weights_n(self.h, sampleRate, _ptr(d), NC)); self.NC = NC

    def setActiveWeights_f(self, fbinX, packedWeights, option=0):
        w = np.ascontiguousarray(packedWeights, np.float64)
        if w.ndim != 2:
            raise DsrError(5, "packedWeights must be a matrix")
        check(_core._lib.dsr_mmi_set_active_weights_f(self.h, fbinX, _ptr(w), w.shape[0], w.shape[1], option))

    def setHiActiveWeights_f(self, fbinX, pkdWa, pkdwb, option=0):
        a = np.ascontiguousarray(pkdWa, np.float64).ravel(); b = np.ascontiguousarray(pkdwb, np.float64).ravel()
        check(_core._lib.dsr_mmi_set_hi_active_weights_f(self.h, fbinX, _ptr(a), a.size, _ptr(b), b.size, option))

    def get(self, srcX, kind):
        """kind: 'wq' [M][C], 'wl' [M][C], 'B' [M][C][C-NC], 'ta' [M][C], 'wa' [M][C-NC] (complex128)"""
        k = {"wq": 0, "wl": 1, "B": 2, "ta": 3, "wa": 4}[kind]; bs = self.C - self.NC
        shape = {0: (self.M, self.C), 1: (self.M, self.C), 2: (self.M, self.C, bs), 3: (self.M, self.C), 4: (self.M, bs)}[k]
        out = np.zeros(shape, np.complex128)
        check(_core._lib.dsr_mmi_get(self.h, srcX, k, _ptr(out), 2 * out.size))
        return out

    def apply(self, X, nframes=None):
        """X: cuda complex64 [U][C][T][bins] -> [U][T][outBins]"""
        U, Cn, T, F = X.shape
        if Cn != self.C or F != self.bins():
            raise DsrError(5, "snapshots must be [U][%d][T][%d]" % (self.C, self.bins()))
        nframes = _counts(nframes, U, T, X.device)
        out = torch.zeros((U, T, self.outBins()), dtype=torch.complex64, device=X.device)
        check(_core._lib.dsr_mmi_apply(self.h, _dev(X.contiguous()), _dev(nframes), U, T, _dev(out), cur_stream()))
        return out


class DoaSRP(Handle):
    """DOAEstimatorSRPDSBLA (btk/beamformer/beamformer.h:462-560, beamformer.cc:2920-3283) over a batch: settings and steering table on the
    host, the response powers of X [U][C][T][M/2+1] on the fp64 MFMA (dsr_doa_srp).  The accumulators belong to the caller."""

    _destroy = "dsr_doa_destroy"

    def __init__(self, nBest, sampleRate, fftLen, chanN):
        L = load(); self.nBest, self.M, self.C = nBest, fftLen, chanN
        self._create(L.dsr_doa_create, int(nBest), int(sampleRate), int(fftLen), int(chanN))

    def setArrayGeometry(self, positions):
        p = _np(positions, np.float64).ravel()
        check(_core._lib.dsr_doa_set_array_geometry(self.h, _ptr(p), p.size))

    def setSearchParam(self, minTheta=-np.pi / 2, maxTheta=np.pi / 2, widthTheta=0.1):
        check(_core._lib.dsr_doa_set_search_param(self.h, float(minTheta), float(maxTheta), float(widthTheta)))

    def setFrequencyRange(self, fbinMin, fbinMax):
        check(_core._lib.dsr_doa_set_frequency_range(self.h, int(fbinMin), int(fbinMax)))

    def frequencyRange(self):
        a, b = C.c_int(), C.c_int(); check(_core._lib.dsr_doa_frequency_range(self.h, C.byref(a), C.byref(b))); return a.value, b.value

    def setEnergyThreshold(self, threshold):
        check(_core._lib.dsr_doa_set_energy_threshold(self.h, float(threshold)))

    def thetaN(self):
        n = C.c_int(); check(_core._lib.dsr_doa_theta_n(self.h, C.byref(n))); return n.value

    def thetas(self):
        n = self.thetaN(); out = np.zeros(n, np.float64); check(_core._lib.dsr_doa_thetas(self.h, _ptr(out), n)); return out

    def lookDelays(self, theta):
        out = np.zeros(self.C, np.float64); check(_core._lib.dsr_doa_look_delays(self.h, float(theta), _ptr(out))); return out

    def steering(self, thetaX):
        out = np.zeros((self.M // 2 + 1, self.C), np.complex128)
        check(_core._lib.dsr_doa_steering(self.h, int(thetaX), _ptr(out), out.size * 2)); return out

    def cell(self):
        """-> ((TG, BC, KS), dynamic LDS bytes): the k_doa_srp<TG> srp() launches and its staging (dsr_doa_srp_cell); needs no device"""
        c = (C.c_int * 3)(); b = C.c_int64(); check(_core._lib.dsr_doa_srp_cell(self.h, c, C.byref(b))); return tuple(c), b.value

    def srp(self, X, nframes=None, acc=None, want_rp=False, want_y=False):
        """X cuda complex64 [U][C][T][M/2+1] -> dict(energy [U][T] f32, nbest_rp [U][T][nBest] f64, nbest_idx [U][T][nBest] i32, gated [U][T] i32,
        acc [U][nTheta] f64 (the one passed in, added to), rp [U][T][nTheta] f64 and y [U][T][M/2+1] complex64 on request).  Frames past
        nframes[u] keep the zeros they start with."""
        U, Cn, T, F = X.shape
        dev = X.device; nT = self.thetaN()
        nframes = _counts(nframes, U, T, dev)
        if acc is None:
            acc = torch.zeros((U, nT), dtype=torch.float64, device=dev)
        elif tuple(acc.shape) != (U, nT) or acc.dtype != torch.float64 or not acc.is_contiguous():
            raise ValueError("acc: contiguous float64 [U][nTheta] expected")
        r = dict(energy=torch.zeros((U, T), dtype=torch.float32, device=dev), nbest_rp=torch.zeros((U, T, self.nBest), dtype=torch.float64, device=dev),
                 nbest_idx=torch.zeros((U, T, self.nBest), dtype=torch.int32, device=dev), gated=torch.zeros((U, T), dtype=torch.int32, device=dev), acc=acc)
        r["rp"] = torch.zeros((U, T, nT), dtype=torch.float64, device=dev) if want_rp else None
        r["y"] = torch.zeros((U, T, F), dtype=torch.complex64, device=dev) if want_y else None
        Xc = torch.view_as_real(X.contiguous())
        check(_core._lib.dsr_doa_srp(self.h, _dev(Xc), _dev(nframes), U, T, _dev(r["energy"]), _dev(r["rp"]) if want_rp else None, _dev(r["nbest_rp"]),
                               _dev(r["nbest_idx"]), _dev(acc), _dev(r["y"]) if want_y else None, _dev(r["gated"]), cur_stream()))
        return r

    def finalNBest(self, acc):
        """getFinalNBestHypotheses for each row of acc [U][nTheta] (host or device) -> (rp [U][nBest], theta index [U][nBest], -1 = empty)"""
        a = np.ascontiguousarray(acc.detach().cpu().numpy() if hasattr(acc, "detach") else acc, np.float64)
        a = a.reshape(-1, a.shape[-1]); U = a.shape[0]
        R = np.zeros((U, self.nBest), np.float64); I = np.zeros((U, self.nBest), np.int32)
        check(_core._lib.dsr_doa_final_nbest(self.h, _ptr(a), U, _ptr(R), _ptr(I)))
        return R, I


class _Sph(Handle):
    """the dsr_sph handle (modalBeamformer.{h,cc}): kind "EB" (EigenBeamformer weights), "DS" (SphericalDSBeamformer weights) or one of the
    further beamformers "HWNC", "GSC", "HWNCGSC", "SPATIALDS", "MOEN"; settings, geometry and tables on the host"""
    KINDS = {"EB": 0, "DS": 1, "HWNC": 2, "GSC": 3, "HWNCGSC": 4, "SPATIALDS": 5, "MOEN": 6}

    _destroy = "dsr_sph_destroy"

    def __init__(self, kind, nBest, sampleRate, fftLen, chanN, maxOrder, normalizeWeight=False, halfBandShift=False, NC=1):
        L = load(); self.nBest, self.M, self.C = nBest, fftLen, chanN
        k = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self._create(L.dsr_sph_create, k, int(nBest), int(sampleRate), int(fftLen), int(bool(halfBandShift)), int(NC), int(maxOrder), int(bool(normalizeWeight)),
                     int(chanN))
        self.dim = L.dsr_sph_dim(self.h); self.NC = int(NC)

    def setWNG(self, ratio):
        check(_core._lib.dsr_sph_set_wng(self.h, float(ratio)))

    def setActiveWeights_f(self, fbinX, packedWeight):
        p = _np(packedWeight, np.float64).ravel()
        check(_core._lib.dsr_sph_set_active_weights_f(self.h, int(fbinX), _ptr(p), p.size))

    def setLevelOfDiagonalLoading(self, fbinX, diagonalWeight):
        check(_core._lib.dsr_sph_set_diagonal_loading(self.h, int(fbinX), float(diagonalWeight)))

    def fixTerms(self, flag):
        check(_core._lib.dsr_sph_fix_terms(self.h, int(bool(flag))))

    def wl(self):
        return self._table(_core._lib.dsr_sph_wl, (self.M // 2 + 1, self.dim))

    def blockingMatrix(self, fbinX):
        return self._table(_core._lib.dsr_sph_blocking_matrix, (self.dim, self.dim - self.NC), int(fbinX))

    def sensorWeights(self):
        return self._table(_core._lib.dsr_sph_sensor_weights, (self.M // 2 + 1, self.C))

    def setBeam(self, b, theta, phi):
        check(_core._lib.dsr_sph_set_beam(self.h, int(b), float(theta), float(phi)))

    def setBeamsFromNBest(self, doa, nbest_idx):
        """beams 0..n-1 = the directions of doa's (a SphDoaSRP) units nbest_idx [n], e.g. one row of finalNBest's indices"""
        idx = np.ascontiguousarray(nbest_idx, np.int32).ravel()
        check(_core._lib.dsr_sph_set_beams_nbest(self.h, doa.h, _ptr(idx), idx.size)); return idx.size

    def beamWeights(self, NB=1):
        """V [NB][M/2+1][C]: the sensor-domain vectors of dsr_sph_beams, y = v^H x"""
        n = max(1, min(int(NB), 16)); out = np.zeros((n, self.M // 2 + 1, self.C), np.complex128)
        check(_core._lib.dsr_sph_beam_weights(self.h, int(NB), _ptr(out), out.size * 2)); return out

    def beams(self, X, nframes=None, NB=1):
        """X cuda complex64 [U][C][T][M/2+1] -> y [U][NB][T][M/2+1] complex64, every beam in one pass over X (dsr_sph_beams); rows past
        nframes[u] are zero"""
        U, Cn, T, F = X.shape
        dev = X.device
        nframes = _counts(nframes, U, T, dev)
        y = torch.empty((U, max(int(NB), 0), T, F), dtype=torch.complex64, device=dev)
        Xc = torch.view_as_real(X.contiguous())
        check(_core._lib.dsr_sph_beams(self.h, _dev(Xc), _dev(nframes), U, T, int(NB), _dev(y), cur_stream()))
        return y

    def getBeamPattern(self, fbinX, theta=0.0, phi=0.0, minTheta=-np.pi, maxTheta=np.pi, minPhi=-np.pi, maxPhi=np.pi, widthTheta=0.1, widthPhi=0.1):
        a, b = C.c_int(), C.c_int()
        g = (float(minTheta), float(maxTheta), float(minPhi), float(maxPhi), float(widthTheta), float(widthPhi))
        check(_core._lib.dsr_sph_beam_pattern_n(*g, C.byref(a), C.byref(b)))
        out = np.zeros((max(a.value, 0), max(b.value, 0)), np.float64)
        check(_core._lib.dsr_sph_beam_pattern(self.h, int(fbinX), float(theta), float(phi), *g, _ptr(out), out.size)); return out

    def _table(self, fn, shape, *args):
        out = np.zeros(shape, np.complex128); check(fn(self.h, *args, _ptr(out), out.size * 2)); return out

    def setArrayGeometry(self, a, theta_s, phi_s):
        t = _np(theta_s, np.float64).ravel(); p = _np(phi_s, np.float64).ravel()
        if t.size != p.size:
            raise DsrError(E_DIMENSION, "theta_s and phi_s differ in length")
        check(_core._lib.dsr_sph_set_array_geometry(self.h, float(a), _ptr(t), _ptr(p), t.size))

    def setEigenMikeGeometry(self):
        check(_core._lib.dsr_sph_set_eigenmike_geometry(self.h))

    def getArrayGeometry(self, type):
        out = np.zeros(self.C, np.float64); check(_core._lib.dsr_sph_array_geometry(self.h, int(type), _ptr(out), self.C)); return out

    def setLookDirection(self, theta, phi):
        check(_core._lib.dsr_sph_set_look_direction(self.h, float(theta), float(phi)))

    def setSigma2(self, sigma2):
        check(_core._lib.dsr_sph_set_sigma2(self.h, float(sigma2)))

    def setWeightGain(self, wgain):
        check(_core._lib.dsr_sph_set_weight_gain(self.h, float(wgain)))

    def modeAmplitudes(self):
        return self._table(_core._lib.dsr_sph_mode_amplitudes, (self.M // 2 + 1, _core._lib.dsr_sph_max_order(self.h)))

    def harmonics(self):
        return self._table(_core._lib.dsr_sph_harmonics, (self.dim, self.C))

    def lookWeights(self):
        return self._table(_core._lib.dsr_sph_look_weights, (self.M // 2 + 1, self.dim))

    def calcWNG(self):
        out = np.zeros(self.M // 2 + 1, np.float64); check(_core._lib.dsr_sph_calc_wng(self.h, _ptr(out), out.size)); return out

    def apply(self, X, nframes=None, want_F=False):
        """X cuda complex64 [U][C][T][M/2+1] -> (y [U][T][M/2+1] complex64, F [U][T][M/2+1][dim] complex64 or None); frames past nframes[u] stay 0"""
        U, Cn, T, F = X.shape
        dev = X.device
        nframes = _counts(nframes, U, T, dev)
        y = torch.zeros((U, T, F), dtype=torch.complex64, device=dev)
        Fo = torch.zeros((U, T, F, self.dim), dtype=torch.complex64, device=dev) if want_F else None
        Xc = torch.view_as_real(X.contiguous())
        check(_core._lib.dsr_sph_apply(self.h, _dev(Xc), _dev(nframes), U, T, _dev(y), _dev(Fo) if want_F else None, cur_stream()))
        return y, Fo


class SphBeamformer(_Sph):
    """EigenBeamformer (kind "EB") / SphericalDSBeamformer (kind "DS") over a batch (dsr_sph_apply); the further kinds ("HWNC", "GSC",
    "HWNCGSC", "SPATIALDS", "MOEN") and several beams at once through beams() (dsr_sph_beams).  ratio: the HWNC kinds' setWNG."""

    def __init__(self, kind, sampleRate, fftLen, chanN, maxOrder, normalizeWeight=False, halfBandShift=False, NC=1, ratio=None):
        _Sph.__init__(self, kind, 1, sampleRate, fftLen, chanN, maxOrder, normalizeWeight, halfBandShift, NC)
        if ratio is not None:
            self.setWNG(ratio)


class SphDoaSRP(_Sph):
    """DOAEstimatorSRPEB (kind "EB") / DOAEstimatorSRPSphDSB (kind "DS") over a batch: the (theta, phi) grid and steering table on the host, the
    response powers of X [U][C][T][M/2+1] on the fp64 MFMA (dsr_sph_srp).  The accumulators belong to the caller."""

    def __init__(self, kind, *args, **kw):
        if (self.KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)) not in (0, 1):
            raise DsrError(1, "SphDoaSRP searches with the EB or DS weights; kind %r has no steering table" % (kind,))
        _Sph.__init__(self, kind, *args, **kw)

    def setSearchParam(self, minTheta=0.0, maxTheta=np.pi, minPhi=-np.pi, maxPhi=np.pi, widthTheta=0.1, widthPhi=0.1):
        check(_core._lib.dsr_sph_set_search_param(self.h, float(minTheta), float(maxTheta), float(minPhi), float(maxPhi), float(widthTheta), float(widthPhi)))

    def setFrequencyRange(self, fbinMin, fbinMax):
        check(_core._lib.dsr_sph_set_frequency_range(self.h, int(fbinMin), int(fbinMax)))

    def frequencyRange(self):
        a, b = C.c_int(), C.c_int(); check(_core._lib.dsr_sph_frequency_range(self.h, C.byref(a), C.byref(b))); return a.value, b.value

    def setEnergyThreshold(self, threshold):
        check(_core._lib.dsr_sph_set_energy_threshold(self.h, float(threshold)))

    def gridN(self):
        a, b = C.c_int(), C.c_int(); check(_core._lib.dsr_sph_grid_n(self.h, C.byref(a), C.byref(b))); return a.value, b.value

    def grid(self):
        """(theta [units], phi [units]), unit = iTheta nPhi + iPhi"""
        nT, nP = self.gridN(); th = np.zeros(nT * nP); ph = np.zeros(nT * nP)
        check(_core._lib.dsr_sph_grid(self.h, _ptr(th), _ptr(ph), nT * nP)); return th, ph

    def units(self):
        nT, nP = self.gridN(); return nT * nP

    def steering(self, unit):
        return self._table(_core._lib.dsr_sph_steering, (self.M // 2 + 1, self.dim), int(unit))

    def path(self):
        p = _core._lib.dsr_sph_srp_path(self.h)
        if p < 0:
            raise DsrError(1, (_core._lib.dsr_last_error() or b"").decode(errors="replace"))
        return ("fused", "folded")[p]

    def cell(self):
        """-> ((path 0 fused / 1 folded, TG, DT or 0, BC, KS), dynamic LDS bytes) of the kernel srp() launches (dsr_sph_srp_cell); needs no device"""
        c = (C.c_int * 5)(); b = C.c_int64(); check(_core._lib.dsr_sph_srp_cell(self.h, c, C.byref(b))); return tuple(c), b.value

    def srp(self, X, nframes=None, acc=None, want_rp=False, want_y=False):
        """as DoaSRP.srp, units in place of theta: dict(energy, nbest_rp, nbest_idx, gated, acc [U][units], rp, y)"""
        U, Cn, T, F = X.shape
        dev = X.device; nU = self.units()
        nframes = _counts(nframes, U, T, dev)
        if acc is None:
            acc = torch.zeros((U, nU), dtype=torch.float64, device=dev)
        elif tuple(acc.shape) != (U, nU) or acc.dtype != torch.float64 or not acc.is_contiguous():
            raise ValueError("acc: contiguous float64 [U][units] expected")
        r = dict(energy=torch.zeros((U, T), dtype=torch.float32, device=dev), nbest_rp=torch.zeros((U, T, self.nBest), dtype=torch.float64, device=dev),
                 nbest_idx=torch.zeros((U, T, self.nBest), dtype=torch.int32, device=dev), gated=torch.zeros((U, T), dtype=torch.int32, device=dev), acc=acc)
        r["rp"] = torch.zeros((U, T, nU), dtype=torch.float64, device=dev) if want_rp else None
        r["y"] = torch.zeros((U, T, F), dtype=torch.complex64, device=dev) if want_y else None
        Xc = torch.view_as_real(X.contiguous())
        check(_core._lib.dsr_sph_srp(self.h, _dev(Xc), _dev(nframes), U, T, _dev(r["energy"]), _dev(r["rp"]) if want_rp else None, _dev(r["nbest_rp"]),
                               _dev(r["nbest_idx"]), _dev(acc), _dev(r["y"]) if want_y else None, _dev(r["gated"]), cur_stream()))
        return r

    def finalNBest(self, acc):
        """getFinalNBestHypotheses for each row of acc [U][units] -> (rp [U][nBest], unit index [U][nBest], -1 = empty)"""
        a = np.ascontiguousarray(acc.detach().cpu().numpy() if hasattr(acc, "detach") else acc, np.float64)
        a = a.reshape(-1, a.shape[-1]); U = a.shape[0]
        R = np.zeros((U, self.nBest), np.float64); I = np.zeros((U, self.nBest), np.int32)
        check(_core._lib.dsr_sph_final_nbest(self.h, _ptr(a), U, _ptr(R), _ptr(I)))
        return R, I


def sph_beams_cell(NB, chanN, bins):
    """-> ((0 valu, rows, CC) or (1 mfma, BCT, KS), dynamic LDS bytes) of one beams() call (dsr_sph_beams_cell); needs no device"""
    c = (C.c_int * 3)(); b = C.c_int64(); check(load().dsr_sph_beams_cell(int(NB), int(chanN), int(bins), c, C.byref(b))); return tuple(c), b.value


class SphTracker(Handle):
    """The spherical-array speaker trackers of btk/beamformer/tracker.{h,cc} (include/dsr.h section 2c''): kind "modal" (ModalDecomposition +
    ModalSphericalArrayTracker) or "spatial" (SpatialDecomposition + SpatialSphericalArrayTracker) over a batch.  The handle holds the
    decomposition's tables and the tracker's parameters; the filter's state (position, K) is a device buffer of the caller (newState) that
    run() continues from and leaves behind, so an utterance may come in blocks."""
    KINDS = {"modal": 0, "spatial": 1}
    CLAMP, ERROR = 1 << 8, 1 << 9

    _destroy = "dsr_trk_destroy"

    def __init__(self, kind, orderN, fftLen, a=42.0, sampleRate=16000.0, useSubbandsN=0, sigma2_u=10.0, sigma2_v=10.0, sigma2_init=10.0, maxLocalN=1,
                 chanN=32):
        L = load(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self._create(L.dsr_trk_create, self.kind, int(orderN), int(fftLen), float(a), float(sampleRate), int(useSubbandsN), float(sigma2_u), float(sigma2_v),
                     float(sigma2_init), int(maxLocalN), int(chanN))
        self.M, self.F, self.orderN = int(fftLen), int(fftLen) // 2 + 1, int(orderN)
        self.modesN = L.dsr_trk_modes_n(self.h); self.L = L.dsr_trk_subband_length(self.h); self.useSubbandsN = L.dsr_trk_use_subbands_n(self.h)

    @staticmethod
    def maxRows(kind, orderN, useSubbandsN):
        return int(load().dsr_trk_max_rows(SphTracker.KINDS[kind] if isinstance(kind, str) else int(kind), int(orderN), int(useSubbandsN)))

    def setV(self, Vk, subbandX):
        v = _np(Vk, np.complex128)
        if v.shape != (self.L, self.L):
            raise DsrError(E_PARAMETER, "Vk: [%d][%d] expected" % (self.L, self.L))
        check(_core._lib.dsr_trk_set_v(self.h, _ptr(v), v.size * 2, int(subbandX)))

    def getV(self, subbandX):
        out = np.zeros((2 * self.L, 2 * self.L), np.float64); check(_core._lib.dsr_trk_get_v(self.h, int(subbandX), _ptr(out), out.size)); return out

    def setInitialPosition(self, theta, phi):
        check(_core._lib.dsr_trk_set_initial_position(self.h, float(theta), float(phi)))

    def nextSpeaker(self):
        check(_core._lib.dsr_trk_next_speaker(self.h))

    def bn(self):
        out = np.zeros((self.F, self.orderN + 1), np.complex128); check(_core._lib.dsr_trk_bn(self.h, _ptr(out), out.size * 2)); return out

    def sensorHarmonics(self):
        out = np.zeros((self.modesN, 32), np.complex128); check(_core._lib.dsr_trk_sensor_harmonics(self.h, _ptr(out), out.size * 2)); return out

    @staticmethod
    def geometry():
        t, p = np.zeros(32), np.zeros(32); check(load().dsr_trk_geometry(_ptr(t), _ptr(p), 32)); return t, p

    @staticmethod
    def _static(fn, *args):
        out = np.zeros(2, np.float64); load(); check(fn(*args, _ptr(out))); return complex(out[0], out[1])

    @staticmethod
    def harmonic(order, degree, theta, phi):
        return SphTracker._static(load().dsr_trk_harmonic, int(order), int(degree), float(theta), float(phi))

    @staticmethod
    def harmonicDerivPolarAngle(order, degree, theta, phi):
        return SphTracker._static(load().dsr_trk_harmonic_deriv_polar, int(order), int(degree), float(theta), float(phi))

    @staticmethod
    def harmonicDerivAzimuth(order, degree, theta, phi):
        return SphTracker._static(load().dsr_trk_harmonic_deriv_azimuth, int(order), int(degree), float(theta), float(phi))

    @staticmethod
    def modalCoefficient(order, ka):
        return SphTracker._static(load().dsr_trk_modal_coefficient, int(order), float(ka))

    def stateDoubles(self):
        return int(_core._lib.dsr_trk_state_doubles(self.h))

    def newState(self, U, device="cuda:0"):
        st = torch.zeros((int(U), self.stateDoubles()), dtype=torch.float64, device=device)
        self.initState(st); return st

    def initState(self, state, positionOnly=False):
        """positionOnly False: as nextSpeaker leaves the tracker (the handle's initial position, the initial K); True: setInitialPosition"""
        check(_core._lib.dsr_trk_init_state(self.h, _dev(state), int(state.shape[0]), int(bool(positionOnly)), cur_stream()))

    def run(self, X, nframes=None, state=None):
        """X cuda complex64 [U][32][T][M/2+1] -> (pos [U][T][2] float32, pos64 [U][T][2] float64, info [U][T] int32); rows past nframes[u] are
        zero.  state None: a fresh one, discarded."""
        U, Cn, T, F = X.shape
        if Cn != 32 or F != self.F or X.dtype != torch.complex64:
            raise ValueError("X: complex64 [U][32][T][%d] expected" % self.F)
        dev = X.device
        nframes = _counts(nframes, U, T, dev)
        if state is None:
            state = self.newState(U, dev)
        pos = torch.zeros((U, T, 2), dtype=torch.float32, device=dev); pos64 = torch.zeros((U, T, 2), dtype=torch.float64, device=dev)
        info = torch.zeros((U, T), dtype=torch.int32, device=dev)
        check(_core._lib.dsr_trk_run(self.h, _dev(torch.view_as_real(X.contiguous())), _dev(nframes), U, T, _dev(state), _dev(pos), _dev(pos64), _dev(info), cur_stream()))
        return pos, pos64, info


class PlaneWaveSim:
    """PlaneWaveSimulator (tracker.cc:1444-1488) for all 32 channels at once: coefficients on the host (over a SphTracker's decomposition), the
    product with the source spectrum on the device"""

    def __init__(self, tracker, theta, phi):
        self.trk, self.F, self.M = tracker, tracker.F, tracker.M
        self.coef = np.zeros((32, self.F), np.complex128)
        check(_core._lib.dsr_pws_coefficients(tracker.h, float(theta), float(phi), _ptr(self.coef), self.coef.size * 2))
        self._dev = None

    def apply(self, src, nframes=None, full=False):
        """src cuda complex64 [U][T][M/2+1] -> [U][32][T][M/2+1] complex64, or rows of M bins with the conjugate mirror (full)"""
        U, T, F = src.shape
        if F != self.F or src.dtype != torch.complex64:
            raise ValueError("src: complex64 [U][T][%d] expected" % self.F)
        dev = src.device
        if self._dev is None or self._dev.device != dev:
            self._dev = torch.view_as_real(torch.from_numpy(self.coef)).contiguous().to(dev)
        nframes = _counts(nframes, U, T, dev)
        out = torch.zeros((U, 32, T, self.M if full else F), dtype=torch.complex64, device=dev)
        check(_core._lib.dsr_pws_apply(_dev(self._dev), 32, _dev(torch.view_as_real(src.contiguous())), _dev(nframes), U, T, self.M, int(bool(full)), _dev(out), cur_stream()))
        return out


MK_PR, MK_NRM = 0, 1
MK_EXIT_MAX_ITERATIONS, MK_EXIT_GRADIENT, MK_EXIT_DIFFERENCE, MK_EXIT_NO_PROGRESS, MK_EXIT_EVAL_CAP, MK_EXIT_SKIPPED = 0, 1, 2, 3, 4, 5
MK_FRAMES_LDS, MK_FRAMES_STREAMED = 0, 1
MK_EVAL_CAP = 2048


def mk_path(chanN, Tsel):
    """-> ((CT, residence), (frames that fit the LDS residence, dynamic LDS of the launch)): the k_mk_minimize<CT> dsr_mk_estimate launches for chanN
    channels and Tsel selected frames, and where a problem's frames live; needs no device"""
    L = load()
    out = (C.c_int * 2)(); lds = (C.c_int64 * 2)()
    check(L.dsr_mk_path(int(chanN), int(Tsel), out, lds))
    return tuple(out), tuple(lds)


class MkBeamformer(Handle):
    """Maximum empirical kurtosis beamforming (btk/lib/mkBeamforming.py: MEKSubbandBeamformer_pr / _nrm) for a batch: every (utterance, bin) is one
    problem, all of them minimised in one launch.  kind: MK_PR (conjugate gradient) or MK_NRM (steepest descent, |wa| clipped to |gamma|); the
    defaults of alpha and DIFFSTOPTOLERANCE are the reference's for that kind."""

    _destroy = "dsr_mk_destroy"

    def __init__(self, fftLen, chanN, kind=MK_PR, alpha=None, beta=3.0, gamma=-1.0, NC=1, nSource=1, halfBandShift=False):
        L = load()
        self.M, self.C, self.F, self.kind = fftLen, chanN, fftLen // 2 + 1, kind
        self._create(L.dsr_mk_create, fftLen, chanN, int(NC), int(nSource), int(bool(halfBandShift)))
        self.config(kind, (1.0e-2 if kind == MK_PR else 0.1) if alpha is None else alpha, beta, gamma)
        self.minimizer()

    def config(self, kind, alpha, beta=3.0, gamma=-1.0):
        check(_core._lib.dsr_mk_config(self.h, int(kind), alpha, beta, gamma)); self.kind, self.alpha = kind, alpha

    def minimizer(self, MAXITNS=40, TOLERANCE=1.0e-3, STOPTOLERANCE=1.0e-2, DIFFSTOPTOLERANCE=None, STEPSIZE=0.01):
        if DIFFSTOPTOLERANCE is None:
            DIFFSTOPTOLERANCE = 1.0e-5 if self.kind == MK_PR else 1.0e-10
        check(_core._lib.dsr_mk_minimizer(self.h, int(MAXITNS), TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE))

    def setFixedWeightsFromBeamformer(self, bf):
        """the quiescent vectors and blocking matrices of a Beamformer after calcGSCWeights"""
        check(_core._lib.dsr_mk_set_fixed_weights_from_bf(self.h, bf.h))

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
        check(_core._lib.dsr_mk_set_fixed_weights(self.h, _ptr(w), _ptr(b) if b is not None else None))

    def getFixedWeights(self):
        wq = np.zeros((self.F, self.C), np.complex128); B = np.zeros((self.F, self.C, self.C - 1), np.complex128)
        check(_core._lib.dsr_mk_get_fixed_weights(self.h, _ptr(wq), _ptr(B)))
        return wq, B

    def forceStreamed(self, on=True):
        check(_core._lib.dsr_mk_force_streamed(self.h, int(bool(on))))

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

    def eval(self, X, wa, nframes=None, sFrame=0, eFrame=None, R=1, stats=None, fbinX=-1):
        """X: cuda complex64 [U][C][T][F]; wa [U][F][C-1] complex128; nframes: cuda int32 [U]; stats: cuda fp64 [3][U][F]
        -> (cost [U][F], packed gradient [U][F][2 (C-1)]) fp64"""
        a = self._args(X, nframes, sFrame, eFrame, R, fbinX); w = self._wa(wa, X); U = X.shape[0]
        cost = torch.zeros((U, self.F), dtype=torch.float64, device=X.device)
        grad = torch.zeros((U, self.F, 2 * (self.C - 1)), dtype=torch.float64, device=X.device)
        check(_core._lib.dsr_mk_eval(self.h, *a, _dev(torch.view_as_real(w)), _dev(stats) if stats is not None else None, _dev(cost), _dev(grad), cur_stream()))
        return cost, grad

    def estimate(self, X, wa=None, nframes=None, sFrame=0, eFrame=None, R=1, stats=None, fbinX=-1):
        """-> (wa [U][F][C-1] complex128, info [U][F][4] int32: iterations, evaluations, failed trials, exit reason, final cost [U][F]).  wa: the
        starting point (None: zero).  stats (cuda fp64 [3][U][F]: prevAvgY2, prevAvgY4, prevFrameN) is read, and for MK_NRM updated in place."""
        a = self._args(X, nframes, sFrame, eFrame, R, fbinX); w = self._wa(wa, X); U = X.shape[0]
        info = torch.zeros((U, self.F, 4), dtype=torch.int32, device=X.device)
        cost = torch.zeros((U, self.F), dtype=torch.float64, device=X.device)
        check(_core._lib.dsr_mk_estimate(self.h, *a, _dev(torch.view_as_real(w)), _dev(stats) if stats is not None else None, _dev(info), _dev(cost), cur_stream()))
        return w, info, cost

    def apply(self, X, wa):
        """Y [U][T][F] = (wq - B wa[u][f])^H X, per-utterance active weights"""
        U, Cn, T, F = X.shape
        w = self._wa(wa, X)
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        check(_core._lib.dsr_mk_apply(self.h, _dev(torch.view_as_real(X.contiguous())), U, T, _dev(torch.view_as_real(w)), _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)
