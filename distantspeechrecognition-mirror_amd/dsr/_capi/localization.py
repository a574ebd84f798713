"""btk/localization: GCC time-delay estimation, search grids, multichannel cross-correlation."""
import ctypes as C

import numpy as np

from . import _core
from ._core import (DsrError, Handle, check, cur_stream, load, torch, E_DIMENSION, _np, _ptr, _dev)


class Gcc(Handle):
    """The GCC family of btk/localization (include/dsr.h section 2e): kind "raw", "gnnsub", "phat", "gnnsubphat", "mlrraw" or "mlrgnnsub".
    The handle holds the pair list [P][2] and the parameters (defaults of localization.h:123); what the estimator carries from frame to
    frame is a device buffer of the caller (newState) that run() continues from and leaves behind."""
    KINDS = {"raw": 0, "gnnsub": 1, "phat": 2, "gnnsubphat": 3, "mlrraw": 4, "mlrgnnsub": 5}
    HUGE = float(np.finfo(np.float32).max)                       # <math.h> HUGE, findMaximum's default window (localization.h:126)
    NOISE_POWER, NOISE_CROSS, CROSS, CORRELATION = 0, 1, 2, 3

    _destroy = "dsr_gcc_destroy"

    def __init__(self, kind, pairs, sampleRate=44100.0, fftLen=2048, nChan=16, alpha=0.95, beta=0.5, q=0.3, interpolate=True, noisereduction=True):
        L = load(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self.pairs = _np(pairs, np.int32).reshape(-1, 2); self.P = self.pairs.shape[0]; self.C = int(nChan); self.N = int(fftLen); self.F = self.N // 2 + 1
        self.sampleRate = float(sampleRate)
        self._create(L.dsr_gcc_create, self.kind, float(sampleRate), int(fftLen), int(nChan), _ptr(self.pairs), self.P, float(alpha), float(beta), float(q),
                     int(bool(interpolate)), int(bool(noisereduction)))

    def setAlpha(self, alpha):
        check(_core._lib.dsr_gcc_set_alpha(self.h, float(alpha)))

    def getAlpha(self):
        return float(_core._lib.dsr_gcc_alpha(self.h))

    def stateBytes(self, U):
        return int(_core._lib.dsr_gcc_state_bytes(self.h, int(U)))

    def newState(self, U, device="cuda:0"):
        st = torch.zeros((self.stateBytes(U) + 7) // 8, dtype=torch.float64, device=device)
        check(_core._lib.dsr_gcc_state_init(self.h, _dev(st), int(U), cur_stream()))
        return st

    def run(self, X, sad, timestamp, state, nframes=None, smooth=True, minDelay=None, maxDelay=None, want_corr=False, want_xspec=False):
        """X cuda complex64 or complex128 [U][C][T][fftLen/2+1], sad [U][T] (non-zero = speech), timestamp [U][T] float64 ->
        dict(result [U][T][P][3] = delay, maxCorr, ratio; valid [U][T][P] int32; corr [U][T][P][fftLen] and xspec [U][T][P][fftLen/2+1] on request)"""
        U, Cn, T, F = X.shape
        if Cn != self.C or F != self.F or X.dtype not in (torch.complex64, torch.complex128):
            raise ValueError("X: complex64 or complex128 [U][%d][T][%d] expected" % (self.C, self.F))
        dev = X.device
        sad = sad.to(device=dev, dtype=torch.int32).contiguous(); timestamp = timestamp.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(sad.shape) != (U, T) or tuple(timestamp.shape) != (U, T):
            raise ValueError("sad, timestamp: [U][T] expected")
        r = dict(result=torch.zeros((U, T, self.P, 3), dtype=torch.float64, device=dev), valid=torch.zeros((U, T, self.P), dtype=torch.int32, device=dev))
        r["corr"] = torch.zeros((U, T, self.P, self.N), dtype=torch.float64, device=dev) if want_corr else None
        r["xspec"] = torch.zeros((U, T, self.P, F), dtype=torch.complex128, device=dev) if want_xspec else None
        Xc = torch.view_as_real(X.contiguous())
        check(_core._lib.dsr_gcc_run(self.h, _dev(Xc), int(X.dtype == torch.complex128), _dev(nframes) if nframes is not None else None, _dev(sad), _dev(timestamp),
                               int(bool(smooth)), float(-self.HUGE if minDelay is None else minDelay), float(self.HUGE if maxDelay is None else maxDelay), U, T,
                               _dev(state), _dev(r["result"]), _dev(r["valid"]), _dev(r["corr"]) if want_corr else None,
                               _dev(torch.view_as_real(r["xspec"])) if want_xspec else None, cur_stream()))
        return r

    def findMaximum(self, state, U, minDelay=None, maxDelay=None):
        """findMaximum over the carried correlations -> (result [U][P][3], valid [U][P]) on the device"""
        res = torch.zeros((U, self.P, 3), dtype=torch.float64, device=state.device); valid = torch.zeros((U, self.P), dtype=torch.int32, device=state.device)
        check(_core._lib.dsr_gcc_find_maximum(self.h, float(-self.HUGE if minDelay is None else minDelay), float(self.HUGE if maxDelay is None else maxDelay), int(U),
                                        _dev(state), _dev(res), _dev(valid), cur_stream()))
        return res, valid

    def read(self, state, U, what, u, index):
        """-> (array, exists): noise power [F] float64, noise cross-spectrum / cross-spectrum [F] complex128, correlation [fftLen] float64"""
        cplx = what in (1, 2); n = self.N if what == 3 else self.F
        out = np.zeros(n, np.complex128 if cplx else np.float64); ex = C.c_int32(0)
        check(_core._lib.dsr_gcc_state_read(self.h, _dev(state), int(U), int(what), int(u), int(index), _ptr(out), n * (2 if cplx else 1), C.byref(ex)))
        return out, bool(ex.value)

    def channelDelays(self, pairDelays):
        """per-channel delays (channel 0 at zero) for dsr_bf_calc_array_manifold / Beamformer.calcArrayManifoldVectors from the P pair delays"""
        d = _np(pairDelays, np.float64).ravel()
        if d.size != self.P:
            raise DsrError(E_DIMENSION, "%d pair delays for %d pairs" % (d.size, self.P))
        out = np.zeros(self.C, np.float64); check(_core._lib.dsr_gcc_channel_delays(self.h, _ptr(d), _ptr(out))); return out


def cctde(a, b, fftLen, nHeldMaxCC=1, sampleRate=16000):
    """CCTDE::next over a batch of block pairs (dsr_cctde_run): a, b cuda float32 [n][blockLen] -> (delays [n][nHeld] seconds, lags as FFT
    indices [n][nHeld] int32, correlation values [n][nHeld])"""
    load()
    a = a.to(torch.float32).contiguous(); b = b.to(torch.float32).contiguous()
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError("a, b: float32 [n][blockLen] of one shape expected")
    n, bl = a.shape
    d = torch.zeros((n, nHeldMaxCC), dtype=torch.float64, device=a.device); ar = torch.zeros((n, nHeldMaxCC), dtype=torch.int32, device=a.device)
    v = torch.zeros((n, nHeldMaxCC), dtype=torch.float64, device=a.device)
    check(_core._lib.dsr_cctde_run(_dev(a), _dev(b), int(n), int(bl), int(fftLen), int(nHeldMaxCC), int(sampleRate), _dev(d), _dev(ar), _dev(v), cur_stream()))
    return d, ar, v


class SearchGrid(Handle):
    """SGB4LinearArray / SGB4CircularArray (include/dsr.h section 2f): kind "linear" or "circular"; host code, no GPU needed.  Units are
    millimetres.  enumerate() walks the whole far-field grid once."""
    KINDS = {"linear": 0, "circular": 1}

    _destroy = "dsr_sgb_destroy"

    def __init__(self, kind, nChan, isFarField=True, samplingFreq=16000):
        L = load(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind); self.C = int(nChan); self.fs = int(samplingFreq)
        self._create(L.dsr_sgb_create, self.kind, int(nChan), int(bool(isFarField)), int(samplingFreq))

    def setDistanceBtwMicrophones(self, distance):
        check(_core._lib.dsr_sgb_set_distance(self.h, float(distance)))

    def setPositionsOfMicrophones(self, mpos):
        m = _np(mpos, np.float64); check(_core._lib.dsr_sgb_set_positions(self.h, _ptr(m), int(m.shape[0])))

    def setRadius(self, radius, height=0.0):
        check(_core._lib.dsr_sgb_set_radius(self.h, float(radius), float(height)))

    def reset(self):
        check(_core._lib.dsr_sgb_reset(self.h))

    def nextSearchGrid(self):
        more = C.c_int32(0); check(_core._lib.dsr_sgb_next(self.h, C.byref(more))); return bool(more.value)

    def getSearchPosition(self):
        out = np.zeros(3); check(_core._lib.dsr_sgb_position(self.h, _ptr(out))); return out

    def getTimeDelays(self):
        out = np.zeros(self.C); check(_core._lib.dsr_sgb_time_delays(self.h, _ptr(out))); return out

    def maxTimeDelay(self):
        return float(_core._lib.dsr_sgb_max_time_delay(self.h))

    def chanN(self):
        return int(_core._lib.dsr_sgb_chan_n(self.h))

    def samplingFrequency(self):
        return int(_core._lib.dsr_sgb_sampling_frequency(self.h))

    def microphonePositions(self):
        out = np.zeros((self.C, 3)); check(_core._lib.dsr_sgb_microphone_positions(self.h, _ptr(out))); return out

    def enumerate(self):
        """-> (positions [G][3], delays [G][C] seconds, tau [G][C] int32)"""
        G = C.c_int32(0); check(_core._lib.dsr_sgb_enumerate(self.h, 0, C.byref(G), None, None, None)); g = G.value
        pos = np.zeros((g, 3)); d = np.zeros((g, self.C)); tau = np.zeros((g, self.C), np.int32)
        check(_core._lib.dsr_sgb_enumerate(self.h, g, C.byref(G), _ptr(pos), _ptr(d), _ptr(tau)))
        return pos, d, tau


def mcc_check(sgb, maxSource=1, blockLen=0):
    """what MccLocalizer and its run() refuse, checked on the host (dsr_mcc_check)"""
    load(); check(_core._lib.dsr_mcc_check(sgb.h, int(maxSource), int(blockLen)))


class MccLocalizer(Handle):
    """MCCLocalizer over a batch (include/dsr.h section 2f): the grid of `sgb` is walked once at construction."""

    _destroy = "dsr_mcc_destroy"

    def __init__(self, sgb, maxSource=1):
        L = load(); self.sgb = sgb
        self._create(L.dsr_mcc_create, sgb.h, int(maxSource))
        self.C = int(L.dsr_mcc_chan_n(self.h)); self.G = int(L.dsr_mcc_grid_n(self.h)); self.S = int(maxSource); self.D = int(L.dsr_mcc_max_sample_delay(self.h))

    def _x(self, x, blockLen):
        if x.dim() != 3 or x.shape[1] != self.C or x.dtype != torch.float32:
            raise ValueError("x: float32 [U][%d][N] expected" % self.C)
        x = x.contiguous(); U, _, N = x.shape
        return x, U, N, N // int(blockLen) if blockLen > 0 else 0

    def run(self, x, blockLen, nsamples=None, want_costmap=False, want_R=False, want_eig=True):
        """x cuda float32 [U][C][N] -> dict(valid [U][B], index [U][B][S], cost [U][B][S], tau [U][B][S][C], position [U][B][S][3],
        eig [U][B][S][C], costmap [U][B][G] and R [U][B][C][C] on request)"""
        x, U, N, B = self._x(x, blockLen); dev = x.device; S = self.S; Cn = self.C
        z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
        r = dict(valid=z((U, B), torch.int32), index=z((U, B, S), torch.int32), cost=z((U, B, S)), tau=z((U, B, S, Cn), torch.int32), position=z((U, B, S, 3)),
                 eig=z((U, B, S, Cn)) if want_eig else None, costmap=z((U, B, self.G)) if want_costmap else None, R=z((U, B, Cn, Cn)) if want_R else None)
        if nsamples is not None:
            nsamples = nsamples.to(device=dev, dtype=torch.int32).contiguous()
        opt = lambda t: _dev(t) if t is not None else None
        check(_core._lib.dsr_mcc_run(self.h, _dev(x), opt(nsamples), U, N, int(blockLen), _dev(r["valid"]), _dev(r["index"]), _dev(r["cost"]), _dev(r["tau"]),
                               _dev(r["position"]), opt(r["eig"]), opt(r["costmap"]), opt(r["R"]), cur_stream()))
        return r

    def calc(self, x, blockLen, delays, normalizeVariance=True, nsamples=None, want_R=False, want_eig=False):
        """MCCCalculator over the batch -> dict(valid [U][B], cost [U][B], tau [C] numpy, eig [U][B][C], R [U][B][C][C])"""
        x, U, N, B = self._x(x, blockLen); dev = x.device; Cn = self.C
        d = _np(delays, np.float64).ravel()
        if d.size != Cn:
            raise DsrError(E_DIMENSION, "%d delays for %d channels" % (d.size, Cn))
        r = dict(valid=torch.zeros((U, B), dtype=torch.int32, device=dev), cost=torch.zeros((U, B), dtype=torch.float64, device=dev), tau=np.zeros(Cn, np.int32),
                 eig=torch.zeros((U, B, Cn), dtype=torch.float64, device=dev) if want_eig else None,
                 R=torch.zeros((U, B, Cn, Cn), dtype=torch.float64, device=dev) if want_R else None)
        if nsamples is not None:
            nsamples = nsamples.to(device=dev, dtype=torch.int32).contiguous()
        opt = lambda t: _dev(t) if t is not None else None
        check(_core._lib.dsr_mcc_calc(self.h, _dev(x), opt(nsamples), U, N, int(blockLen), _ptr(d), int(bool(normalizeVariance)), _dev(r["valid"]), _dev(r["cost"]),
                                _ptr(r["tau"]), opt(r["eig"]), opt(r["R"]), cur_stream()))
        return r

    def channelDelays(self, tau):
        """tau [C] samples -> the delays in seconds that Beamformer.calcArrayManifoldVectors takes"""
        t = _np(tau, np.int32).ravel()
        if t.size != self.C:
            raise DsrError(E_DIMENSION, "%d shifts for %d channels" % (t.size, self.C))
        out = np.zeros(self.C); check(_core._lib.dsr_mcc_channel_delays(self.h, _ptr(t), _ptr(out))); return out

    def setTiming(self, on=True):
        check(_core._lib.dsr_mcc_set_timing(self.h, int(bool(on))))

    def kernelMs(self):
        out = np.zeros(3); check(_core._lib.dsr_mcc_kernel_ms(self.h, _ptr(out))); return out


class MccCalculator(MccLocalizer):
    """MCCCalculator over a batch: one candidate from the caller's delays; calling the object is calc() with the constructor's normalizeVariance."""

    def __init__(self, sgb, normalizeVariance=True):
        MccLocalizer.__init__(self, sgb, 1); self.normalizeVariance = bool(normalizeVariance)

    def __call__(self, x, blockLen, delays, nsamples=None, want_R=False, want_eig=False):
        return self.calc(x, blockLen, delays, self.normalizeVariance, nsamples, want_R, want_eig)
