"""btk.localization: GCCRawPtr, GCCGnnSubPtr, GCCPhatPtr, GCCGnnSubPhatPtr, GCCMLRRawPtr, GCCMLRGnnSubPtr (localization.i:94-143) -- constructor
keywords and defaults of localization.h:123.  The per-call methods (dsr_gcc_calculate / dsr_gcc_peak / dsr_gcc_get) run the batch kernels with
one utterance and one frame on the object's own carried state; run_batch() is the batch face (dsr._capi.Gcc.run).  Before a pair's first speech frame the answers are zero (the reference
reads an uninitialised correlation there).

SearchGridBuilderPtr, SGB4LinearArrayPtr, SGB4CircularArrayPtr, MCCLocalizerPtr and MCCCalculatorPtr (MCCLocalizer.h:55-301) follow at the end: the
grids are host code, the localiser and the calculator are streams over float block streams (include/dsr.h section 2f)."""
import ctypes as C

import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, lib


class _GCC(object):
    _KIND = "raw"

    def __init__(self, sampleRate=44100.0, fftLen=2048, nChan=16, pairs=6, alpha=0.95, beta=0.5, q=0.3, interpolate=True, noisereduction=True):
        self._g = K.Gcc(self._KIND, np.zeros((pairs, 2), np.int32), sampleRate=sampleRate, fftLen=fftLen, nChan=nChan, alpha=alpha, beta=beta, q=q,
                        interpolate=interpolate, noisereduction=noisereduction)
        self._last = 0; self._ret = np.zeros(3)

    def calculate(self, spectralSample1, chan1, spectralSample2, chan2, pair, timestamp, sad=False, smooth=True):
        s1 = np.ascontiguousarray(np.asarray(spectralSample1, np.complex128).ravel()); s2 = np.ascontiguousarray(np.asarray(spectralSample2, np.complex128).ravel())
        K.check(K.load().dsr_gcc_calculate(self._g.h, K._ptr(s1), s1.size, int(chan1), K._ptr(s2), s2.size, int(chan2), int(pair), float(timestamp),
                                           int(bool(sad)), int(bool(smooth))))
        self._last = int(pair)

    def findMaximum(self, minDelay=-K.Gcc.HUGE, maxDelay=K.Gcc.HUGE):
        out = np.zeros(3); valid = C.c_int32(0)
        K.check(K.load().dsr_gcc_peak(self._g.h, self._last, float(minDelay), float(maxDelay), K._ptr(out), C.byref(valid)))
        self._ret = out
        return self._ret

    def getPeakDelay(self):
        return float(self._ret[0])

    def getPeakCorr(self):
        return float(self._ret[1])

    def getRatio(self):
        return float(self._ret[2])

    def _read(self, what, index, always=False):
        cplx = what in (K.Gcc.NOISE_CROSS, K.Gcc.CROSS); n = self._g.N if what == K.Gcc.CORRELATION else self._g.F
        out = np.zeros(n, np.complex128 if cplx else np.float64); ex = C.c_int32(0)
        K.check(K.load().dsr_gcc_get(self._g.h, int(what), int(index), K._ptr(out), n * (2 if cplx else 1), C.byref(ex)))
        return out if (ex.value or always) else None

    def getNoisePowerSpectrum(self, chan):
        return self._read(K.Gcc.NOISE_POWER, chan)

    def getNoiseCrossSpectrum(self, pair):
        return self._read(K.Gcc.NOISE_CROSS, pair)

    def getCrossSpectrum(self):
        return self._read(K.Gcc.CROSS, self._last, True)

    def getCrossCorrelation(self):
        return self._read(K.Gcc.CORRELATION, self._last, True)

    def setAlpha(self, alpha):
        self._g.setAlpha(alpha)

    def getAlpha(self):
        return self._g.getAlpha()

    @classmethod
    def run_batch(cls, X, sad, timestamp, pairs, sampleRate=44100.0, alpha=0.95, beta=0.5, q=0.3, interpolate=True, noisereduction=True, state=None,
                  nframes=None, smooth=True, minDelay=None, maxDelay=None, want_corr=False, want_xspec=False):
        """the frame loop over a batch: X cuda complex [U][C][T][fftLen/2+1], sad / timestamp [U][T], pairs [P][2] -> (dict of dsr._capi.Gcc.run,
        the Gcc plan, the state to hand to the next block)"""
        U, Cn, T, F = X.shape
        g = K.Gcc(cls._KIND, pairs, sampleRate=sampleRate, fftLen=2 * (F - 1), nChan=Cn, alpha=alpha, beta=beta, q=q, interpolate=interpolate,
                  noisereduction=noisereduction)
        if state is None:
            state = g.newState(U, X.device)
        return g.run(X, sad, timestamp, state, nframes, smooth, minDelay, maxDelay, want_corr, want_xspec), g, state


class GCCRawPtr(_GCC):
    _KIND = "raw"


class GCCGnnSubPtr(_GCC):
    _KIND = "gnnsub"


class GCCPhatPtr(_GCC):
    _KIND = "phat"


class GCCGnnSubPhatPtr(_GCC):
    _KIND = "gnnsubphat"


class GCCMLRRawPtr(_GCC):
    _KIND = "mlrraw"


class GCCMLRGnnSubPtr(_GCC):
    _KIND = "mlrgnnsub"


# ---- MCCLocalizer.h:55-301: the search grids (host code) and the localiser / calculator streams (dsr_mcc_stream_create) ------------------------
class SearchGridBuilderPtr(K.SearchGrid):
    """SearchGridBuilder(nChan, isFarField, samplingFreq=16000).  The base class of the reference has no walk of its own; here it is the
    linear one until a geometry setter says otherwise."""
    _KIND = "linear"

    def __init__(self, nChan, isFarField, samplingFreq=16000):
        K.SearchGrid.__init__(self, self._KIND, nChan, isFarField, samplingFreq)


class SGB4LinearArrayPtr(SearchGridBuilderPtr):
    _KIND = "linear"


class SGB4CircularArrayPtr(SearchGridBuilderPtr):
    _KIND = "circular"


class MCCLocalizerPtr(FeatureStreamPtr):
    """MCCLocalizer(sgb, maxSource=1, nm): next() pulls one block from every channel and returns the best position (3 doubles)."""

    def __init__(self, sgbPtr, maxSource=1, nm="MCCSourceLocalizer"):
        self._m = K.MccLocalizer(sgbPtr, maxSource); self._chans = []
        h = C.c_void_p(); K.check(self._create(nm.encode(), h))
        FeatureStreamPtr.__init__(self, h)

    def _create(self, nm, h):
        return lib().dsr_mcc_stream_create(self._m.h, nm, C.byref(h))

    def __del__(self):
        FeatureStreamPtr.__del__(self)                       # the stream first: it uses the plan

    def setChannel(self, chan):
        K.check(lib().dsr_mcc_stream_set_channel(self._h, chan._h)); self._chans.append(chan)

    def _get(self, what, nth, n):
        out = np.zeros(n); m = C.c_size_t(0)
        K.check(lib().dsr_mcc_stream_get(self._h, int(what), int(nth), K._ptr(out), n, C.byref(m)))
        return out[:m.value]

    def getNthBestDelayedSample(self, nth, chanX):
        return int(self._get(1, nth, self._m.C)[chanX])

    def getNthBestMCCC(self, nth):
        return float(1.0 - np.exp(self._get(0, nth, 1)[0]))

    def getNthBestPosition(self, nth):
        return self._get(2, nth, 3)

    def getDelayedSample(self, chanX):
        return self.getNthBestDelayedSample(0, chanX)

    def getMaxMCCC(self):
        return self.getNthBestMCCC(0)

    def getPosition(self):
        return self.getNthBestPosition(0)

    def getEigenValues(self):
        return self._get(3, 0, self._m.C)

    def getR(self):
        return self._get(4, 0, self._m.C * self._m.C).reshape(self._m.C, self._m.C)

    def getChannelDelays(self, nth=0):
        """the nth best candidate's tau / fs, for calcArrayManifoldVectors"""
        return self._m.channelDelays(self._get(1, nth, self._m.C).astype(np.int32))


class MCCCalculatorPtr(MCCLocalizerPtr):
    """MCCCalculator(sgb, normalizeVariance=True, nm): next() returns a vector whose element 0 is the cost of the delays set with setTimeDelays()."""

    def __init__(self, sgbPtr, normalizeVariance=True, nm="MCCCalculator"):
        self._nv = bool(normalizeVariance)
        MCCLocalizerPtr.__init__(self, sgbPtr, 1, nm)

    def _create(self, nm, h):
        return lib().dsr_mcccalc_stream_create(self._m.h, int(self._nv), nm, C.byref(h))

    def setTimeDelays(self, delays):
        d = np.ascontiguousarray(np.asarray(delays, np.float64).ravel())
        K.check(lib().dsr_mcccalc_stream_set_time_delays(self._h, K._ptr(d), d.size))

    def getCostV(self):
        return float(self._get(0, 0, 1)[0])

    def getMCCC(self):
        return float(1.0 - np.exp(self.getCostV()))
