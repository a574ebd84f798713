"""btk.localization: GCCRawPtr, GCCGnnSubPtr, GCCPhatPtr, GCCGnnSubPhatPtr, GCCMLRRawPtr, GCCMLRGnnSubPtr (localization.i:94-143) -- constructor
keywords and defaults of localization.h:123.  The per-call methods (dsr_gcc_calculate / dsr_gcc_peak / dsr_gcc_get) run the batch kernels with
one utterance and one frame on the object's own carried state; run_batch() is the batch face (dsr._capi.Gcc.run).  Before a pair's first speech frame the answers are zero (the reference
reads an uninitialised correlation there)."""
import ctypes as C

import numpy as np

from .. import _capi as K


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
