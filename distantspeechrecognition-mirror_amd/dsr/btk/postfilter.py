"""btk.postfilter: ZelinskiPostFilterPtr (postfilter.i:77-90, postfilter.h:95-126) and its relatives; the noise suppressors of
spectralsubtraction.h and the binaural masks and threshold estimators of binauralprocessing.h (postfilter.i:150-440)."""
import ctypes as C

import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, lib, _new

TYPE_ZELINSKI1_REAL, TYPE_ZELINSKI1_ABS, TYPE_APAB, TYPE_ZELINSKI2, NO_USE_POST_FILTER = 0x01, 0x02, 0x04, 0x08, 0x00


class ZelinskiPostFilterPtr(FeatureStreamPtr):
    def __init__(self, output, M, alpha=0.6, type=2, minFrames=0, nm="ZelinskPostFilter"):
        h, _ = _new(lib().dsr_zelinski_stream_create, output._h, int(M), float(alpha), int(type), int(minFrames), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(output,)); self._M = M; self._type = type; self._chans = []

    def setBeamformer(self, bf):
        """the beamformer's snapshot array (its channel streams) and its weight object (postfilter.cc:376-385,441-444):
        arrayManifold(), or wq() for TYPE_ZELINSKI2 -- both are the delay-and-sum vectors of calcArrayManifoldVectors here"""
        w = bf._weights().get(0)
        for c in bf._chans:
            K.check(lib().dsr_zelinski_stream_set_channel(self._h, c._h)); self._chans.append(c)
        for f in range(self._M // 2 + 1):
            self.setArrayManifoldVector(f, w[f], False)

    def setSnapShotArray(self, channels):
        for c in channels:
            K.check(lib().dsr_zelinski_stream_set_channel(self._h, c._h)); self._chans.append(c)

    def setArrayManifoldVector(self, fbinX, arrayManifoldVector, halfBandShift=False, NC=1):
        if halfBandShift:
            raise K.DsrError(2, "halfBandShift==true is not supported")
        v = np.ascontiguousarray(arrayManifoldVector, np.complex128)
        K.check(lib().dsr_zelinski_stream_set_manifold(self._h, int(fbinX), v.ctypes.data_as(C.c_void_p), v.size))


class McCowanPostFilterPtr(ZelinskiPostFilterPtr):
    """postfilter.i:113-126 (McCowanPostFilter, postfilter.cc:502-945)."""

    def __init__(self, output, fftLen, alpha=0.6, type=2, minFrames=0, threshold=0.99, nm="McCowanPostFilterPtr"):
        h, _ = _new(lib().dsr_mccowan_stream_create, output._h, int(fftLen), float(alpha), int(type), int(minFrames), float(threshold), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(output,)); self._M = fftLen; self._type = type; self._chans = []; self._C = None

    def _noise(self, what, fbinX, data, chanN, a=0.0, b=0.0):
        d = None if data is None else np.ascontiguousarray(data)
        K.check(lib().dsr_mccowan_stream_set_noise(self._h, what, int(fbinX), None if d is None else d.ctypes.data_as(C.c_void_p), int(chanN), float(a), float(b)))

    def setDiffuseNoiseModel(self, micPositions, sampleRate, sspeed=343740.0):
        mp = np.ascontiguousarray(micPositions, np.float64); self._C = mp.shape[0]
        self._noise(1, 0, mp, self._C, sampleRate, sspeed); return True

    def setNoiseSpatialSpectralMatrix(self, fbinX, Rnn):
        r = np.ascontiguousarray(Rnn, np.complex128); self._C = r.shape[0]
        self._noise(0, fbinX, r, self._C); return True

    def setAllLevelsOfDiagonalLoading(self, diagonalWeight):
        self._noise(2, -1, None, self._C or 0, diagonalWeight)

    def setLevelOfDiagonalLoading(self, fbinX, diagonalWeight):
        self._noise(2, fbinX, None, self._C or 0, diagonalWeight)

    def divideAllNonDiagonalElements(self, myu):
        self._noise(3, 0, None, self._C or 0, myu)


class LefkimmiatisPostFilterPtr(McCowanPostFilterPtr):
    """postfilter.i (LefkimmiatisPostFilter, postfilter.h:180-204, postfilter.cc:948-1210); calcInverseNoiseSpatialSpectralMatrix() is
    implied: the inverse is refreshed whenever the coherence matrices or the manifold change."""

    def __init__(self, output, fftLen, minSV=1.0E-8, fbinX1=0, alpha=0.6, type=2, minFrames=0, threshold=0.99, nm="LefkimmiatisPostFilte"):
        h, _ = _new(lib().dsr_lefkimmiatis_stream_create, output._h, int(fftLen), float(minSV), int(fbinX1), float(alpha), int(type), int(minFrames),
                    float(threshold), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(output,)); self._M = fftLen; self._type = type; self._chans = []; self._C = None

    def calcInverseNoiseSpatialSpectralMatrix(self):
        return None


class highPassFilterPtr(FeatureStreamPtr):
    """postfilter.i:229-252 (highPassFilter, postfilter.cc:1222-1261)."""

    def __init__(self, output, cutOffFreq, sampleRate, nm="highPassFilter"):
        h, _ = _new(lib().dsr_highpass_filter_create, output._h, float(cutOffFreq), int(sampleRate), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(output,))


class averagePSDEstimatorPtr(object):
    """postfilter.i:150-170 (averagePSDEstimator, spectralsubtraction.cc:52-129): one SpectralSubtractor channel's estimator on its own"""

    def __init__(self, fftLen2, alpha=-1.0):
        self._s = K.SpectralSubtractor(2 * int(fftLen2)); self._s.setChannel(float(alpha)); self._st = None; self._F = int(fftLen2) + 1

    def _state(self):
        if self._st is None:
            self._st = self._s.newState(1)
        return self._st

    def addSample(self, sample):
        import torch
        x = np.ascontiguousarray(np.asarray(sample, np.complex128)[:self._F].astype(np.complex64)).reshape(1, 1, 1, self._F)
        self._s.startTraining(); self._s.apply(torch.from_numpy(x).to(self._state().device), self._state(), train_only=True); return True

    def average(self):
        self._s.stopTraining(self._state()); return self.getEstimate()

    def getEstimate(self):
        return self._s.read(self._state(), 0, 0, 0)

    def clear(self):
        self._s.clear(self._state())

    def clearSamples(self):
        self._s.clearNoiseSamples(self._state())

    def readEstimates(self, fn):
        self._s.readNoiseFile(fn, self._state()); return True

    def writeEstimates(self, fn):
        self._s.writeNoiseFile(fn, self._state()); return True


class SpectralSubtractorPtr(FeatureStreamPtr):
    """postfilter.i:182-184 (SpectralSubtractor, spectralsubtraction.cc:141-267).  An utterance is computed at its first next(): the control calls
    act from the next reset() (or __iter__) on."""

    def __init__(self, fftLen, halfBandShift=False, ft=1.0, flooringV=0.001, nm="SpectralSubtractor"):
        h, _ = _new(lib().dsr_specsub_stream_create, int(fftLen), int(bool(halfBandShift)), float(ft), float(flooringV), nm.encode())
        FeatureStreamPtr.__init__(self, h); self._chans = []

    def setChannel(self, chan, alpha=-1):
        K.check(lib().dsr_specsub_stream_set_channel(self._h, chan._h, float(alpha))); self._chans.append(chan)

    def _ctl(self, what, value=0.0, fn=None, idx=0):
        K.check(lib().dsr_specsub_stream_control(self._h, int(what), float(value), None if fn is None else str(fn).encode(), int(idx)))

    def setNoiseOverEstimationFactor(self, ft):
        self._ctl(0, ft)

    def startTraining(self):
        self._ctl(1)

    def stopTraining(self):
        self._ctl(2)

    def startNoiseSubtraction(self):
        self._ctl(3)

    def stopNoiseSubtraction(self):
        self._ctl(4)

    def clear(self):
        self._ctl(5)

    def clearNoiseSamples(self):
        self._ctl(6)

    def readNoiseFile(self, fn, idx=0):
        self._ctl(7, 0.0, fn, idx); return True

    def writeNoiseFile(self, fn, idx=0):
        self._ctl(8, 0.0, fn, idx); return True


class WienerFilterPtr(FeatureStreamPtr):
    """postfilter.i:213-215 (WienerFilter, spectralsubtraction.cc:269-347)"""

    def __init__(self, targetSignal, noiseSignal, halfBandShift=False, alpha=0.0, flooringV=0.001, beta=1.0, nm="WienerFilter"):
        h, _ = _new(lib().dsr_wiener_stream_create, targetSignal._h, noiseSignal._h, int(bool(halfBandShift)), float(alpha), float(flooringV), float(beta), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(targetSignal, noiseSignal))

    def setNoiseAmplificationFactor(self, beta):
        K.check(lib().dsr_wiener_stream_control(self._h, 0, float(beta)))

    def startUpdatingNoisePSD(self):
        K.check(lib().dsr_wiener_stream_control(self._h, 1, 0.0))

    def stopUpdatingNoisePSD(self):
        K.check(lib().dsr_wiener_stream_control(self._h, 2, 0.0))


class BinaryMaskFilterPtr(FeatureStreamPtr):
    """postfilter.i:274-276 (BinaryMaskFilter, binauralprocessing.cc:47-106): next() only advances, the output stays zero"""
    _KIND = 0

    def __init__(self, chanX, srcL, srcR, M, threshold, alpha, dEta=0.01, nm="BinaryMaskFilter", dPowerCoeff=0.0):
        h, _ = _new(lib().dsr_binmask_stream_create, self._KIND, int(chanX), srcL._h, srcR._h, int(M), float(threshold), float(alpha), float(dEta), float(dPowerCoeff),
                    nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(srcL, srcR)); self._M = int(M)

    def setThreshold(self, threshold):
        K.check(lib().dsr_binmask_stream_set_threshold(self._h, float(threshold)))

    def setThresholds(self, thresholds):
        t = np.ascontiguousarray(thresholds, np.float64); K.check(lib().dsr_binmask_stream_set_thresholds(self._h, t.ctypes.data_as(C.c_void_p), t.size))

    def getThreshold(self):
        v = C.c_double(0.0); K.check(lib().dsr_binmask_stream_threshold(self._h, C.byref(v))); return v.value

    def getThresholds(self):
        out = np.zeros(self._M // 2 + 1); ex = C.c_int32(0)
        K.check(lib().dsr_binmask_stream_thresholds(self._h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(ex))); return out if ex.value else None


class KimBinaryMaskFilterPtr(BinaryMaskFilterPtr):
    """postfilter.i:301-303 (KimBinaryMaskFilter, binauralprocessing.cc:121-211).  dPowerCoeff: the reference's default `1/15` is integer division,
    0.0; the filter never uses it."""
    _KIND = 1

    def __init__(self, chanX, srcL, srcR, M, threshold, alpha, dEta=0.01, dPowerCoeff=0.0, nm="KimBinaryMaskFilter"):
        BinaryMaskFilterPtr.__init__(self, chanX, srcL, srcR, M, threshold, alpha, dEta, nm, dPowerCoeff)


class IIDBinaryMaskFilterPtr(BinaryMaskFilterPtr):
    """postfilter.i:364-368 (IIDBinaryMaskFilter, binauralprocessing.cc:431-520)"""
    _KIND = 2

    def __init__(self, chanX, srcL, srcR, M, threshold, alpha, dEta=0.01, nm="IIDBinaryMaskFilter"):
        BinaryMaskFilterPtr.__init__(self, chanX, srcL, srcR, M, threshold, alpha, dEta, nm)


class KimITDThresholdEstimatorPtr(FeatureStreamPtr):
    """postfilter.i:332-336 (KimITDThresholdEstimator, binauralprocessing.cc:232-426).  dPowerCoeff defaults to the reference's `1/15` == 0.0
    (integer division), with which every cost function is degenerate: pass a value."""
    _KIND = 0

    def __init__(self, srcL, srcR, M, minThreshold=0.0, maxThreshold=0.0, width=0.02, minFreq=-1, maxFreq=-1, sampleRate=-1, dEta=0.01, dPowerCoeff=0.0,
                 nm="KimITDThresholdEstimator"):
        h, _ = _new(lib().dsr_thest_stream_create, self._KIND, srcL._h, srcR._h, int(M), float(minThreshold), float(maxThreshold), float(width), float(minFreq),
                    float(maxFreq), int(sampleRate), float(dEta), float(dPowerCoeff), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(srcL, srcR)); self._M = int(M)

    def calcThreshold(self):
        v = C.c_double(0.0); K.check(lib().dsr_thest_stream_calc_threshold(self._h, C.byref(v))); return v.value

    def getThreshold(self):
        v = C.c_double(0.0); K.check(lib().dsr_thest_stream_threshold(self._h, C.byref(v))); return v.value

    def getCostFunction(self, freqX=0):
        out = np.zeros(max(1, lib().dsr_thest_stream_n_cand(self._h))); n = C.c_size_t(0)
        K.check(lib().dsr_thest_stream_get_cost_function(self._h, int(freqX), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))); return out[:n.value].copy()


class IIDThresholdEstimatorPtr(KimITDThresholdEstimatorPtr):
    """postfilter.i:396-400 (IIDThresholdEstimator, binauralprocessing.cc:525-683)"""
    _KIND = 1

    def __init__(self, srcL, srcR, M, minThreshold=0.0, maxThreshold=0.0, width=0.02, minFreq=-1, maxFreq=-1, sampleRate=-1, dEta=0.01, dPowerCoeff=0.0,
                 nm="IIDThresholdEstimator"):
        KimITDThresholdEstimatorPtr.__init__(self, srcL, srcR, M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, nm)


class FDIIDThresholdEstimatorPtr(KimITDThresholdEstimatorPtr):
    """postfilter.i:427-429 (FDIIDThresholdEstimator, binauralprocessing.cc:702-928); _beta is uninitialised there, 3.0 here"""
    _KIND = 2

    def __init__(self, srcL, srcR, M, minThreshold=0.0, maxThreshold=0.0, width=1000.0, dEta=0.01, dPowerCoeff=0.0, nm="FDIIDThresholdEstimator"):
        KimITDThresholdEstimatorPtr.__init__(self, srcL, srcR, M, minThreshold, maxThreshold, width, -1, -1, -1, dEta, dPowerCoeff, nm)

    def getThresholds(self):
        out = np.zeros(self._M // 2 + 1); K.check(lib().dsr_thest_stream_thresholds(self._h, out.ctypes.data_as(C.c_void_p), out.size)); return out
