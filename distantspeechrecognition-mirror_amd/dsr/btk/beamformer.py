"""btk.beamformer: SubbandDSPtr / SubbandGSCPtr / SubbandGSCRLSPtr / SubbandMMIPtr / SubbandMVDRPtr (beamformer.i:227-323) and
DOAEstimatorSRPDSBLAPtr (beamformer.i:479-513), EigenBeamformerPtr / SphericalDSBeamformerPtr / DOAEstimatorSRPEBPtr /
DOAEstimatorSRPSphDSBPtr (beamformer.i:416-633) as streams."""
import ctypes as C

import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, lib, _new


class _Subband(FeatureStreamPtr):
    _MODE = 0

    def __init__(self, fftLen=512, halfBandShift=False, nm="SubbandBeamformer"):
        if halfBandShift and self._MODE == 1:
            raise K.DsrError(2, "halfBandShift==true is not yet supported")            # beamformer.cc:2324-2327
        self._fftLen, self._hbs, self._nm = fftLen, halfBandShift, nm
        self._chans = []; self._w = None; FeatureStreamPtr.__init__(self, None)

    def setChannel(self, chan):
        self._chans.append(chan)

    def chanN(self):
        return len(self._chans)

    def _weights(self):
        if self._w is None:
            self._w = K.Beamformer(self._fftLen, len(self._chans), self._hbs); self._w.select(self._MODE)
            h, _ = _new(lib().dsr_subband_bf_create, self._w.h, self._nm.encode()); self._h = h
            for c in self._chans:
                K.check(lib().dsr_subband_bf_set_channel(self._h, c._h))
        return self._w

    def calcArrayManifoldVectors(self, sampleRate, delays):
        self._weights().calcArrayManifoldVectors(sampleRate, delays)

    def next(self, frameX=-5):
        if self._w is None:
            raise K.DsrError(1, "call calcArrayManifoldVectorsX() once")
        return FeatureStreamPtr.next(self, frameX)

    __next__ = next


class SubbandDSPtr(_Subband):
    _MODE = 0


class SubbandGSCPtr(_Subband):
    _MODE = 2

    def calcGSCWeights(self, sampleRate, delaysT):
        self._weights().calcGSCWeights(sampleRate, delaysT)

    def setActiveWeights_f(self, fbinX, packedWeight):
        self._weights().setActiveWeights_f(fbinX, packedWeight)

    def zeroActiveWeights(self):
        self._weights().zeroActiveWeights()


class SubbandGSCRLSPtr(SubbandGSCPtr):
    """beamformer.i:227-253 (SubbandGSCRLS, beamformer.cc:1497-1698).  As in the reference the object keeps adapting across reset(): the
    precision matrices and active weights an utterance leaves are where the next one starts (dsr_bf_rls_carry); only
    initPrecisionMatrix()/setPrecisionMatrix() re-seed them."""

    def __init__(self, fftLen=512, halfBandShift=False, myu=0.9, sigma2=0.01, nm="SubbandGSCRLS"):
        SubbandGSCPtr.__init__(self, fftLen, halfBandShift, nm); self._myu, self._sigma2 = myu, sigma2

    def calcGSCWeights(self, sampleRate, delaysT):
        SubbandGSCPtr.calcGSCWeights(self, sampleRate, delaysT)
        self._weights().rlsConfig(self._myu, self._sigma2)
        self._weights().rlsCarry(True)

    def initPrecisionMatrix(self, sigma2=0.01):
        self._weights().initPrecisionMatrix(sigma2)

    def setPrecisionMatrix(self, fbinX, Pz):
        self._weights().setPrecisionMatrix(fbinX, Pz)

    def setQuadraticConstraint(self, alpha, qctype=1):
        self._weights().setQuadraticConstraint(alpha, qctype)

    def updateActiveWeightVecotrs(self, flag):
        self._weights().updateActiveWeightVecotrs(flag)


class SubbandMMIPtr(_Subband):
    """beamformer.i:255-287 (SubbandMMI, beamformer.cc:1753-2319): one GSC per source, Zelinski post-filter, binary mask."""

    def __init__(self, fftLen=512, halfBandShift=False, targetSourceX=0, nSource=2, pfType=0, alpha=0.9, nm="SubbandMMI"):
        _Subband.__init__(self, fftLen, halfBandShift, nm)
        self._args = (targetSourceX, nSource, pfType, alpha); self._mask = None

    def _weights(self):
        if self._w is None:
            t, n, pf, a = self._args
            self._w = K.SubbandMMI(self._fftLen, len(self._chans), self._hbs, t, n, pf, a)
            if self._mask is not None:
                self._w.useBinaryMask(*self._mask)
            h, _ = _new(lib().dsr_subband_mmi_stream_create, self._w.h, self._fftLen, self._nm.encode()); self._h = h
            for c in self._chans:
                K.check(lib().dsr_subband_bf_set_channel(self._h, c._h))
        return self._w

    def useBinaryMask(self, avgFactor=-1.0, fwidth=1, type=0):
        self._mask = (avgFactor, fwidth, type)
        if self._w is not None:
            self._w.useBinaryMask(avgFactor, fwidth, type)

    def calcWeights(self, sampleRate, delays):
        self._weights().calcWeights(sampleRate, delays)

    def calcWeightsN(self, sampleRate, delays, NC=2):
        self._weights().calcWeightsN(sampleRate, delays, NC)

    def setActiveWeights_f(self, fbinX, packedWeights, option=0):
        if self._w is None:
            raise K.DsrError(1, "call calcWeightsX() once")
        self._w.setActiveWeights_f(fbinX, packedWeights, option)

    def setHiActiveWeights_f(self, fbinX, pkdWa, pkdwb, option=0):
        if self._w is None:
            raise K.DsrError(1, "call calcWeightsX() once")
        self._w.setHiActiveWeights_f(fbinX, pkdWa, pkdwb, option)

    def next(self, frameX=-5):
        if self._w is None:
            raise K.DsrError(1, "call calcWeightsX() once")
        return FeatureStreamPtr.next(self, frameX)

    __next__ = next


class SubbandBlockingMatrixPtr(SubbandGSCPtr):
    """beamformer.h:453-460: a SubbandGSC under another name (its next() is SubbandGSC::next, beamformer.cc:2852-2917)."""


class SubbandMVDRPtr(_Subband):
    _MODE = 1

    def setDiffuseNoiseModel(self, micPositions, sampleRate, sspeed=343740.0):
        self._weights().setDiffuseNoiseModel(micPositions, sampleRate, sspeed); return True

    def divideAllNonDiagonalElements(self, myu):
        self._weights().divideAllNonDiagonalElements(myu)

    def setAllLevelsOfDiagonalLoading(self, w):
        self._weights().setAllLevelsOfDiagonalLoading(w)

    def setNoiseSpatialSpectralMatrix(self, fbinX, Rnn):
        self._weights().setNoiseSpatialSpectralMatrix(fbinX, Rnn); return True

    def calcMVDRWeights(self, sampleRate, dThreshold=1.0e-8, calcInverseMatrix=True):
        self._weights().calcMVDRWeights(sampleRate, dThreshold); return True

    def getMVDRWeights(self, fbinX):
        return self._weights().get(1)[fbinX]


def calcDelaysPolar2(azimuth, elevation, micPositions):
    return K.calcDelaysPolar2(np.float32(azimuth), np.float32(elevation), micPositions)


class SubbandMVDRGSCPtr(SubbandMVDRPtr):
    """beamformer.i (SubbandMVDRGSC, beamformer.h:394-425): setChannel, calcArrayManifoldVectors, noise model, calcMVDRWeights,
    calcBlockingMatrix1/2, setActiveWeights_f; next() = (w_mvdr - B wa)^H X."""
    _MODE = 4

    def setActiveWeights_f(self, fbinX, packedWeight):
        self._weights().setActiveWeights_f(fbinX, packedWeight)

    def zeroActiveWeights(self):
        self._weights().zeroActiveWeights()

    def calcBlockingMatrix1(self, sampleRate, delaysT):
        return self._weights().calcBlockingMatrix1(sampleRate, delaysT)

    def calcBlockingMatrix2(self):
        return self._weights().calcBlockingMatrix2()

    def upgradeBlockingMatrix(self):
        self._weights().upgradeBlockingMatrix()


class SubbandOrthogonalizerPtr(FeatureStreamPtr):
    """beamformer.i (SubbandOrthogonalizer, beamformer.cc:2817-2849): outChanX <= 0 hands the beamformer's output on, outChanX > 0 the output
    of column outChanX-1 of its blocking matrices."""

    def __init__(self, beamformer, outChanX=0, nm="SubbandOrthogonalizer"):
        beamformer._weights()
        h, _ = _new(lib().dsr_subband_orthogonalizer_create, beamformer._h, int(outChanX), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(beamformer,))


class DOAEstimatorSRPDSBLAPtr(FeatureStreamPtr):
    """beamformer.i:479-513 (DOAEstimatorSRPDSBLA, beamformer.cc:2920-3283): steered-response-power DOA estimation on a linear array.
    setChannel(analysis stream) per channel, setArrayGeometry(x positions), then iterate: next() returns the last search direction's
    delay-and-sum frame; getNBestRPs / getNBestDOAs / getEnergy / getResponsePowerMatrix describe the frame just returned,
    getFinalNBestHypotheses ranks the accumulated powers.  The constructor searches (-pi/2, pi/2, 0.1); setSearchParam() without
    arguments (0, pi/2, 0.1), as the two defaults of the reference differ."""

    def __init__(self, nBest, sampleRate, fftLen, nm="DOAEstimatorSRPDSBLAPtr"):
        self._nBest, self._fs, self._fftLen, self._nm = nBest, sampleRate, fftLen, nm
        self._chans = []; self._est = None; self._set = []; FeatureStreamPtr.__init__(self, None)

    def _estimator(self):
        if self._est is None:
            self._est = K.DoaSRP(self._nBest, self._fs, self._fftLen, len(self._chans))
            for fn, args in self._set:
                getattr(self._est, fn)(*args)
            h, _ = _new(lib().dsr_doa_stream_create, self._est.h, self._nm.encode()); self._h = h
            for c in self._chans:
                K.check(lib().dsr_subband_bf_set_channel(self._h, c._h))
        return self._est

    def _apply(self, fn, *args):
        if self._est is None:
            self._set.append((fn, args))
        else:
            getattr(self._est, fn)(*args)

    def setChannel(self, chan):
        if self._est is not None:
            raise K.DsrError(5, "channels must be set before the first frame")
        self._chans.append(chan)

    def chanN(self):
        return len(self._chans)

    def setArrayGeometry(self, positions):
        self._apply("setArrayGeometry", np.array(positions, np.float64))

    def setSearchParam(self, minTheta=0.0, maxTheta=np.pi / 2, widthTheta=0.1):
        self._apply("setSearchParam", minTheta, maxTheta, widthTheta)

    def setFrequencyRange(self, fbinMin, fbinMax):
        self._apply("setFrequencyRange", fbinMin, fbinMax)

    def setEnergyThreshold(self, engeryThreshold):
        self._apply("setEnergyThreshold", engeryThreshold)

    def _get(self, what, n):
        self._estimator()
        out = np.zeros(max(n, 1), np.float64); got = C.c_size_t()
        K.check(lib().dsr_doa_stream_get(self._h, what, K._ptr(out), out.size, C.byref(got)))
        return out[:got.value]

    def getNBestRPs(self):
        return self._get(0, self._nBest)

    def getNBestDOAs(self):
        return self._get(1, 2 * self._nBest).reshape(self._nBest, 2)

    def getEnergy(self):
        return float(np.float32(self._get(4, 1)[0]))

    def getResponsePowerMatrix(self):
        """[nTheta][1]: the last ungated frame's response powers (the accumulators after getFinalNBestHypotheses); None before the first frame"""
        v = self._get(2, self._estimator().thetaN())
        return v.reshape(-1, 1) if v.size else None

    def getAccumulators(self):
        return self._get(3, self._estimator().thetaN())

    def getFinalNBestHypotheses(self):
        self._estimator(); K.check(lib().dsr_doa_stream_final_nbest(self._h))

    def initAccs(self):
        self._estimator(); K.check(lib().dsr_doa_stream_init_accs(self._h))

    def reset(self):
        self._estimator(); FeatureStreamPtr.reset(self)

    def next(self, frameX=-5):
        self._estimator()
        return FeatureStreamPtr.next(self, frameX)

    __next__ = next

    def __iter__(self):
        self.reset(); return self


class _Spherical(FeatureStreamPtr):
    """the spherical-array family (modalBeamformer.{h,cc}) over one dsr_sph handle, made at the first frame once the channels are known;
    settings made before that are replayed on it"""
    _KIND, _DOA = "EB", False

    def __init__(self, nBest, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm):
        if halfBandShift:
            raise K.DsrError(K.E_PARAMETER, "_halfBandShift == true is not implemented yet")        # modalBeamformer.cc:391-394
        self._args = (nBest, sampleRate, fftLen, NC, maxOrder, normalizeWeight)
        self._fftLen, self._maxOrder, self._nBest, self._nm = fftLen, maxOrder, nBest, nm
        self._chans = []; self._sph = None; self._set = []; FeatureStreamPtr.__init__(self, None)

    def _handle(self):
        if self._sph is None:
            nBest, fs, M, NC, mo, nw = self._args
            self._sph = (K.SphDoaSRP if self._DOA else K._Sph)(self._KIND, nBest, fs, M, len(self._chans), mo, nw, False, NC)
            for fn, args in self._set:
                getattr(self._sph, fn)(*args)
            create = lib().dsr_sph_doa_stream_create if self._DOA else lib().dsr_sph_bf_stream_create
            h, _ = _new(create, self._sph.h, self._nm.encode()); self._h = h
            for c in self._chans:
                K.check(lib().dsr_subband_bf_set_channel(self._h, c._h))
        return self._sph

    def _query(self):
        """the handle for the geometry getters: before setChannel (the reference allows them once a geometry is set) a throw-away handle over
        as many channels as the last geometry has sensors, with the settings so far; without a geometry its getters fail with DSR_E_ERROR"""
        if self._sph is not None or self._chans:
            return self._handle()
        n = 1
        for fn, args in self._set:
            if fn == "setEigenMikeGeometry":
                n = 32
            elif fn == "setArrayGeometry":
                n = len(args[1])
        nBest, fs, M, NC, mo, nw = self._args
        q = K._Sph(self._KIND, nBest, fs, M, n, mo, nw, False, NC)
        for fn, args in self._set:
            if hasattr(q, fn):
                getattr(q, fn)(*args)
        return q

    def _apply(self, fn, *args):
        if self._sph is None:
            self._set.append((fn, args))
        else:
            getattr(self._sph, fn)(*args)

    def setChannel(self, chan):
        if self._sph is not None:
            raise K.DsrError(5, "channels must be set before the first frame")
        self._chans.append(chan)

    def chanN(self):
        return len(self._chans)

    def dim(self):
        return self._maxOrder * self._maxOrder

    def setEigenMikeGeometry(self):
        self._apply("setEigenMikeGeometry")

    def setArrayGeometry(self, a, theta_s, phi_s):
        self._apply("setArrayGeometry", float(a), np.array(theta_s, np.float64), np.array(phi_s, np.float64))

    def setLookDirection(self, theta, phi):
        self._apply("setLookDirection", float(theta), float(phi))

    def setSigma2(self, sigma2):
        self._apply("setSigma2", sigma2)

    def setWeightGain(self, wgain):
        self._apply("setWeightGain", wgain)

    def getModeAmplitudes(self):
        return self._query().modeAmplitudes()

    def getBeamPattern(self, fbinX, theta=0.0, phi=0.0, minTheta=-np.pi, maxTheta=np.pi, minPhi=-np.pi, maxPhi=np.pi, widthTheta=0.1, widthPhi=0.1):
        """beamformer.i:434-436, :756-758: [nTheta][nPhi]; it sets the look direction to (theta, phi) as the reference does"""
        q = self._query()
        self._lookSet = True                                                                # (the GSC classes' setActiveWeights_f asks for it)
        if self._sph is None:
            self._set.append(("setLookDirection", (float(theta), float(phi))))
        return q.getBeamPattern(fbinX, theta, phi, minTheta, maxTheta, minPhi, maxPhi, widthTheta, widthPhi)

    def getArrayGeometry(self, type):
        return self._query().getArrayGeometry(type)

    def getSnapShotArray(self):
        """the current frame's eigenbeams [fftLen/2+1][dim] (the reference's _sphericalTransformSnapShotArray)"""
        self._handle(); D = self.dim(); out = np.zeros((self._fftLen // 2 + 1) * D * 2, np.float64); got = C.c_size_t()
        K.check(lib().dsr_sph_stream_get_eigenbeams(self._h, K._ptr(out), out.size, C.byref(got)))
        return out.view(np.complex128).reshape(self._fftLen // 2 + 1, D)

    def reset(self):
        self._handle(); FeatureStreamPtr.reset(self)

    def next(self, frameX=-5):
        self._handle()
        return FeatureStreamPtr.next(self, frameX)

    __next__ = next

    def __iter__(self):
        self.reset(); return self


class EigenBeamformerPtr(_Spherical):
    """beamformer.i:416-455 (EigenBeamformer, modalBeamformer.cc:219-399): the phase-mode (HMDI) beamformer in the eigenbeam domain"""

    def __init__(self, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=8, normalizeWeight=False, nm="EigenBeamformer"):
        _Spherical.__init__(self, 1, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)


class SphericalDSBeamformerPtr(_Spherical):
    """beamformer.i:551-575 (SphericalDSBeamformer, modalBeamformer.cc:990-1091): delay-and-sum modal weights"""
    _KIND = "DS"

    def __init__(self, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=3, normalizeWeight=False, nm="SphericalDSBeamformer"):
        _Spherical.__init__(self, 1, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)

    def calcWNG(self):
        return self._query().calcWNG()


class SphericalHWNCBeamformerPtr(_Spherical):
    """beamformer.i:648-660 (SphericalHWNCBeamformer, modalBeamformer.cc:1387-1478): HMDI weights held to a white noise gain"""
    _KIND = "HWNC"

    def __init__(self, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=3, normalizeWeight=False, ratio=0.1, nm="SphericalHWNCBeamformer"):
        _Spherical.__init__(self, 1, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)
        self._apply("setWNG", ratio)

    def setWNG(self, ratio):
        self._apply("setWNG", ratio)

    def calcWNG(self):
        return self._query().calcWNG()


class _SphericalGSC(_Spherical):
    def setLookDirection(self, theta, phi):
        self._lookSet = True; _Spherical.setLookDirection(self, theta, phi)

    def setActiveWeights_f(self, fbinX, packedWeight):
        if self._sph is None and not getattr(self, "_lookSet", False):
            raise K.DsrError(1, "call setLookDirection() once")                             # modalBeamformer.cc:1588-1591
        self._apply("setActiveWeights_f", int(fbinX), np.array(packedWeight, np.float64))


class SphericalGSCBeamformerPtr(_SphericalGSC):
    """beamformer.i:677-689 (SphericalGSCBeamformer, modalBeamformer.cc:1483-1594): the modal GSC, active weights set from outside"""
    _KIND = "GSC"

    def __init__(self, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=4, normalizeWeight=False, nm="SphericalGSCBeamformer"):
        _Spherical.__init__(self, 1, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)

    def calcWNG(self):
        return self._query().calcWNG()


class SphericalHWNCGSCBeamformerPtr(_SphericalGSC):
    """beamformer.i:706-718 (SphericalHWNCGSCBeamformer, modalBeamformer.cc:1599-1713): the GSC over the HWNC quiescent weights"""
    _KIND = "HWNCGSC"

    def __init__(self, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=4, normalizeWeight=False, ratio=1.0, nm="SphericalHWNCGSCBeamformer"):
        _Spherical.__init__(self, 1, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)
        self._apply("setWNG", ratio)

    def setWNG(self, ratio):
        self._apply("setWNG", ratio)

    def calcWNG(self):
        return self._query().calcWNG()


class SphericalMOENBeamformerPtr(_Spherical):
    """beamformer.i:761-773 (SphericalMOENBeamformer, modalBeamformer.cc:1804-2099): the Li / Duraiswami optimal design in the sensor domain"""
    _KIND = "MOEN"

    def __init__(self, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=4, normalizeWeight=False, nm="SphericalMOENBeamformer"):
        _Spherical.__init__(self, 1, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)

    def setLevelOfDiagonalLoading(self, fbinX, diagonalWeight):
        self._apply("setLevelOfDiagonalLoading", int(fbinX), float(diagonalWeight))

    def fixTerms(self, flag):
        self._apply("fixTerms", bool(flag))

    def calcWNG(self):
        return self._query().calcWNG()


class SphericalSpatialDSBeamformerPtr(_Spherical):
    """beamformer.i:994-1006 (SphericalSpatialDSBeamformer, modalBeamformer.cc:2106-2270): delay-and-sum in the sensor domain"""
    _KIND = "SPATIALDS"

    def __init__(self, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=3, normalizeWeight=False, nm="SphericalSpatialDSBeamformer"):
        _Spherical.__init__(self, 1, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)

    def calcWNG(self):
        return self._query().calcWNG()


class _SphericalDOA(_Spherical):
    _DOA = True

    def setSearchParam(self, minTheta=0.0, maxTheta=np.pi, minPhi=-np.pi, maxPhi=np.pi, widthTheta=0.1, widthPhi=0.1):
        self._apply("setSearchParam", minTheta, maxTheta, minPhi, maxPhi, widthTheta, widthPhi)

    def setFrequencyRange(self, fbinMin, fbinMax):
        self._apply("setFrequencyRange", fbinMin, fbinMax)

    def setEnergyThreshold(self, engeryThreshold):
        self._apply("setEnergyThreshold", engeryThreshold)

    def _get(self, what, n):
        self._handle()
        out = np.zeros(max(n, 1), np.float64); got = C.c_size_t()
        K.check(lib().dsr_sph_doa_stream_get(self._h, what, K._ptr(out), out.size, C.byref(got)))
        return out[:got.value]

    def getNBestRPs(self):
        return self._get(0, self._nBest)

    def getNBestDOAs(self):
        """[nBest][2]: (theta, phi) of each rank"""
        return self._get(1, 2 * self._nBest).reshape(self._nBest, 2)

    def getEnergy(self):
        return float(np.float32(self._get(4, 1)[0]))

    def getResponsePowerMatrix(self):
        """[nTheta][nPhi]: the last ungated frame's response powers (the accumulators after getFinalNBestHypotheses); None before the first frame"""
        nT, nP = self._handle().gridN()
        v = self._get(2, nT * nP)
        return v.reshape(nT, nP) if v.size else None

    def getAccumulators(self):
        return self._get(3, self._handle().units())

    def getFinalNBestHypotheses(self):
        self._handle(); K.check(lib().dsr_sph_doa_stream_final_nbest(self._h))

    def initAccs(self):
        self._handle(); K.check(lib().dsr_sph_doa_stream_init_accs(self._h))


class DOAEstimatorSRPEBPtr(_SphericalDOA):
    """beamformer.i:515-550 (DOAEstimatorSRPEB, modalBeamformer.cc:762-988): 2-D SRP over (theta, phi) with EigenBeamformer weights.  The
    constructor searches (-pi, pi) x (-pi, pi) by 0.25; setSearchParam() without arguments (0, pi, -pi, pi, 0.1, 0.1)."""

    def __init__(self, nBest, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=8, normalizeWeight=False, nm="DirectionEstimatorSRPMB"):
        _Spherical.__init__(self, nBest, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)


class DOAEstimatorSRPSphDSBPtr(_SphericalDOA):
    """beamformer.i:601-633 (DOAEstimatorSRPSphDSB, modalBeamformer.cc:1170-1385): 2-D SRP with SphericalDSBeamformer weights.  The defaults
    are those of the Python constructor (%extend, beamformer.i:624): maxOrder 8, name "DirectionEstimatorSRPMB"."""
    _KIND = "DS"

    def __init__(self, nBest, sampleRate, fftLen=512, halfBandShift=False, NC=1, maxOrder=8, normalizeWeight=False, nm="DirectionEstimatorSRPMB"):
        _Spherical.__init__(self, nBest, sampleRate, fftLen, halfBandShift, NC, maxOrder, normalizeWeight, nm)


class _Decomposition(object):
    """ModalDecompositionPtr / SpatialDecompositionPtr(orderN, subbandsN, a, sampleRate, useSubbandsN=0) (beamformer.i:820-872): the arguments and
    the host-side tables; the tracker built on it makes the handle that also holds the tracker's parameters"""
    _KIND = "modal"

    def __init__(self, orderN, subbandsN, a, sampleRate, useSubbandsN=0):
        self._args = (int(orderN), int(subbandsN), float(a), float(sampleRate), int(useSubbandsN))
        self._trk = K.SphTracker(self._KIND, orderN, subbandsN, a, sampleRate, 1)      # the tables only: the tracker's handle checks the observation's length

    def orderN(self):
        return self._args[0]

    def modesN(self):
        return self._trk.modesN

    def subbandsN(self):
        return self._args[1]

    def subbandsN2(self):
        return self._args[1] // 2

    def useSubbandsN(self):
        return self._args[4] or self._args[1] // 2 + 1

    def subbandLengthN(self):
        return self._trk.L

    def reset(self):
        pass

    def modalCoefficient(self, order, subbandX):
        return self._trk.bn()[subbandX, order]

    def harmonic(self, order, degree, *at):
        """harmonic(order, degree, theta, phi), or harmonic(order, degree, channelX): the stored (conjugated) harmonic of a sensor"""
        if len(at) == 1:
            return self._trk.sensorHarmonics()[order * order + order + degree, at[0]]
        return K.SphTracker.harmonic(order, degree, *at)

    harmonicDerivPolarAngle = staticmethod(K.SphTracker.harmonicDerivPolarAngle)
    harmonicDerivAzimuth = staticmethod(K.SphTracker.harmonicDerivAzimuth)


class ModalDecompositionPtr(_Decomposition):
    _KIND = "modal"


class SpatialDecompositionPtr(_Decomposition):
    _KIND = "spatial"


class _SphericalArrayTracker(FeatureStreamPtr):
    """Modal / SpatialSphericalArrayTrackerPtr(decomposition, sigma2_u=10.0, sigma2_v=10.0, sigma2_init=10.0, maxLocalN=1, nm) (beamformer.i:874-948):
    a stream of float (theta, phi) over the 32 channels given by setChannel"""
    _KIND, _NAME = "modal", "ModalSphericalArrayTracker"

    def __init__(self, decomposition, sigma2_u=10.0, sigma2_v=10.0, sigma2_init=10.0, maxLocalN=1, nm=None):
        if decomposition._KIND != self._KIND:
            raise K.DsrError(K.E_PARAMETER, "%s needs a %s decomposition" % (self._NAME, self._KIND))
        o, M, a, fs, use = decomposition._args
        self._dec = decomposition
        self._trk = K.SphTracker(self._KIND, o, M, a, fs, use, sigma2_u, sigma2_v, sigma2_init, maxLocalN)
        self._chans = []
        h, _ = _new(lib().dsr_trk_stream_create, self._trk.h, (nm or self._NAME).encode())
        FeatureStreamPtr.__init__(self, h)

    def setChannel(self, chan):
        K.check(lib().dsr_trk_stream_set_channel(self._h, chan._h)); self._chans.append(chan)

    def chanN(self):
        return len(self._chans)

    def setV(self, Vk, subbandX):
        self._trk.setV(Vk, subbandX)

    def setInitialPosition(self, theta, phi):
        K.check(lib().dsr_trk_stream_set_initial_position(self._h, float(theta), float(phi)))

    def nextSpeaker(self):
        K.check(lib().dsr_trk_stream_next_speaker(self._h))


class ModalSphericalArrayTrackerPtr(_SphericalArrayTracker):
    _KIND, _NAME = "modal", "ModalSphericalArrayTracker"


class SpatialSphericalArrayTrackerPtr(_SphericalArrayTracker):
    _KIND, _NAME = "spatial", "SpatialSphericalArrayTracker"


class PlaneWaveSimulatorPtr(FeatureStreamPtr):
    """PlaneWaveSimulatorPtr(source, modalDecomposition, channelX, theta, phi, nm="Plane Wave Simulator") (beamformer.i:950-977)"""

    def __init__(self, source, modalDecomposition, channelX, theta, phi, nm="Plane Wave Simulator"):
        h, _ = _new(lib().dsr_pws_stream_create, source._h, modalDecomposition._trk.h, int(channelX), float(theta), float(phi), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(source, modalDecomposition))
