"""btk.lib.subbandBeamforming: SubbandBeamformerDS / GSC / GriffithsJim / MVDR / MPDR and the helpers they are set up with
(btk/lib/subbandBeamforming.py:227-676, :982-1265) under the reference's names and signatures, over dsr._abf.AdaptiveBeamformer.

Sources are a list of analysis banks or an array [C][T][fftLen/2+1 or fftLen], as in dsr.btk.mkBeamforming.  An iteration reads the sources to
their end, runs the whole utterance on the device in one call and yields one full fftLen vector per frame: bins 0..fftLen/2 come from the device,
the upper half is their conjugate mirror (the reference's MPDR computes all fftLen bins independently; its upper half equals the mirror up to
rounding).  Iterating again without nextSpkr() continues from the state the last iteration left, as the reference object does.  nextSpkr() starts
a new speaker: state, frame counter and post-filter position (the reference's Griffiths-Jim keeps its frame counter there; this one does not).

One constraint (the static GSC: also two), no halfBandShift: anything else is refused with the consistency error.  SubbandBeamformerMVDR and
SubbandBeamformerMPDR keep the reference's default halfBandShift=True and refuse it: pass halfBandShift=False.
Not built: SubbandBeamformerRLS, SubbandBeamformerCovarSqRoot, SubbandBeamformerInfoSqRoot."""
import copy
import pickle

import numpy as np

from .. import _abf as A
from .._capi._core import DsrError, E_CONSISTENCY


def calcDelays(x, y, z, mpos):
    """:227-246"""
    mpos = np.asarray(mpos, np.float64); chanN = len(mpos)
    delays = np.array([np.sqrt((x - mpos[i, 0]) ** 2 + (y - mpos[i, 1]) ** 2 + (z - mpos[i, 2]) ** 2) / 343740.0 for i in range(chanN)], np.float64)
    return delays - delays[chanN // 2]


def calcBlockingMatrix(vs, NC=1):
    return A.blocking_matrix(vs, NC)


def calcNullBeamformer(w_t, w_j, NC):
    return A.null_beamformer(w_t, w_j, NC)


def calcArrayManifold_f(fbinX, fftLen, chanN, sampleRate, delays, halfBandShift):
    return A.manifold(fbinX, fftLen, chanN, sampleRate, delays, halfBandShift, True)


def calcArrayManifoldWoNorm_f(fbinX, fftLen, chanN, sampleRate, delays, halfBandShift):
    return A.manifold(fbinX, fftLen, chanN, sampleRate, delays, halfBandShift, False)


class SubbandBeamformerDS(object):
    _KIND = "ds"

    def __init__(self, spectralSources, halfBandShift=False, NC=1, **params):
        self._spectralSources = spectralSources
        if hasattr(spectralSources, "shape"):
            self._nChan = int(spectralSources.shape[0]); F = int(spectralSources.shape[2])
            self._fftLen = 2 * (F - 1) if F % 2 else F
        else:
            self._nChan = len(spectralSources); self._fftLen = int(spectralSources[0].fftLen())
        self._fftLen2 = self._fftLen // 2; self._F = self._fftLen2 + 1
        self._halfBandShift, self._NC = halfBandShift, NC
        self._bf = A.AdaptiveBeamformer(self._KIND, self._fftLen, self._nChan, NC, halfBandShift, **params)   # refuses halfBandShift and other NC
        self._bf.carry(True)
        self._wp = []; self._isamp = 0; self._dirty = True
        self._arrayManifold = None; self._blockingMatrix = None; self._w = None

    def size(self):
        return self._fftLen

    def reset(self):
        if not hasattr(self._spectralSources, "shape"):
            for source in self._spectralSources:
                source.reset()

    # ---- set-up
    def calcArrayManifoldVectors(self, sampleRate, delays, normalize=True):
        self._arrayManifold = [A.manifold(f, self._fftLen, self._nChan, sampleRate, delays, self._halfBandShift, normalize) for f in range(self._fftLen)]
        self._dirty = True
        return self._arrayManifold

    def setWp(self, wp):
        for frameX in range(len(wp)):
            self._wp.append(wp[frameX])

    def loadWq(self, fileName):
        with open(fileName, "rb") as fp:
            self._arrayManifold = copy.deepcopy(pickle.load(fp))
        self._dirty = True

    def saveWeights(self, fileName):
        with open(fileName, "wb") as fp:
            pickle.dump(self._weights(), fp, 1)

    def _weights(self):
        if self._w is None:
            raise DsrError(1, "no weights yet: iterate first")
        return [self._w[f].copy() for f in range(self._F)]

    def nextSpkr(self):
        self._isamp = 0; self._w = None
        self._bf.reset()

    # ---- an utterance
    def _upload(self):
        if self._arrayManifold is None:
            raise DsrError(1, "call calcArrayManifoldVectors() once")
        if self._dirty:
            B = None if self._blockingMatrix is None else np.array(self._blockingMatrix[:self._F])
            self._bf.setFixedWeights(np.array(self._arrayManifold[:self._F]), B)
            self._dirty = False

    def _read(self):
        """-> the utterance's snapshots, numpy complex64 [C][T][F]"""
        src = self._spectralSources
        if hasattr(src, "shape"):
            return np.ascontiguousarray(np.asarray(src)[:, :, :self._F], np.complex64)
        rows = []
        try:
            while True:
                rows.append([np.array(fb.next(), np.complex128)[:self._F] for fb in src])
        except (StopIteration, DsrError):
            pass
        return np.ascontiguousarray(np.array(rows, np.complex64).reshape(len(rows), self._nChan, self._F).transpose(1, 0, 2))

    def _post_filter(self, T):
        """-> (wp [1][T][F] float32, rows of it that apply) for the frames isamp .. isamp + T - 1; (None, 0) without"""
        rows = self._wp[self._isamp:self._isamp + T]
        if not len(rows):
            return None, 0
        wp = np.ones((1, T, self._F), np.float32)
        wp[0, :len(rows)] = np.real(np.array([np.asarray(r)[:self._F] for r in rows]))
        return wp, len(rows)

    def __iter__(self):
        import torch
        X = self._read(); T = X.shape[1]
        self._upload()
        wp, nwp = self._post_filter(T)
        if T == 0:
            return
        dev = torch.device("cuda")
        kw = {}
        if nwp or wp is not None:
            kw = dict(wp=torch.from_numpy(wp).to(dev), wpFrames=torch.tensor([nwp], dtype=torch.int32, device=dev))
        Y, w = self._bf.run(torch.from_numpy(X)[None].to(dev), **kw)
        if w is not None:
            self._w = w[0].cpu().numpy()
        self._isamp += T
        Yh = Y[0].cpu().numpy().astype(np.complex128)
        for t in range(T):
            out = np.zeros(self._fftLen, np.complex128)
            out[:self._F] = Yh[t]; out[self._F:] = np.conj(Yh[t][1:self._F - 1][::-1])
            yield out


class SubbandBeamformerGSC(SubbandBeamformerDS):
    _KIND = "gsc"

    def __init__(self, spectralSources, halfBandShift=False, NC=1, **params):
        SubbandBeamformerDS.__init__(self, spectralSources, halfBandShift, NC, **params)
        self._waHK = [np.zeros(self._nChan - NC, np.complex128) for _ in range(self._fftLen)]

    def calcArrayManifoldVectors(self, sampleRate, delays):
        SubbandBeamformerDS.calcArrayManifoldVectors(self, sampleRate, delays)
        self.calcBlockingMatrix()

    def calcArrayManifoldVectors2(self, sampleRate, delays1, delays2):
        self._arrayManifold = []
        for fbinX in range(self._fftLen):
            wds1 = calcArrayManifoldWoNorm_f(fbinX, self._fftLen, self._nChan, sampleRate, delays1, self._halfBandShift)
            wds2 = calcArrayManifoldWoNorm_f(fbinX, self._fftLen, self._nChan, sampleRate, delays2, self._halfBandShift)
            self._arrayManifold.append(calcNullBeamformer(wds1, wds2, self._NC))
        self.calcBlockingMatrix()

    def calcBlockingMatrix(self):
        self._blockingMatrix = [calcBlockingMatrix(vs, self._NC) for vs in self._arrayManifold]
        self._dirty = True

    def setWa(self, waHK):
        Len = self._nChan - self._NC
        if len(waHK[0]) != Len:
            raise ValueError("The length of an adaptive filter must be not %d but %d" % (len(waHK[0]), Len))
        for fbinX in range(self._fftLen):
            self._waHK[fbinX] = np.array(waHK[fbinX], np.complex128)

    def loadWeights(self, fileName):
        with open(fileName, "rb") as fp:
            w = pickle.load(fp)
        self._waHK = [np.array(v, np.complex128) for v in w] + [np.zeros(self._nChan - self._NC, np.complex128)] * (self._fftLen - len(w))

    def _weights(self):
        return self._waHK if self._KIND == "gsc" else SubbandBeamformerDS._weights(self)

    def _upload(self):
        SubbandBeamformerDS._upload(self)
        if self._KIND == "gsc":
            self._bf.setActiveWeights(np.array(self._waHK[:self._F]))


class SubbandBeamformerGriffithsJim(SubbandBeamformerGSC):
    _KIND = "gj"

    def __init__(self, spectralSources, beta=0.999, gamma=0.0005, initDiagLoad=1.0E+10, floorSubBandSigmaK=2.0E+7, silThresh=1.0E+10, alpha2=0.001,
                 plotting=False, staticAfter=1000, halfBandShift=False):
        SubbandBeamformerGSC.__init__(self, spectralSources, halfBandShift, 1, beta=beta, gamma=gamma, initDiagLoad=initDiagLoad,
                                      floorSubBandSigmaK=floorSubBandSigmaK, silThresh=silThresh, alpha2=alpha2, staticAfter=staticAfter)


class SubbandBeamformerMVDR(SubbandBeamformerDS):
    _KIND = "mvdr"

    def __init__(self, spectralSources, diagLoad=0.001, forgetFactor=0.99, halfBandShift=True, end=20, wp1L=[]):
        SubbandBeamformerDS.__init__(self, spectralSources, halfBandShift, 1, diagLoad=diagLoad, forgetFactor=forgetFactor, end=end)
        self._wp1L = wp1L

    def _post_filter(self, T):
        if len(self._wp1L) == 0:
            return None, 0
        if len(self._wp1L) < self._isamp + T:
            raise DsrError(E_CONSISTENCY, "wp1L holds %d frames, the utterance has %d" % (len(self._wp1L), self._isamp + T))
        rows = self._wp1L[self._isamp:self._isamp + T]
        return np.real(np.array([np.asarray(r)[:self._F] for r in rows])).astype(np.float32)[None], T


class SubbandBeamformerMPDR(SubbandBeamformerGSC):
    _KIND = "mpdr"

    def __init__(self, spectralSources, diagLoad=0.001, forgetFactor=0.99, halfBandShift=True, end=20):
        SubbandBeamformerGSC.__init__(self, spectralSources, halfBandShift, 1, diagLoad=diagLoad, forgetFactor=forgetFactor, end=end)
