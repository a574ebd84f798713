"""btk.lib.mkBeamforming: MEKSubbandBeamformer_pr / MEKSubbandBeamformer_nrm (btk/lib/mkBeamforming.py:398-658) under the reference's method
names, over dsr._capi.MkBeamformer.  The observations of an utterance go to the device once (accumObservations); estimateActiveWeights(fbinX, ...)
runs one bin's minimiser on the device, estimateAllActiveWeights() every bin in one launch.  NC = 1, one source, no halfBandShift."""
import numpy as np

from .. import _capi as K


class MKSubbandBeamformer(object):
    _KIND = K.MK_PR

    def __init__(self, spectralSources, NC, alpha, halfBandShift):
        self._nSource = 1
        self._spectralSources = spectralSources
        if hasattr(spectralSources, "shape"):                        # an array [C][T][fftLen/2+1 or fftLen] instead of a list of filter banks
            self._nChan = int(spectralSources.shape[0]); F = int(spectralSources.shape[2])
            self._fftLen = 2 * (F - 1) if F % 2 else F
        else:
            self._nChan = len(spectralSources); self._fftLen = int(spectralSources[0].fftLen())
        self._NC, self._alpha, self._halfBandShift = NC, alpha, halfBandShift
        self._mk = K.MkBeamformer(self._fftLen, self._nChan, self._KIND, alpha, getattr(self, "_beta", 3.0), getattr(self, "_gamma", -1.0),
                                  NC=NC, nSource=self._nSource, halfBandShift=halfBandShift)      # refuses NC != 1 and halfBandShift
        self._F = self._fftLen // 2 + 1
        self._X = None; self._sel = (0, 0, 1); self._nSel = 0; self._info = None
        self._haveFixed = False

    def nextSpkr(self):
        self._X = None; self._nSel = 0; self._haveFixed = False
        self._mk = K.MkBeamformer(self._fftLen, self._nChan, self._KIND, self._alpha, self._beta, getattr(self, "_gamma", -1.0))

    # ---- observations
    def accumObservations(self, sFrame, eFrame, R=1):
        """reads frames 0 .. eFrame-1 (or to the end of the sources) and keeps sFrame <= s < eFrame with s % R == 0 -> [frameN][fftLen/2+1][chanN]"""
        import torch
        R = max(int(R), 1)
        src = self._spectralSources
        if hasattr(src, "shape"):
            X = torch.as_tensor(src)[:, :eFrame, :self._F]
        else:
            rows = []
            try:
                for _ in range(eFrame):
                    rows.append([np.array(fb.next(), np.complex128)[:self._F] for fb in src])
            except (StopIteration, K.DsrError):
                pass
            for fb in src:
                fb.reset()
            X = torch.from_numpy(np.array(rows, np.complex64).reshape(len(rows), self._nChan, self._F).transpose(1, 0, 2).copy())
        self._X = X.to(device="cuda", dtype=torch.complex64)[None].contiguous()
        T = self._X.shape[2]
        sel = [s for s in range(max(sFrame, 0), min(eFrame, T)) if s % R == 0]
        self._sel = (sFrame, eFrame, R); self._nSel = len(sel)
        return self._X[0][:, sel, :].permute(1, 2, 0).cpu().numpy()

    def _observations(self):
        if self._X is None:
            raise K.DsrError(1, "Zero observation! Call getObservations() first!")
        s, e, R = self._sel
        return self._X, dict(sFrame=s, eFrame=e, R=R)

    def calcCov(self):
        """-> SigmaX [fftLen/2+1][chanN][chanN]: the mean of x x^H over the accumulated frames"""
        X, kw = self._observations()
        if self._nSel == 0:
            raise K.DsrError(1, "Zero observation! Call getObservations() first!")
        sel = [s for s in range(max(kw["sFrame"], 0), min(kw["eFrame"], X.shape[2])) if s % kw["R"] == 0]
        x = X[0][:, sel, :].cpu().numpy().astype(np.complex128)      # [C][T][F]
        self._SigmaX = np.einsum("ctf,dtf->fcd", x, np.conj(x)) / len(sel)
        return self._SigmaX

    # ---- getters
    def getSourceN(self):
        return self._nSource

    def getChanN(self):
        return self._nChan

    def getSampleN(self):
        return self._nSel

    def getFftLen(self):
        return self._fftLen

    def getWq(self, srcX, fbinX):
        return self._mk.getFixedWeights()[0][fbinX]

    def getB(self, srcX, fbinX):
        return self._mk.getFixedWeights()[1][fbinX]

    def getAlpha(self):
        return self._alpha

    # ---- fixed weights
    def setFixedWeights(self, wq, updateBlockingMatrix=False, norm=1):
        """wq[srcX][fbinX][chanX]; the blocking matrices are recalculated with updateBlockingMatrix, kept otherwise"""
        w = np.array([np.asarray(wq[0][f], np.complex128) / norm for f in range(self._F)])
        if not updateBlockingMatrix and not self._haveFixed:
            raise K.DsrError(1, "no blocking matrices yet: call calcFixedWeights() or setFixedWeights(wq, True) once")
        self._mk.setFixedWeights(w, None if updateBlockingMatrix else self._mk.getFixedWeights()[1])
        self._haveFixed = True

    def calcFixedWeights(self, sampleRate, delays):
        """delays[nSource][nChan]: the array manifold vectors as quiescent vectors and their blocking matrices (SubbandGSC's calcGSCWeights)"""
        bf = K.Beamformer(self._fftLen, self._nChan)
        bf.calcGSCWeights(sampleRate, np.asarray(delays, np.float64).reshape(-1, self._nChan)[0])
        self._mk.setFixedWeightsFromBeamformer(bf)
        self._haveFixed = True

    def UnpackWeights(self, waAs):
        waAs = np.asarray(waAs, np.float64); n = self._nChan - self._NC
        return [waAs[2 * n * s:2 * n * (s + 1):2] + 1j * waAs[2 * n * s + 1:2 * n * (s + 1):2] for s in range(self._nSource)]


class MEKSubbandBeamformer_pr(MKSubbandBeamformer):
    _KIND = K.MK_PR
    _DIFF = 1.0e-5

    def __init__(self, spectralSources, NC=1, alpha=1.0e-2, beta=3.0, halfBandShift=False):
        self._beta = beta
        MKSubbandBeamformer.__init__(self, spectralSources, NC, alpha, halfBandShift)
        self.resetStatistics()

    def resetStatistics(self):
        self._stats = None                                           # [3][1][F] on the device from the first use on: prevAvgY2, prevAvgY4, prevFrameN

    def _carried(self):
        import torch
        if self._stats is None:
            self._stats = torch.zeros((3, 1, self._F), dtype=torch.float64, device="cuda")
        return self._stats

    def normalizeWeight(self, srcX, fbinX, wa):
        return wa

    def normalizeWa(self, fbinX, wa):
        return [self.normalizeWeight(s, fbinX, wa[s]) for s in range(self._nSource)]

    def _full(self, fbinX, wa):
        w = np.zeros((1, self._F, self._nChan - 1), np.complex128); w[0, fbinX] = wa
        return w

    def calcKurtosis(self, srcX, fbinX, wa_f):
        """E|Y|^4 - beta (E|Y|^2)^2 at the active weights wa_f[srcX] of bin fbinX, carried statistics included"""
        X, kw = self._observations()
        wa = np.asarray(wa_f[srcX], np.complex128)
        cost, _ = self._mk.eval(X, self._full(fbinX, wa), stats=self._carried(), fbinX=fbinX, **kw)
        wn = self.normalizeWeight(srcX, fbinX, wa)
        return float(self._alpha * np.sum(np.abs(wn) ** 2) - cost[0, fbinX].item())

    def gradient(self, srcX, fbinX, wa_f):
        """the derivative of the kurtosis with respect to conj(wa) -> [chanN - NC] complex"""
        X, kw = self._observations()
        wa = np.asarray(wa_f[srcX], np.complex128)
        _, g = self._mk.eval(X, self._full(fbinX, wa), stats=self._carried(), fbinX=fbinX, **kw)
        g = g[0, fbinX].cpu().numpy()
        return -((g[0::2] + 1j * g[1::2]) - self._alpha * self.normalizeWeight(srcX, fbinX, wa))

    def _run(self, fbinX, start, MAXITNS, TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE):
        X, kw = self._observations()
        self._mk.minimizer(MAXITNS, TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE)
        wa, info, cost = self._mk.estimate(X, start, stats=self._carried(), fbinX=fbinX, **kw)
        self._info = (info[0].cpu().numpy(), cost[0].cpu().numpy())
        w = wa[0].cpu().numpy()
        packed = np.zeros((self._F, 2 * (self._nChan - 1))); packed[:, 0::2] = w.real; packed[:, 1::2] = w.imag
        return packed

    def estimateActiveWeights(self, fbinX, startpoint, MAXITNS=40, TOLERANCE=1.0E-03, STOPTOLERANCE=1.0E-02, DIFFSTOPTOLERANCE=None, STEPSIZE=0.01):
        """-> the packed active weight vector of bin fbinX"""
        if fbinX < 0 or fbinX > self._fftLen // 2:
            raise K.DsrError(6, "fbinX %d > fftLen/2 %d?" % (fbinX, self._fftLen // 2))
        sp = np.asarray(startpoint, np.float64)
        start = self._full(fbinX, sp[0::2] + 1j * sp[1::2])
        return self._run(fbinX, start, MAXITNS, TOLERANCE, STOPTOLERANCE, self._DIFF if DIFFSTOPTOLERANCE is None else DIFFSTOPTOLERANCE, STEPSIZE)[fbinX]

    def estimateAllActiveWeights(self, startpoints=None, MAXITNS=40, TOLERANCE=1.0E-03, STOPTOLERANCE=1.0E-02, DIFFSTOPTOLERANCE=None, STEPSIZE=0.01):
        """every bin in one launch; startpoints [fftLen/2+1][2 (chanN - NC)] packed (None: zero) -> the packed vectors, same shape"""
        start = None
        if startpoints is not None:
            sp = np.asarray(startpoints, np.float64).reshape(self._F, -1)
            start = (sp[:, 0::2] + 1j * sp[:, 1::2])[None]
        return self._run(-1, start, MAXITNS, TOLERANCE, STOPTOLERANCE, self._DIFF if DIFFSTOPTOLERANCE is None else DIFFSTOPTOLERANCE, STEPSIZE)

    def lastInfo(self):
        """(info [F][4]: iterations, evaluations, failed trials, exit reason; final cost [F]) of the last estimate"""
        return self._info


class MEKSubbandBeamformer_nrm(MEKSubbandBeamformer_pr):
    _KIND = K.MK_NRM
    _DIFF = 1.0e-10

    def __init__(self, spectralSources, NC=1, alpha=0.1, beta=3.0, gamma=-1.0, halfBandShift=False):
        self._gamma = gamma
        MEKSubbandBeamformer_pr.__init__(self, spectralSources, NC, alpha, beta, halfBandShift)

    def normalizeWeight(self, srcX, fbinX, wa):
        wa = np.asarray(wa, np.complex128)
        nrm_wa = np.sqrt(np.sum(np.abs(wa) ** 2))
        gamma = np.sqrt(np.sum(np.abs(self.getWq(srcX, fbinX)) ** 2)) if self._gamma < 0 else self._gamma
        return abs(gamma) * wa / nrm_wa if nrm_wa > abs(gamma) else wa
