"""btk.lib.mnBeamforming: MNSubbandBeamformerGGDc_pr / MNSubbandBeamformerGGDc_nrm (btk/lib/mnBeamforming.py:431-792) under the reference's method
names, over dsr._mn.MnBeamformer and the base of dsr.btk.mkBeamforming (observations, covariance, fixed weights, getters).  ggdL[fbinX] is the
generalised Gaussian model of a bin (dsr.btk.GGDcEst.CGGaussianD; only its shape parameter enters).  normalizeWeight is the identity in both
reference classes, so the two differ in the default beta only and both run conjugate_pr; gamma is accepted and has no effect.  NC = 1, one source,
no halfBandShift; MNSubbandBeamformerGamma is not offered.  Log-file methods are accepted and do nothing."""
import numpy as np

from .. import _mn as M
from .mkBeamforming import MKSubbandBeamformer


class MNSubbandBeamformer(MKSubbandBeamformer):
    def __init__(self, spectralSources, ggdL, nSource, NC, alpha, beta, gamma, halfBandShift):
        if nSource != 1:
            raise M.DsrError(13, "one source only (nSource = %d)" % nSource)
        self._beta, self._gamma, self._ggdL = beta, gamma, ggdL
        MKSubbandBeamformer.__init__(self, spectralSources, NC, alpha, halfBandShift)      # refuses NC != 1 and halfBandShift
        self._wa = {}
        self._newBeamformer()

    def _newBeamformer(self):
        shape = [float(self._ggdL[f].getShapePar()) for f in range(self._F)]
        self._mk = M.MnBeamformer(self._fftLen, self._nChan, shape, self._alpha, self._beta, self._gamma)

    def nextSpkr(self):
        self._X = None; self._nSel = 0; self._haveFixed = False; self._wa = {}
        self._newBeamformer()

    def openLogFile(self, logfilename, fbinXD=None):
        pass

    def closeLogFile(self):
        pass

    def writeLogFile(self, msg):
        pass

    def normalizeWeight(self, srcX, fbinX, wa):
        return wa

    def normalizeWa(self, fbinX, wa_f):
        return [self.normalizeWeight(s, fbinX, wa_f[s]) for s in range(self._nSource)]

    # ---- the objective at the weights of calcEntireWeights_f
    def calcEntireWeights_f(self, fbinX, wa_f):
        self._wa[fbinX] = np.asarray(wa_f[0], np.complex128)

    def calcCovarOutputs_f(self, fbinX):
        pass

    def _full(self, fbinX, wa):
        w = np.zeros((1, self._F, self._nChan - 1), np.complex128); w[0, fbinX] = wa
        return w

    def _eval(self, fbinX, wa):
        X, kw = self._observations()
        cost, g = self._mk.eval(X, self._full(fbinX, wa), fbinX=fbinX, **kw)
        return cost[0, fbinX].item(), g[0, fbinX].cpu().numpy()

    def negentropy(self, srcX, fbinX):
        """H_gaussian - beta H_ggaussian of the beamformer's output at the weights given to calcEntireWeights_f"""
        wa = self._wa[fbinX]
        return float(self._alpha * np.sum(np.abs(wa) ** 2) - self._eval(fbinX, wa)[0])

    def gradient(self, srcX, fbinX):
        """the derivative of the negentropy with respect to conj(wa) -> [chanN - NC] complex"""
        wa = self._wa[fbinX]
        g = self._eval(fbinX, wa)[1]
        return -((g[0::2] + 1j * g[1::2]) - self._alpha * wa)

    def _run(self, fbinX, start, MAXITNS, TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE):
        X, kw = self._observations()
        self._mk.minimizer(MAXITNS, TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE)
        wa, info, cost = self._mk.estimate(X, start, fbinX=fbinX, **kw)
        self._info = (info[0].cpu().numpy(), cost[0].cpu().numpy())
        w = wa[0].cpu().numpy()
        packed = np.zeros((self._F, 2 * (self._nChan - 1))); packed[:, 0::2] = w.real; packed[:, 1::2] = w.imag
        return packed

    def estimateActiveWeights(self, fbinX, startpoint, MAXITNS=40, TOLERANCE=1.0E-03, STOPTOLERANCE=1.0E-02, DIFFSTOPTOLERANCE=1.0E-05, STEPSIZE=0.2):
        """-> the packed active weight vector of bin fbinX"""
        if fbinX < 0 or fbinX > self._fftLen // 2:
            raise M.DsrError(6, "fbinX %d > fftLen/2 %d?" % (fbinX, self._fftLen // 2))
        sp = np.asarray(startpoint, np.float64)
        return self._run(fbinX, self._full(fbinX, sp[0::2] + 1j * sp[1::2]), MAXITNS, TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE)[fbinX]

    def estimateAllActiveWeights(self, startpoints=None, MAXITNS=40, TOLERANCE=1.0E-03, STOPTOLERANCE=1.0E-02, DIFFSTOPTOLERANCE=1.0E-05, STEPSIZE=0.2):
        """every bin in one launch; startpoints [fftLen/2+1][2 (chanN - NC)] packed (None: zero) -> the packed vectors, same shape"""
        start = None
        if startpoints is not None:
            sp = np.asarray(startpoints, np.float64).reshape(self._F, -1)
            start = (sp[:, 0::2] + 1j * sp[:, 1::2])[None]
        return self._run(-1, start, MAXITNS, TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE)

    def lastInfo(self):
        """(info [F][4]: iterations, evaluations, failed trials, exit reason; final cost [F]) of the last estimate"""
        return self._info

    def apply(self, waAll):
        """the beamformer's output [T][F] for the accumulated utterance with the packed active weights waAll [F][2 (chanN - NC)]"""
        X, _ = self._observations()
        sp = np.asarray(waAll, np.float64).reshape(self._F, -1)
        return self._mk.apply(X, (sp[:, 0::2] + 1j * sp[:, 1::2])[None])[0]


class MNSubbandBeamformerGGDc_pr(MNSubbandBeamformer):
    def __init__(self, spectralSources, ggdL, nSource=1, NC=1, alpha=1.0E-02, beta=0.5, gamma=-1.0, halfBandShift=False):
        MNSubbandBeamformer.__init__(self, spectralSources, ggdL, nSource, NC, alpha, beta, gamma, halfBandShift)


class MNSubbandBeamformerGGDc_nrm(MNSubbandBeamformer):
    def __init__(self, spectralSources, ggdL, nSource=1, NC=1, alpha=1.0E-02, beta=1.0, gamma=-1.0, halfBandShift=False):
        MNSubbandBeamformer.__init__(self, spectralSources, ggdL, nSource, NC, alpha, beta, gamma, halfBandShift)


def _packed_eval(x, args):
    fbinX, bf, NC = args
    wa = bf.normalizeWa(fbinX, bf.UnpackWeights(x))
    return bf._eval(fbinX, np.asarray(wa[0], np.complex128))


def fun_MN(x, args):
    """the objective of the minimiser at the packed weights x; args = (fbinX, beamformer, NC)"""
    return _packed_eval(x, args)[0]


def dfun_MN(x, args):
    """its packed gradient"""
    return _packed_eval(x, args)[1]


def fdfun_MN(x, args):
    return _packed_eval(x, args)
