"""btk.lib.GGDcEst: CGGaussianD / MLE4CGGaussianD (btk/lib/GGDcEst.py:24-293) under the reference's method names, over dsr._mn.  The generalised
Gaussian model of a zero-mean complex subband sample: shape p, scaling sa.  acc() of an array of samples runs on the device (dsr_ggd_accumulate);
constants, update and files are host code of the library.  trainGGD() trains every bin of a [U][T][F] tensor at once.  A mean that is not zero is
refused.  readAccs, which cannot run in the reference (float() of a list), does what it evidently means to: a file whose nItr is not 1 is ignored."""
import os

import numpy as np

from .. import _mn as K

LZERO = (-1.0E10)


class CGGaussianD(object):
    def __init__(self, p=0.7, sa=0.0, zeroMean=True, mean=0.0):
        if not zeroMean and mean != 0.0:
            raise K.DsrError(13, "zero-mean models only (mean = %g)" % mean)
        self._zeroMean, self._mean = True, 0.0
        self._sa, self._p = sa, p
        self._B, self._lNF, self._NgConst, self._LlConst = -1, 0.0, 0.0, 0.0
        self._fixed = False

    def fixed(self):
        return self._fixed

    def fixConst(self):
        B, lNF, Ng, Ll = K.ggd_constants(np.array([self._p], np.float64))
        self._B, self._lNF, self._NgConst, self._LlConst = float(B[0]), float(lNF[0]), float(Ng[0]), float(Ll[0])
        self._fixed = True

    def setScalingPar(self, sa):
        self._sa = sa; self._fixed = False

    def getScalingPar(self):
        return self._sa

    def setShapePar(self, p):
        self._p = p; self._fixed = False

    def getShapePar(self):
        return self._p

    def getB(self):
        return self._B

    def getLlConst(self):
        return self._LlConst

    def prob(self, X, sigma=0):
        """the log-likelihood of a sample (or an array of samples)"""
        if not self._fixed:
            raise K.DsrError(1, "call fixConst(self)")
        s = self._sa if sigma == 0 else sigma
        X2 = np.abs(np.asarray(X) - self._mean) ** 2
        with np.errstate(divide="ignore"):
            return self._LlConst - np.log(s) - np.power(X2 / (s * self._B), self._p)

    def entropy(self, sigma):
        if not self._fixed:
            self.fixConst()
        if sigma == 0:
            return LZERO
        return self._NgConst + np.log(sigma)

    def writeParam(self, filename):
        K.ggd_write_param(filename, self._sa, self._p, self._mean)

    def readParam(self, filename, zeroMean=True, fixValues=True):
        if not os.path.exists(filename):
            return False
        self._sa, self._p, mean, self._B, self._lNF = K.ggd_read_param(filename)
        if not zeroMean and mean != 0.0:
            raise K.DsrError(13, "zero-mean models only (mean = %g)" % mean)
        if fixValues:
            self.fixConst()
        self._fixed = True
        return True


class MLE4CGGaussianD(CGGaussianD):
    def __init__(self, p=0.7, sigma=0.0, zeroMean=True, mean=0.0, alpha=0.05):
        CGGaussianD.__init__(self, p, sigma, zeroMean, mean)
        self._alpha, self._nItr, self._thresh, self._floorV, self._floorP, self._converge = alpha, 0, 0.00001, 10e-8, 0.07, False
        self.clearAcc()

    def isConverged(self):
        return self._converge

    def accs(self):
        """(acc1S, acc1P, acc2P, nSample, totalL)"""
        return self._acc.copy()

    def clearAcc(self):
        self._acc = np.zeros(5)

    def writeAccs(self, filename):
        K.ggd_write_accs(filename, self._acc, self._alpha, self._nItr, self._thresh, self._floorV, self._floorP)

    def readAccs(self, filename):
        used = K.ggd_read_accs(filename, self._acc)
        if used:
            self._nItr = 1
        return used

    def acc(self, Xi):
        """one sample (added on the host, as the reference's loop over samples does), or an array / tensor of samples of this model's bin, which
        goes through the device entry as one utterance"""
        if not self._fixed:
            raise K.DsrError(1, "Error: Parameters are not initialized correctly")
        if not (self._sa > 0.0):
            raise K.DsrError(13, "the scaling parameter is %g" % self._sa)
        if np.ndim(Xi) == 0 and not hasattr(Xi, "is_cuda"):
            return self._acc_host(np.asarray([Xi], np.complex64))
        import torch
        x = torch.as_tensor(Xi).to(device="cuda", dtype=torch.complex64).reshape(1, -1, 1)
        self._acc = K.ggd_accumulate(x, [self._p], [self._sa], acc_in=self._acc.reshape(5, 1))[:, 0]

    def _acc_host(self, x):
        """single values: the statistics of the device entry with the library's det functions, one sample at a time"""
        re, im = x.real.astype(np.float64), x.imag.astype(np.float64); v2 = re * re + im * im
        la0 = K.det_log(np.array([self._B * self._sa]))[0]; ll0 = self._LlConst - K.det_log(np.array([self._sa]))[0]
        pos = v2 > 0.0; l = K.det_log(np.where(pos, v2, 1.0)); la = l - la0
        t1 = np.where(pos, K.det_exp(self._p * l), 0.0); tmp = np.where(pos, K.det_exp(self._p * la), 0.0)
        t1P = np.where(v2 > 1.0e-22, tmp * la, 0.0)
        for row, term in ((0, t1), (1, t1P), (2, tmp), (4, ll0 - tmp)):
            self._acc[row] += _tree64(term)
        self._acc[3] += float(len(x))

    def update(self, filename="", sigmaOnly=False):
        if not self._fixed:
            raise K.DsrError(1, "Parameters are not initialized correctly")
        if self._converge:
            return [self._sa, self._p, self._converge]
        sa, p, cv = K.ggd_update(self._acc.reshape(5, 1), [self._p], [self._sa], self._nItr, self._alpha, self._thresh, self._floorV, self._floorP, sigmaOnly)
        self._sa, self._p, self._converge = float(sa[0]), float(p[0]), bool(cv[0])
        self.fixConst()
        if filename != "":
            self.writeParam(filename)
        self.clearAcc(); self._nItr += 1
        return [self._sa, self._p, self._converge]


def _tree64(term):
    """the device's order for one utterance: 64 partial sums (partial q adds samples q, q + 64, ...), then a binary tree"""
    acc = np.zeros(64)
    for k in range(0, len(term), 64):
        seg = term[k:k + 64]; acc[:len(seg)] = acc[:len(seg)] + seg
    while len(acc) > 1:
        acc = acc[0::2] + acc[1::2]
    return float(acc[0])


def trainGGD(X, nframes=None, p=0.7, sa=1.0, alpha=0.05, maxUpdates=20, thresh=0.00001, floorV=10e-8, floorP=0.07, sigmaOnly=False):
    """ML training of all F bins at once from subband samples X (cuda complex64 [U][T][F]): accumulate on the device, update on the host, until
    every bin has converged or maxUpdates is reached; a bin that has converged keeps its parameters, as update() of a converged model does.
    alpha multiplies the gradient of the whole sample set (update() does not divide by the sample count).
    -> (ggdL: a list of F fixed CGGaussianD, p [F], sa [F], converged [F])"""
    F = X.shape[2]
    p = np.full(F, p, np.float64) if np.ndim(p) == 0 else np.array(p, np.float64)
    sa = np.full(F, sa, np.float64) if np.ndim(sa) == 0 else np.array(sa, np.float64)
    conv = np.zeros(F, bool)
    for it in range(maxUpdates):
        acc = K.ggd_accumulate(X, p, sa, nframes)
        ns, npp, cv = K.ggd_update(acc, p, sa, it, alpha, thresh, floorV, floorP, sigmaOnly)
        sa = np.where(conv, sa, ns); p = np.where(conv, p, npp); conv = conv | cv
        if conv.all():
            break
    ggdL = []
    for f in range(F):
        g = CGGaussianD(float(p[f]), float(sa[f])); g.fixConst(); ggdL.append(g)
    return ggdL, p, sa, conv
