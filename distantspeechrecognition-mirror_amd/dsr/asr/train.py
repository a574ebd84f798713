"""asr.train: CodebookSetTrainPtr / CodebookTrainPtr / DistribSetTrainPtr / DistribTrainPtr (asr/train/codebookTrain.h, distribTrain.h) for 1:1
diagonal models, over dsr_train_* (include/dsr.h section 9).

The two sets share one training handle: the distribution set is built on the codebook set (as in the reference) and creates it; the codebook
set's methods need that to have happened.  Frames come from the feature stream the codebook set names -- accumulate() pulls frames 0..len(path)-1
through the stream protocol, puts them on the device once and runs the whole path as one batch -- or from `feats`, a cuda float32 [T][dimN]
tensor handed to setFeatures() (what a pipeline that already holds its features on the device uses).

    path = decoder.bestPath()                 # DecoderFlyWeightPtr.bestPath(): distribution names
    dss.accumulate(path, 1.0)
    cbs.update(); dss.update(); cbs.floorVariances(); cbs.fixGConsts(); cbs.invertVariances()
    dss.save(cbkFile, distFile)
"""
import numpy as np

from .. import _capi as K
from ..btk.stream import FeatureStreamPtr, _new
from .adapt import CodebookSetAdaptPtr, LDATransformerPtr, STCTransformerPtr, TransformerTreePtr
from .gaussian import DistribSetBasicPtr


class CodebookTrainPtr(object):
    def __init__(self, cbs, cbX):
        self._cbs, self._x = cbs, cbX

    def name(self):
        return K.load().dsr_gmm_codebook_name(self._cbs._need().gmm.h, self._x).decode()

    def refN(self):
        return int(self._cbs._need().gmm.params()["refN"][self._x])


class CodebookSetTrainPtr(CodebookSetAdaptPtr):
    """CodebookSetTrain(descFile, fs, cbkFile, massThreshold) (codebookTrain.cc:586-599); a CodebookSetAdapt, as in the reference"""

    def __init__(self, descFile="", fs=None, cbkFile="", massThreshold=5.0):
        CodebookSetAdaptPtr.__init__(self, descFile, fs, cbkFile)
        self._massThreshold = float(massThreshold); self._trainer = None; self.totalPr, self.totalT = 0.0, 0

    def _need(self):
        if self._trainer is None:
            raise K.DsrError(K.E_CONSISTENCY, "Must allocate codebook accumulators before accumulating FB statistics: build the DistribSetTrainPtr first")
        return self._trainer

    def find(self, key):
        t = self._need(); g = t.gmm
        names = [K.load().dsr_gmm_codebook_name(g.h, k).decode() for k in range(g.K)]
        x = names.index(key) if isinstance(key, str) else int(key)
        return CodebookTrainPtr(self, x)

    def allocAccus(self):
        if self._trainer is not None:
            self._trainer.zero(1)

    def zeroAccus(self, nParts=1, part=1):
        self._need().zero(1, nParts, part)

    def saveAccus(self, fileName, totalPr=0.0, totalT=0, onlyCountsFlag=False):
        self._need().save_codebook_accus(fileName, totalPr, totalT, onlyCountsFlag)

    def loadAccus(self, fileName, factor=1.0, nParts=1, part=1):
        self.totalPr, self.totalT = self._need().load_codebook_accus(fileName, factor, nParts, part)

    def update(self, nParts=1, part=1, verbose=False):
        self._need().update(1, nParts, part)

    def updateMMI(self, nParts=1, part=1, E=1.0):
        self._need().update_mmi(1, E, False, nParts, part)

    def floorVariances(self, nParts=1, part=1):
        total, floored = self._need().floor_variances(nParts, part)
        print("Floored %d of %d total variance components." % (floored, total))
        return total, floored

    def fixGConsts(self, nParts=1, part=1):
        self._need().fix_gconsts(nParts, part)

    def invertVariances(self, nParts=1, part=1):
        self._need().invert_variances(nParts, part)

    def save(self, cbkFile, distFile):
        self._need().gmm.save(cbkFile, distFile)


class DistribTrainPtr(object):
    def __init__(self, dss, distX):
        self._dss, self._x = dss, distX

    def name(self):
        return K.load().dsr_gmm_dist_name(self._dss.gmm.h, self._x).decode()

    def split(self, minCount=0.0, splitFactor=0.2):
        """DistribTrain::split (distribTrain.cc:92-109)"""
        self._dss._trainer.split(self._x, minCount, splitFactor)


class DistribSetTrainPtr(DistribSetBasicPtr):
    """DistribSetTrain(cbs, descFile, distFile) (distribTrain.cc:424-437)"""

    def __init__(self, cbs, descFile="", distFile="", gmmMode=0):
        DistribSetBasicPtr.__init__(self, cbs, descFile, distFile, gmmMode)
        self._trainer = K.Trainer(self.gmm, getattr(cbs, "_massThreshold", 5.0)); cbs._trainer = self._trainer
        self._feats = None

    def find(self, key):
        x = self.index(key) if isinstance(key, str) else int(key)
        if not 0 <= x < self.gmm.K:
            raise K.DsrError(K.E_INDEX, "distribution %d of %d" % (x, self.gmm.K))
        return DistribTrainPtr(self, x)

    def setFeatures(self, feats):
        """frames already on the device: cuda float32 [T][dimN] (None: pull them from the feature stream again)"""
        self._feats = feats

    def _frames(self, T):
        import torch
        if self._feats is not None:
            return self._feats
        rows = [np.array(self._feat.next(t), np.float32) for t in range(T)]
        return torch.from_numpy(np.stack(rows)).cuda().contiguous()

    def accumulate(self, path, factor=1.0):
        """DistribSetTrain::accumulate(path, factor) (distribTrain.cc:515-526): path = DecoderFlyWeightPtr.bestPath()"""
        ids = [self.index(n) if isinstance(n, str) else int(n) for n in path]
        score = self._trainer.accumulate_path(self._frames(len(ids)), ids, factor)
        print("Finished accumulation for %d frames." % len(ids))
        return score

    def accumulateLattice(self, lat, factor=1.0):
        """DistribSetTrain::accumulateLattice(lat, factor) (distribTrain.cc:528-561); lat: a LatticePtr after gammaProbs"""
        L = getattr(lat, "_lat", lat)
        ends = L.data["end"][L.data["in"] != 0]                 # epsilon links are skipped and may lie behind the last frame
        T = int(ends.max()) + 1 if len(ends) else 0
        n = self._trainer.accumulate_lattice(L, self._frames(T), factor)
        print("Finished accumulation for %d links." % n)
        return n

    def zeroAccus(self, nParts=1, part=1):
        self._trainer.zero(2, nParts, part)

    def saveAccus(self, fileName):
        self._trainer.save_distrib_accus(fileName)

    def loadAccus(self, fileName, nParts=1, part=1):
        self._trainer.load_distrib_accus(fileName, 1.0, nParts, part)

    def update(self, nParts=1, part=1):
        self._trainer.update(2, nParts, part)

    def updateMMI(self, nParts=1, part=1, merialdo=False):
        self._trainer.update_mmi(2, 1.0, merialdo, nParts, part)

    def save(self, cbkFile, distFile):
        self.gmm.save(cbkFile, distFile)


class EstimatorTreeMLLRPtr(TransformerTreePtr):
    """EstimatorTreeMLLR(cbs, paramTree, trace = 1, threshold = 1500.0) (estimateAdapt.cc:3143-3165): the regression classes of the Gaussians of
    `cbs` are the leaves; the statistics are the accumulators of the set's training handle"""

    def __init__(self, cbs, paramTree, trace=1, threshold=1500.0):
        TransformerTreePtr.__init__(self, cbs, paramTree)
        self._trace, self._threshold = trace, float(threshold)
        cls = cbs._model().reg_classes()
        if cls is None or (cls == 0).any():
            raise K.DsrError(K.E_INDEX, "Regression class index must be >= 1")
        self._estimated = False

    def _estimate(self):
        m = self._cbs._adapter()
        m.set_stats(0, self._cbs._need()); m.estimate(self._threshold)
        self._paramTree.copy_from(m.tree(0)); self._estimated = True
        if self._trace & 1:
            for s, node, leaf, copy in m.plan():
                print(("Copying parameters for node %d from node %d." % (leaf, node)) if copy else
                      ("Backing off from node %d to node %d." % (leaf, node)) if leaf != node else ("Estimating Parameters for Regression Class %d" % leaf))

    def writeParams(self, fileName):
        self._paramTree.write(fileName)

    def ttlFrames(self):
        """EstimatorTree::ttlFrames (estimateAdapt.cc:3052-3062): the sum over ALL nodes of the tree"""
        m = self._cbs._adapter()
        if not self._estimated:
            raise K.DsrError(K.E_CONSISTENCY, "ttlFrames is known after estimateAdaptationParameters")
        return float(sum(m.ttl_frames(0, n) for n in m.nodes()[0]))


class EstimatorTreeSLAPTPtr(EstimatorTreeMLLRPtr):
    """EstimatorTreeSLAPT(cbs, paramTree, biasType = "CepstraOnly", paramN, noItns = 10, trace = 1, threshold = 150.0) (train.i:366-386) over
    dsr_apt_* (include/dsr.h section 13).  paramTree: an APTParamTreePtr.  Only paramN = 1 -- the line search of the reference's one-parameter
    branch -- is implemented; the reference's default of 9 parameters (its Newton search) is refused with DSR_E_PARAMETER.  The sub-feature
    layout is the codebook set's (setSubFeatures)."""
    _kind = K.APT_SLAPT

    def __init__(self, cbs, paramTree, biasType="CepstraOnly", paramN=1, noItns=10, trace=1, threshold=150.0):
        if not isinstance(paramTree, K.AptParams):
            raise K.DsrError(K.E_CONSISTENCY, "Tree not instantiated with %s parameters." % ("RAPT" if self._kind == K.APT_RAPT else "SLAPT"))
        if biasType not in K.APT_BIAS:
            raise K.DsrError(15, "Unrecognized bias type %s" % biasType)            # jtype_error (getBiasType)
        EstimatorTreeMLLRPtr.__init__(self, cbs, paramTree, trace, threshold)
        self._bias = K.APT_BIAS[biasType]
        self._handle().set_param_n(paramN)

    def _handle(self):
        return self._cbs._apt_adapter(self._kind, self._bias)

    def _adapter(self):
        return self._handle()

    def _estimate(self):
        m = self._handle()
        m.store(0).copy_from(self._paramTree)                                     # not cleared: a tree that is not MLLR keeps its other classes
        m.set_stats(0, self._cbs._need()); m.estimate(self._threshold)
        self._paramTree.copy_from(m.store(0)); self._estimated = True
        if self._trace & 1:
            for s, node, leaf in m.plan():
                print(("Backing off from node %d to node %d." % (leaf, node)) if leaf != node else ("Estimating Parameters for Regression Class %d" % leaf))

    def ttlFrames(self):
        m = self._handle()
        if not self._estimated:
            raise K.DsrError(K.E_CONSISTENCY, "ttlFrames is known after estimateAdaptationParameters")
        return float(sum(m.ttl_frames(0, n) for n in m.nodes()[0]))


class EstimatorTreeBLTPtr(EstimatorTreeSLAPTPtr):
    """the same tree of BLTEstimatorAdapt nodes (estimateAdapt.cc:1623-1690; the reference's train.i does not expose one): one bilinear
    parameter alpha per regression class"""
    _kind = K.APT_RAPT

    def __init__(self, cbs, paramTree, biasType="CepstraOnly", trace=1, threshold=150.0):
        EstimatorTreeSLAPTPtr.__init__(self, cbs, paramTree, biasType, 1, 10, trace, threshold)


def estimateAdaptationParameters(tree):
    """estimateAdapt.cc:3064-3078: an MLLR parameter tree is cleared, then every leaf is estimated with back-off; a tree of all-pass
    parameters is not cleared and nothing is copied"""
    tree._estimate()


class _PathEstimator(object):
    """what STCEstimatorPtr and LDAEstimatorPtr share: the frames of a path.  accumulate() takes the scoring frames from the feature stream of
    the distribution set's codebooks and the statistics' frames from src, both pulled from frame 0 after a reset(); setFeatures() hands over
    frames that are on the device already."""
    _feats = None

    def setFeatures(self, xScore, xSrc=None):
        """cuda float32 [T][dimN]: the codebooks' frames and src's (None, None: pull them from the streams again)"""
        self._feats = None if xScore is None else (xScore, xScore if xSrc is None else xSrc)

    def _frames(self, T):
        import torch
        if self._feats is not None:
            return self._feats

        def pull(s):
            s.reset(); rows = [np.array(s.next(t), np.float32) for t in range(T)]
            return torch.from_numpy(np.stack(rows) if rows else np.zeros((0, s.size()), np.float32)).cuda().contiguous()
        xSrc = pull(self._src)
        feat = self._dss._feat
        return (xSrc if feat is self._src else pull(feat)), xSrc

    def _ids(self, path):
        return [self._dss.index(n) if isinstance(n, str) else int(n) for n in path]

    def zeroAccu(self):
        self._xf.zero(0)

    def saveAccu(self, fileName):
        self._xf.save_accu(fileName, 0)

    def loadAccu(self, fileName):
        self._xf.load_accu(fileName, 0)


class STCEstimatorPtr(_PathEstimator, STCTransformerPtr):
    """STCEstimator(src, pt, dss, idx = 0, bt = CepstralFeat, cascade = False, mmiEstimation = False, trace = 1, nm) (train.i:390-436,
    estimateAdapt.cc:2203-2711) over dsr_stc_* (include/dsr.h section 12).  pt, idx, bt and trace are accepted and unused: the parameter-tree
    path of this estimator ends in "Method not yet finished" in the reference (estimateAdapt.cc:2466-2469).

        stc = STCEstimatorPtr(src, None, dss); stc.accumulate(decoder.bestPath()); stc.estimate(); stc.save("stc.mat")
    """

    def __init__(self, src, pt, dss, idx=0, bt=None, cascade=False, mmiEstimation=False, trace=1, nm="STC Estimator"):
        STCTransformerPtr.__init__(self, src, 0, 0, nm, _cascade=cascade, _mmi=mmiEstimation)
        K.check(K.load().dsr_stc_feature_distrib_set(self._h, dss.gmm.h))
        self._dss, self._pt, self._idx, self._bt, self._trace = dss, pt, idx, bt, trace
        self._bind(); self._xf.gmm = dss.gmm

    def accumulate(self, path, factor=1.0):
        """accumulate(path, factor) (estimateAdapt.cc:2265-2294): path = DecoderFlyWeightPtr.bestPath()"""
        ids = self._ids(path); xScore, xSrc = self._frames(len(ids))
        n = self._xf.accumulate_path(xScore, ids, 0, factor, xSrc=xSrc)
        print("STCEstimator: accumulated %d %s frames." % (n, "numerator" if factor > 0.0 else "denominator"))

    def estimate(self, rc=1, minE=1.0, multE=1.0):
        self._xf.estimate(0, minE, multE)
        print("Using E = %g" % self._xf.E(0))
        return self

    def transMatrix(self):
        return self._xf.trans_matrix(0)

    def save(self, fileName, trans=None):
        """STCEstimator::save(fileName, trans) (estimateAdapt.cc:2327-2346): the float matrix, times `trans` (an LDA matrix in front) when given"""
        self._xf.save_float(fileName, trans, 0)

    def totalPr(self):
        return self._xf.get_accu(0)["totalPr"]

    def totalT(self):
        return self._xf.get_accu(0)["totalT"]


class LDAEstimatorPtr(_PathEstimator, LDATransformerPtr):
    """LDAEstimator(src, pt, dss, globalCodebook, idx = 0, bt = CepstralFeat, trace = 1) (train.i:461-500, estimateAdapt.cc:2714-3036).
    globalCodebook: a distribution or codebook set (or Gmm) whose codebook 0 is the global codebook.  pt, idx, bt and trace are accepted and
    unused.  The output size is the model's dimN (LDATransformer(src, orgSubFeatLen, nSubFeat)); a narrower LDATransformerPtr takes the first
    rows of the saved matrix."""

    def __init__(self, src, pt, dss, globalCodebook, idx=0, bt=None, trace=1):
        LDATransformerPtr.__init__(self, src, 0, 0)
        g = globalCodebook if isinstance(globalCodebook, K.Gmm) else getattr(globalCodebook, "gmm", None) or globalCodebook._model()
        K.check(K.load().dsr_lda_feature_codebooks(self._h, dss.gmm.h, g.h))
        self._dss, self._global, self._pt, self._idx, self._bt, self._trace = dss, g, pt, idx, bt, trace
        self._bind(); self._xf.gmm, self._xf.globalGmm = dss.gmm, g

    def accumulate(self, path, factor=1.0):
        """accumulate(path, factor) (estimateAdapt.cc:2761-2790) -> the summed score"""
        ids = self._ids(path); xScore, xSrc = self._frames(len(ids))
        return self._xf.accumulate_path(xScore, ids, 0, factor, xSrc=xSrc)

    def estimate(self, rc=1):
        self._xf.estimate(0)
        return self


class FeatureSpaceAdaptationFeaturePtr(FeatureStreamPtr):
    """FeatureSpaceAdaptationFeature(src, maxAccu = 1, maxTran = 1, nm) (asr/train/fsa.h, train.i:531-590) over dsr_fsa_* (include/dsr.h section
    11): a feature stream that delivers src under transformation 0, and the estimator of such transformations (constrained MLLR).

        fsa = FeatureSpaceAdaptationFeaturePtr(src); fsa.distribSet(dss); fsa.addAll()
        fsa.accumulate(decoder.bestPath()); fsa.estimate(10)          # then decode again from a distribution set built on fsa

    accumulate() takes the scoring frames from the feature stream of the distribution set's codebooks and the statistics' frames from src, both
    pulled from frame 0 after a reset(); setFeatures() hands over frames that are on the device already."""

    def __init__(self, src, maxAccu=1, maxTran=1, nm="FeatureSpaceAdaptationFeature"):
        h, _ = _new(K.load().dsr_fsa_feature_create, src._h, int(maxAccu), int(maxTran), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(src,))
        self._src, self._dss, self._fsa, self._feats = src, None, None, None

    def _need(self):
        if self._fsa is None:
            raise K.DsrError(K.E_CONSISTENCY, "Must initialize the distribution set before using.")
        return self._fsa

    def distribSet(self, dss):
        """distribSet(dssP) (fsa.h): the adaptation handle is made for the set's model"""
        import ctypes as C
        K.check(K.load().dsr_fsa_feature_distrib_set(self._h, dss.gmm.h))
        self._dss = dss; self._fsa = K.Fsa(gmm=dss.gmm, handle=C.c_void_p(K.load().dsr_fsa_feature_handle(self._h)), owner=self)

    def handle(self):
        """the dsr._capi.Fsa of this stream (the batch entries: accumulate over items, estimate over pairs, apply with per-row transforms)"""
        return self._need()

    def topN(self):
        return self._need().top_n()

    def setTopN(self, topN):
        self._need().set_top_n(topN)

    def count(self, accuX=0):
        return int(self._need().count(accuX))

    def shift(self):
        return self._need().shift()

    def setShift(self, shift):
        self._need().set_shift(shift)

    def setFeatures(self, xScore, xSrc=None):
        """frames already on the device, cuda float32 [T][dimN]: the codebooks' frames and src's (None, None: pull them from the streams again)"""
        self._feats = None if xScore is None else (xScore, xScore if xSrc is None else xSrc)

    def _frames(self, T):
        import torch
        if self._feats is not None:
            return self._feats
        def pull(s):
            s.reset(); rows = [np.array(s.next(t), np.float32) for t in range(T)]
            return torch.from_numpy(np.stack(rows) if rows else np.zeros((0, self.size()), np.float32)).cuda().contiguous()
        xSrc = pull(self._src)
        feat = self._dss._feat
        return (xSrc if feat is self._src else pull(feat)), xSrc

    def accumulate(self, path, accuX=0, factor=1.0):
        """accumulate(path, accuX, factor) (fsa.cc:282-297): path = DecoderFlyWeightPtr.bestPath(); a name the set does not know is passed over
        WITHOUT advancing the frame, as there"""
        f = self._need(); ids = []
        for n in path:
            if isinstance(n, str):
                try:
                    ids.append(self._dss.index(n))
                except K.DsrError:
                    ids.append(-1)
            else:
                ids.append(int(n))
        xScore, xSrc = self._frames(sum(1 for i in ids if i >= 0))
        n = f.accumulate_path(xScore, ids, accuX, factor, xSrc=xSrc)
        print("Accumulated %d frames." % n)
        return n

    def accumulateLattice(self, lat, accuX=0, factor=1.0):
        """accumulateLattice(lat, accuX, factor) (fsa.cc:299-321): every second frame of a link, as there; lat: a LatticePtr after gammaProbs"""
        f = self._need(); L = getattr(lat, "_lat", lat)
        ends = L.data["end"][L.data["in"] != 0]
        T = int(ends.max()) + 1 if len(ends) else 0
        xScore, xSrc = self._frames(T)
        n = f.accumulate_lattice(L, xScore, accuX, factor, xSrc=xSrc)
        print("Finished accumulation for %d links." % n)
        return n

    def zeroAccu(self, accuX=0):
        self._need().zero(accuX)

    def scaleAccu(self, scale, accuX=0):
        self._need().scale(scale, accuX)

    def addAccu(self, accuX, accuY, factor=1.0):
        self._need().add_accu(accuX, accuY, factor)

    def add(self, dsX):
        self._need().add(dsX)

    def addAll(self):
        self._need().add_all()

    def estimate(self, iterN=1, accuX=0, tranX=0):
        self._need().estimate(iterN, accuX, tranX)

    def clear(self, tranX=0):
        self._need().clear(tranX)

    def compareTransform(self, tranX, tranY):
        return float(self._need().compare(tranX, tranY))

    def saveAccu(self, name, accuX=0):
        self._need().save_accu(name, accuX)

    def loadAccu(self, name, accuX=0, factor=1.0):
        self._need().load_accu(name, accuX, factor)

    def save(self, name, tranX=0):
        self._need().save(name, tranX)

    def load(self, name, tranX=0):
        self._need().load(name, tranX)
