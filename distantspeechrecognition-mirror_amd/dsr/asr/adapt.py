"""asr.adapt: ParamTreePtr, CodebookSetAdaptPtr, TransformerTreePtr and adaptCbk (asr/adapt/adapt.i) for MLLR mean transforms, over
dsr_param_tree_* and dsr_mllr_* (include/dsr.h section 10), STCTransformerPtr / LDATransformerPtr over dsr_stc_* / dsr_lda_* (section 12), and the
all-pass transforms -- APTParamTreePtr, RAPTParam, SLAPTParam, BLTTransformer, SLAPTTransformer -- over dsr_apt_* (section 13): the bilinear
transform and the sine-log all-pass transform; RAPT with more than one parameter is refused.

The model lives with the distribution set (as everywhere in this package): a codebook set is bound to it when its DistribSet*Ptr is built.

    paramTree = ParamTreePtr()
    tree = EstimatorTreeMLLRPtr(cbs, paramTree)         # dsr.asr.train; after dss.accumulate(path)
    estimateAdaptationParameters(tree); tree.writeParams("spk.mllr")
    adaptCbk(cbs, paramTree)                             # the model's means move; every scoring mode follows
    cbs.resetMean()

    cbs.setSubFeatures(13, 3); params = APTParamTreePtr()
    tree = EstimatorTreeSLAPTPtr(cbs, params, "CepstraOnly", paramN=1)      # dsr.asr.train; EstimatorTreeBLTPtr for the bilinear transform
    estimateAdaptationParameters(tree); tree.writeParams("spk.slapt"); adaptCbk(cbs, params)
"""
import ctypes as C

from .. import _capi as K
from ..btk.stream import FeatureStreamPtr, _new
from .gaussian import CodebookSetBasicPtr


class ParamTreePtr(K.ParamTree):
    """ParamTree(fileName = "") (transform.h:520-552): read / write / clear / hasIndex / find / findMLLR / type"""

    def __init__(self, fileName=""):
        K.ParamTree.__init__(self, fileName)


class APTParamTreePtr(K.AptParams):
    """ParamTree(fileName = "") holding RAPT or SLAPT parameters: read / write / clear / findAPT / type (1 RAPT, 2 SLAPT)"""

    def __init__(self, fileName=""):
        K.AptParams.__init__(self, fileName)


class _APTParam(object):
    """APTParamBase (transform.h:307-346): _conf, the bias and the regression class of one block of a parameter file"""

    def __init__(self, conf=(), bias=(), regClass=0):
        import numpy as np
        self.conf = np.array(np.atleast_1d(conf), np.float64); self.bias = np.array(np.atleast_1d(bias), np.float32); self._rc = int(regClass)

    def size(self):
        return len(self.conf)

    def __getitem__(self, i):
        return float(self.conf[i])

    def regClass(self):
        return self._rc

    def isZero(self):
        return len(self.conf) == 0

    def write(self, fileName):
        t = K.AptParams(); t.set(self._rc or 1, self._type, self.conf, self.bias); t.write(fileName)

    def transformer(self, sbFtSz, nSubFt):
        return (BLTTransformer if self._type == K.APT_RAPT else SLAPTTransformer)(self, sbFtSz, nSubFt)


class RAPTParam(_APTParam):
    """RAPTParam(alpha, bias, rc) (transform.h:350-375).  Its transformer is the BLTTransformer: more than one parameter is refused"""
    _type = K.APT_RAPT


class SLAPTParam(_APTParam):
    """SLAPTParam(seq, bias, rc) (transform.h:379-404)"""
    _type = K.APT_SLAPT


class _APTTransformer(object):
    """APTTransformerBase for one parameter block: matrix() is _calcTransMatrix of the block's series, transform(rows) the transformed
    means of rows [N][sbFtSz nSubFt] with the bias (transform.cc:1212-1242, 1295-1337); both are made on the device"""

    def __init__(self, par, sbFtSz, nSubFt=1):
        self._par = par if isinstance(par, _APTParam) else type(self)._param(par)
        self._L, self._nSub = int(sbFtSz), int(nSubFt)
        K.apt_transform_rows(self._kind, self._L, self._nSub, self._par.conf)             # the reference's jparameter_error comes at once

    def matrix(self):
        return K.apt_transform_rows(self._kind, self._L, self._nSub, self._par.conf)[0]

    def transform(self, rows, useBias=True):
        return K.apt_transform_rows(self._kind, self._L, self._nSub, self._par.conf, self._par.bias if useBias else (), rows)[1]


class BLTTransformer(_APTTransformer):
    """BLTTransformer(par or alpha, sbFtSz, nSubFt) (transform.cc:1366-1430)"""
    _kind, _param = K.APT_RAPT, RAPTParam


class SLAPTTransformer(_APTTransformer):
    """SLAPTTransformer(par or parameters, sbFtSz, nSubFt) (transform.cc:1636-1741)"""
    _kind, _param = K.APT_SLAPT, SLAPTParam


class CodebookSetAdaptPtr(CodebookSetBasicPtr):
    """CodebookSetAdapt(descFile, fs, cbkFile) (codebookAdapt.h): keeps the original means once a transform has been applied"""

    def __init__(self, descFile="", fs=None, cbkFile=""):
        CodebookSetBasicPtr.__init__(self, descFile, fs, cbkFile)
        self._mllr = None; self._apt = {}; self._sub = None

    def setSubFeatures(self, subFeatLen, nSubFeat=1):
        """the sub-feature layout the all-pass transforms work on (CodebookSetBasic::subFeatLen / nSubFeat): nSubFeat blocks of subFeatLen"""
        self._sub = (int(subFeatLen), int(nSubFeat))

    def _apt_adapter(self, kind, biasType=0):
        """the all-pass handle of this set for one kind and bias type: made on first use, as _adapter"""
        if (kind, biasType) not in self._apt:
            g = self._model(); L, nSub = self._sub or (g.D, 1)
            self._apt[(kind, biasType)] = K.Apt(g, 1, kind, L, nSub, biasType)
        return self._apt[(kind, biasType)]

    def _model(self):
        g = getattr(self, "_gmm", None)
        if g is None:
            raise K.DsrError(K.E_CONSISTENCY, "the codebook set has no model yet: build its DistribSet first")
        return g

    def _adapter(self):
        """the MLLR handle of this set: made on first use, so its originals are the means the set was loaded with"""
        if self._mllr is None:
            self._mllr = K.Mllr(self._model(), 1)
        return self._mllr

    def setRegClasses(self, c=1):
        if self._mllr is not None or self._apt:
            raise K.DsrError(K.E_CONSISTENCY, "regression classes are set before the first estimation or transform")
        self._model().set_reg_classes(int(c))

    def resetMean(self):
        for h in [self._mllr] + list(self._apt.values()):
            if h is not None:
                h.reset_mean(self._model()); break


class TransformerTreePtr(object):
    """TransformerTree(cbs, paramTree) (transform.cc:2122-2163)"""

    def __init__(self, cbs, paramTree):
        self._cbs, self._paramTree = cbs, paramTree

    def paramTree(self):
        return self._paramTree

    def transform(self):
        print("\nTransforming Means")
        if isinstance(self._paramTree, K.AptParams):                  # BLTTransformer / SLAPTTransformer per class
            m = self._cbs._apt_adapter(self._paramTree.type() or K.APT_SLAPT)
            m.store(0).copy_from(self._paramTree); m.adapt(0, self._cbs._model())
            return self
        m = self._cbs._adapter()
        m.tree(0).copy_from(self._paramTree)
        m.adapt(0, self._cbs._model())
        return self


def adaptCbk(cbs, paramTree):
    """adapt.i: transform the means of `cbs` with the parameters of `paramTree`"""
    return TransformerTreePtr(cbs, paramTree).transform()


class _MatrixStream(FeatureStreamPtr):
    """what STCTransformerPtr and LDATransformerPtr share: the handle the stream owns (matrix 0 of it is the stream's transform)"""

    def handle(self):
        """the dsr._capi.Stc / Lda of this stream (the batch entries)"""
        return self._xf

    def matrix(self):
        return self._xf.transform(0)

    def setMatrix(self, M):
        self._xf.set_transform(M, 0)

    def save(self, fileName):
        self._xf.save(fileName, 0)

    def load(self, fileName):
        self._xf.load(fileName, 0)


class STCTransformerPtr(_MatrixStream):
    """STCTransformer(src, sbFtSz = 0, nSubFt = 0, nm) (adapt.i:228-272, transform.cc:1788-1879) over dsr_stc_* (include/dsr.h section 12):
    src under a square matrix, the identity until load() or an estimate.  One sub-feature: sbFtSz is src.size() (0: take it), nSubFt 0 or 1.
    save / load: raw doubles."""

    def __init__(self, src, sbFtSz=0, nSubFt=0, nm="STC Transformer", _cascade=False, _mmi=False):
        if nSubFt not in (0, 1) or sbFtSz not in (0, src.size()):
            raise K.DsrError(K.E_DIMENSION, "STCTransformer is built for one sub-feature of the source's size (%d), not %d x %d" % (src.size(), sbFtSz, nSubFt))
        h, _ = _new(K.load().dsr_stc_feature_create, src._h, int(bool(_cascade)), int(bool(_mmi)), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(src,))
        self._src = src; self._bind()

    def _bind(self):
        self._xf = K.Stc(handle=C.c_void_p(K.load().dsr_stc_feature_handle(self._h)), owner=self)


class LDATransformerPtr(_MatrixStream):
    """LDATransformer(src, sbFtSz = 0, nSubFt = 0, nm) (adapt.i:275-304, transform.cc:1882-1984): the first sbFtSz rows of a src.size() x
    src.size() matrix, so the feature may shrink (0: src.size()).  save writes float32, load reads float64 -- the reference's own "HACK"
    (transform.cc:1961-1984), kept: a saved matrix is not read back by load()."""

    def __init__(self, src, sbFtSz=0, nSubFt=0, nm="LDA Transformer"):
        if nSubFt not in (0, 1):
            raise K.DsrError(K.E_DIMENSION, "LDATransformer is built for one sub-feature, not %d" % nSubFt)
        h, _ = _new(K.load().dsr_lda_feature_create, src._h, int(sbFtSz) or src.size(), nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(src,))
        self._src = src; self._bind()

    def _bind(self):
        self._xf = K.Lda(handle=C.c_void_p(K.load().dsr_lda_feature_handle(self._h)), owner=self)
