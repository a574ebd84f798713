"""asr.adapt: ParamTreePtr, CodebookSetAdaptPtr, TransformerTreePtr and adaptCbk (asr/adapt/adapt.i) for MLLR mean transforms, over
dsr_param_tree_* and dsr_mllr_* (include/dsr.h section 10).  The all-pass transforms (RAPT, SLAPT, BLT), STC and LDA are not implemented.

The model lives with the distribution set (as everywhere in this package): a codebook set is bound to it when its DistribSet*Ptr is built.

    paramTree = ParamTreePtr()
    tree = EstimatorTreeMLLRPtr(cbs, paramTree)         # dsr.asr.train; after dss.accumulate(path)
    estimateAdaptationParameters(tree); tree.writeParams("spk.mllr")
    adaptCbk(cbs, paramTree)                             # the model's means move; every scoring mode follows
    cbs.resetMean()
"""
from .. import _capi as K
from .gaussian import CodebookSetBasicPtr


class ParamTreePtr(K.ParamTree):
    """ParamTree(fileName = "") (transform.h:520-552): read / write / clear / hasIndex / find / findMLLR / type"""

    def __init__(self, fileName=""):
        K.ParamTree.__init__(self, fileName)


class CodebookSetAdaptPtr(CodebookSetBasicPtr):
    """CodebookSetAdapt(descFile, fs, cbkFile) (codebookAdapt.h): keeps the original means once a transform has been applied"""

    def __init__(self, descFile="", fs=None, cbkFile=""):
        CodebookSetBasicPtr.__init__(self, descFile, fs, cbkFile)
        self._mllr = None

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
        if self._mllr is not None:
            raise K.DsrError(K.E_CONSISTENCY, "regression classes are set before the first estimation or transform")
        self._model().set_reg_classes(int(c))

    def resetMean(self):
        if self._mllr is not None:
            self._mllr.reset_mean(self._model())


class TransformerTreePtr(object):
    """TransformerTree(cbs, paramTree) (transform.cc:2122-2163)"""

    def __init__(self, cbs, paramTree):
        self._cbs, self._paramTree = cbs, paramTree

    def paramTree(self):
        return self._paramTree

    def transform(self):
        print("\nTransforming Means")
        m = self._cbs._adapter()
        m.tree(0).copy_from(self._paramTree)
        m.adapt(0, self._cbs._model())
        return self


def adaptCbk(cbs, paramTree):
    """adapt.i: transform the means of `cbs` with the parameters of `paramTree`"""
    return TransformerTreePtr(cbs, paramTree).transform()
