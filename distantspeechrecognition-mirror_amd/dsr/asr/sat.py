"""asr.sat: MeanSATPtr, VarianceSATPtr and SpeakerListPtr (asr/sat/sat.h:736-800, sat.i; asr/adapt/transform.cc:1989-1998) over dsr_sat_*
(include/dsr.h section 14), for the 1:1 diagonal models of a CodebookSetTrainPtr.

    spk = SpeakerListPtr("speakers.txt")
    MeanSATPtr(cbs, massThreshhold=10.0).estimate(spk, "params/", "accus/")        # params/<spkr>, accus/<spkr>.cbs.accu
    VarianceSATPtr(cbs).estimate(spk, "params/", "accus/"); cbs.invertVariances(); cbs.fixGConsts()

The fast form, FastMeanVarianceSATPtr over a CodebookSetFastSATPtr (sat.h:803-844, asr/sat/codebookFastSAT.cc; dsr_fsat_*, section 14b):

    cbs = CodebookSetFastSATPtr(...)                               # a CodebookSetTrainPtr that also keeps the fast accumulators
    for spkr in spk:                                               # the training pass: accumulate the speaker, fold, zero
        ...; cbs.normFastAccus(paramTree); cbs.zeroAccus()         # cbs.saveAccus(accus/<spkr>.cbs.accu, onlyCountsFlag=True) before the zero
    cbs.saveFastAccus("fast.accu")                                 # one file; shards are summed by loadFastAccus
    FastMeanVarianceSATPtr(cbs, lhoodThreshhold=0.1).estimate(spk, "params/", "accus/"); cbs.invertVariances(); cbs.fixGConsts()

One estimation pass re-estimates means (MDLSATMean: a direction is kept only when it earns more than lhoodThreshhold) and variances, from
every speaker's counts and transform alone.  MeanSATPtr and VarianceSATPtr stay the ML slice: they refuse a likelihood threshold.  Extended
means, an ldaFile and the regression-class and MMI accumulators (FastRegClassSATPtr, FastMaxMutualInfoSATPtr, FastMMIRegClassSATPtr) are
not built.
"""
from .. import _capi as K
from .train import CodebookSetTrainPtr


class SpeakerListPtr(object):
    """SpeakerList(spkrList): one label a line"""

    def __init__(self, spkrList):
        self.fileName = spkrList; self._list = K.speaker_list_read(spkrList)

    def __iter__(self):
        return iter(self._list)

    def __len__(self):
        return len(self._list)


class _SATPtr(object):
    _what, _kind = K.SAT_MEAN, 0

    def __init__(self, cbs, meanLen=0, lhoodThreshhold=0.0, massThreshhold=0.0, nParts=1, part=1, mmiMultiplier=1.0, meanOnly=False, slots=16):
        tr = cbs._need()
        K.sat_check(meanLen, tr.gmm.D, lhoodThreshhold, self._kind)
        if mmiMultiplier != 1.0 or meanOnly:                                 # they act in the MMI accumulators only (sat.cc:1760-1761), which are not built
            raise K.DsrError(K.E_PARAMETER, "mmiMultiplier = %g, meanOnly = %s: the MMI-SAT options are not implemented" % (mmiMultiplier, bool(meanOnly)))
        self._cbs = cbs; self.sat = K.Sat(tr, slots, massThreshhold, nParts, part)
        nSub = getattr(cbs, "_sub", None)
        if nSub:
            self.sat.set_apt_sub_features(nSub[1] if isinstance(nSub, tuple) else nSub)

    def zero(self):
        self.sat.zero()

    def estimate(self, sList, spkrAdaptParms, meanVarsStats):
        """SATBase::estimate (sat.cc:1802-1839) -> (sum totalPr) / (sum totalT)"""
        return self.sat.estimate_files(self._what, sList.fileName, spkrAdaptParms, meanVarsStats)


class MeanSATPtr(_SATPtr):
    """SAT<SATBase::MeanAcc>"""


class VarianceSATPtr(_SATPtr):
    """SAT<SATBase::VarianceAcc>"""
    _what, _kind = K.SAT_VARIANCE, 1


class CodebookSetFastSATPtr(CodebookSetTrainPtr):
    """CodebookSetFastSAT(descFile, fs, cbkFile) (codebookFastSAT.cc:571-581): a CodebookSetTrain that keeps one fast accumulator per Gaussian"""

    def __init__(self, descFile="", fs=None, cbkFile="", massThreshold=5.0):
        CodebookSetTrainPtr.__init__(self, descFile, fs, cbkFile, massThreshold); self._fsat = None

    def _fast(self):
        """the handle that holds this set's fast accumulators and description lengths: made on first use, one slot"""
        if self._fsat is None:
            self._fsat = K.FastSat(self._need(), 1)
            nSub = getattr(self, "_sub", None)
            if nSub:
                self._fsat.set_apt_sub_features(nSub[1] if isinstance(nSub, tuple) else nSub)
        return self._fsat

    def normFastAccus(self, paramTree, olen=0):
        """normFastAccus(transTree, olen): fold the accumulators of the current speaker, adapted by paramTree, into the fast accumulators"""
        f = self._fast()
        if olen not in (0, f.D):
            raise K.DsrError(K.E_DIMENSION, "olen = %d for features of %d: extended means are not implemented" % (olen, f.D))
        tree = paramTree.paramTree() if hasattr(paramTree, "paramTree") else paramTree
        if isinstance(tree, K.AptParams):
            m = self._apt_adapter(tree.type() or K.APT_SLAPT); m.store(0).copy_from(tree); f.set_apt(0, m, 0)
        else:
            f.set_tree(0, tree)
        f.set_stats(0, trainer=self._need()); f.norm(1)

    def saveFastAccus(self, fileName):
        self._fast().save_fast(fileName)

    def loadFastAccus(self, fileName, nParts=1, part=1):
        self._fast().load_fast(fileName, nParts, part)

    def zeroFastAccus(self, nParts=1, part=1):
        self._fast().zero_fast()

    def descLength(self):
        return self._fast().desc_length()

    def setRegClassesToOne(self):
        self._fast().set_reg_classes_to_one()


class FastMeanVarianceSATPtr(object):
    """SATFast<SATBase::FastAcc>(cbs, meanLen, lhoodThreshhold, massThreshhold, nParts, part, mmiMultiplier, meanOnly, maxNoRegClass) (sat.i:164-190)"""

    def __init__(self, cbs, meanLen=0, lhoodThreshhold=0.1, massThreshhold=10.0, nParts=1, part=1, mmiMultiplier=1.0, meanOnly=False, maxNoRegClass=1, slots=16):
        tr = cbs._need()
        K.fsat_check(meanLen, tr.gmm.D, massThreshhold, mmiMultiplier, meanOnly, maxNoRegClass)
        self._cbs = cbs; self.sat = K.FastSat(tr, slots, lhoodThreshhold, massThreshhold, nParts, part, meanOnly)
        nSub = getattr(cbs, "_sub", None)
        if nSub:
            self.sat.set_apt_sub_features(nSub[1] if isinstance(nSub, tuple) else nSub)

    def zero(self):
        self.sat.zero()

    def estimate(self, sList, spkrAdaptParms, meanVarsStats):
        """SATFast::estimate (sat.h:825-831) -> (lhoodThreshhold descLength() + sum totalPr) / (sum totalT).  The fast accumulators and the
        description lengths are those of the codebook set; the lengths this update leaves go back to it"""
        src = self._cbs._fast() if hasattr(self._cbs, "_fast") else None
        if src is not None:
            self.sat.set_fast(**src.get_fast())
            if src.desc_blocks():
                self.sat.set_desc_len(src.get_desc_len())
        r = self.sat.estimate_files(sList.fileName, spkrAdaptParms, meanVarsStats)
        if src is not None:
            src.set_desc_len(self.sat.get_desc_len())
        return r


def _not_built(name):
    class _Stub(object):
        def __init__(self, *a, **kw):
            raise K.DsrError(K.E_PARAMETER, "%s is not built" % name)
    _Stub.__name__ = name
    return _Stub


FastRegClassSATPtr = _not_built("FastRegClassSATPtr")                    # SATFast<RegClassAcc>: fast accumulators of several classes per Gaussian
FastMaxMutualInfoSATPtr = _not_built("FastMaxMutualInfoSATPtr")          # SATFast<MMIAcc>
FastMMIRegClassSATPtr = _not_built("FastMMIRegClassSATPtr")              # SATFast<MMIRegClassAcc>
