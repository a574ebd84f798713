"""asr.sat: MeanSATPtr, VarianceSATPtr and SpeakerListPtr (asr/sat/sat.h:736-800, sat.i; asr/adapt/transform.cc:1989-1998) over dsr_sat_*
(include/dsr.h section 14), for the 1:1 diagonal models of a CodebookSetTrainPtr.

    spk = SpeakerListPtr("speakers.txt")
    MeanSATPtr(cbs, massThreshhold=10.0).estimate(spk, "params/", "accus/")        # params/<spkr>, accus/<spkr>.cbs.accu
    VarianceSATPtr(cbs).estimate(spk, "params/", "accus/"); cbs.invertVariances(); cbs.fixGConsts()

The ML slice only: a likelihood threshold (MDLSATMean), extended means and the fast, regression-class and MMI accumulators are refused.
"""
from .. import _capi as K


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
