"""Fast speaker-adaptive training through the C-ABI (include/dsr.h section 14b): the handle that folds the statistics of S speaker slots into
the speaker-independent fast accumulators, keeps them in a file, accumulates the matrix statistic from counts alone and re-estimates the
canonical means (MDL) and variances together (csrc/fsat_kernels.hip, csrc/fsat.cpp).  Built on dsr._capi._core and dsr._sat; dsr._capi
re-exports FastSat and fsat_check.  Importing this module imports neither torch nor the library."""
import ctypes as C

import numpy as np

from ._capi import _core
from ._capi._core import Handle, check, cur_stream, load, _np, _ptr
from ._sat import Sat


def fsat_check(meanLen, featLen, massThreshold=10.0, mmiMultiplier=1.0, meanOnly=False, maxNoRegClass=1):
    """the options of FastMeanVarianceSAT(...) this library takes; raises DsrError otherwise"""
    check(load().dsr_fsat_check(int(meanLen), int(featLen), float(massThreshold), float(mmiMultiplier), int(bool(meanOnly)), int(maxNoRegClass)))


class _InnerSat(Sat):
    """the dsr_sat a dsr_fsat owns, borrowed: transforms, SAT sums, records, solution, statuses and timing are read through it"""

    def __init__(self, owner, h):
        self._owner = owner; self.h = C.c_void_p(h); self.trainer = owner.trainer; self.gmm = owner.gmm; self.D = owner.D; self.G = owner.G
        self.S = _core._lib.dsr_sat_num_slots(self.h)


class FastSat(Handle):
    """FastMeanVarianceSAT over a Trainer's model: S speaker slots; norm folds them into the fast accumulators, accumulate needs their counts
    only, update re-estimates means and variances."""

    _destroy = "dsr_fsat_destroy"

    def __init__(self, trainer, S=1, lhoodThreshold=0.0, massThreshold=0.0, nParts=1, part=1, meanOnly=False):
        L = load(); self.trainer = trainer; self.gmm = trainer.gmm; self.D = self.gmm.D; self.G = trainer.G
        self._create(L.dsr_fsat_create, trainer.h, int(S), float(lhoodThreshold), float(massThreshold), int(nParts), int(part), int(bool(meanOnly)))
        self.sat = _InnerSat(self, L.dsr_fsat_sat(self.h)); self.S = self.sat.S

    def fast_blocks(self):
        return _core._lib.dsr_fsat_fast_blocks(self.h)

    def desc_blocks(self):
        return _core._lib.dsr_fsat_desc_blocks(self.h)

    def set_stats(self, s, trainer=None, count=None, den=None, sumO=None, sumOsq=None):
        """the statistics of slot s: a Trainer (device to device) or host arrays count, den [G] and sumO, sumOsq [G][D] (both None: counts only)"""
        if trainer is not None:
            check(_core._lib.dsr_fsat_set_stats(self.h, int(s), trainer.h)); return
        count = _np(count, np.float64); den = _np(np.zeros(self.G) if den is None else den, np.float64)
        assert count.shape == (self.G,) and den.shape == (self.G,) and (sumO is None) == (sumOsq is None)
        if sumO is not None:
            sumO = _np(sumO, np.float64); sumOsq = _np(sumOsq, np.float64); assert sumO.shape == (self.G, self.D) and sumOsq.shape == (self.G, self.D)
        check(_core._lib.dsr_fsat_set_stats_arrays(self.h, int(s), _ptr(count), _ptr(den), _ptr(sumO) if sumO is not None else None,
                                                   _ptr(sumOsq) if sumOsq is not None else None))

    def set_counts(self, s, trainer=None, count=None, den=None):
        if trainer is not None:
            check(_core._lib.dsr_fsat_set_counts(self.h, int(s), trainer.h)); return
        self.set_stats(s, count=count, den=den)

    def set_tree(self, s, tree):
        check(_core._lib.dsr_fsat_set_tree(self.h, int(s), tree.h))

    def set_apt(self, s, apt, aptSlot=0):
        check(_core._lib.dsr_fsat_set_apt(self.h, int(s), apt.h, int(aptSlot)))

    def set_transform(self, s, rc, kind, A, b=None):
        """A [nBlocks][bl][bl] (or [D][D] for one block), b [D] or None"""
        A = _np(A, np.float64); A = A[None] if A.ndim == 2 else A; assert A.ndim == 3 and A.shape[1] == A.shape[2] and A.shape[0] * A.shape[1] == self.D
        b = _np(b, np.float64) if b is not None else None; assert b is None or b.shape == (self.D,)
        check(_core._lib.dsr_fsat_set_transform(self.h, int(s), int(rc), int(kind), A.shape[0], _ptr(A), _ptr(b) if b is not None else None))

    def clear_slot(self, s):
        check(_core._lib.dsr_fsat_clear_slot(self.h, int(s)))

    def set_apt_sub_features(self, nSubFeat):
        self.sat.set_apt_sub_features(nSubFeat)

    def set_reg_classes_to_one(self):
        check(_core._lib.dsr_fsat_set_reg_classes_to_one(self.h))

    def norm(self, nSlots=None):
        check(_core._lib.dsr_fsat_norm(self.h, int(self.S if nSlots is None else nSlots), cur_stream()))

    def zero_fast(self):
        check(_core._lib.dsr_fsat_zero_fast(self.h))

    def save_fast(self, fileName):
        check(_core._lib.dsr_fsat_save_fast(self.h, fileName.encode()))

    def load_fast(self, fileName, nParts=1, part=1):
        check(_core._lib.dsr_fsat_load_fast(self.h, fileName.encode(), int(nParts), int(part)))

    def get_fast(self):
        """-> dict(count [G], den [G], fastMean [G][D], fastVar [G][D], scalar [G][nblks])"""
        check(_core._lib.dsr_fsat_get_fast(self.h, None, None, None, None, None))                # refused while there are none
        nB = self.fast_blocks(); c = np.zeros(self.G); d = np.zeros(self.G); m = np.zeros((self.G, self.D)); v = np.zeros((self.G, self.D)); sc = np.zeros((self.G, nB))
        check(_core._lib.dsr_fsat_get_fast(self.h, _ptr(c), _ptr(d), _ptr(m), _ptr(v), _ptr(sc)))
        return dict(count=c, den=d, fastMean=m, fastVar=v, scalar=sc)

    def set_fast(self, count, den, fastMean, fastVar, scalar):
        c = _np(count, np.float64); d = _np(den, np.float64); m = _np(fastMean, np.float64); v = _np(fastVar, np.float64); sc = _np(scalar, np.float64)
        assert c.shape == d.shape == (self.G,) and m.shape == v.shape == (self.G, self.D) and sc.ndim == 2 and sc.shape[0] == self.G
        check(_core._lib.dsr_fsat_set_fast(self.h, sc.shape[1], _ptr(c), _ptr(d), _ptr(m), _ptr(v), _ptr(sc)))

    def add_fast(self):
        check(_core._lib.dsr_fsat_add_fast(self.h))

    def accumulate(self, nSlots=None):
        check(_core._lib.dsr_fsat_accumulate(self.h, int(self.S if nSlots is None else nSlots), cur_stream()))

    def update(self):
        """-> dict(info [4], totals [2], aux, status): the counters are filled in even when the call reports flagged Gaussians (status != 0)"""
        info = np.zeros(4, np.uint32); tot = np.zeros(2, np.uint32); aux = C.c_double(0.0)
        st = _core._lib.dsr_fsat_update(self.h, _ptr(info), _ptr(tot), C.byref(aux))
        self.last = dict(info=[int(x) for x in info], totals=[int(x) for x in tot], aux=aux.value, status=st)
        check(st); return self.last

    def zero(self):
        check(_core._lib.dsr_fsat_zero(self.h))

    def desc_length(self):
        dl = C.c_uint(0); check(_core._lib.dsr_fsat_desc_length(self.h, C.byref(dl))); return dl.value

    def get_desc_len(self):
        a = np.zeros((self.G, max(self.desc_blocks(), 1)), np.uint16); check(_core._lib.dsr_fsat_get_desc_len(self.h, _ptr(a))); return a

    def set_desc_len(self, descLen):
        a = _np(descLen, np.uint16); assert a.ndim == 2 and a.shape[0] == self.G
        check(_core._lib.dsr_fsat_set_desc_len(self.h, a.shape[1], _ptr(a)))

    def estimate_files(self, speakerList, paramPrefix, accuPrefix):
        r = C.c_double(0.0)
        check(_core._lib.dsr_fsat_estimate_files(self.h, speakerList.encode(), paramPrefix.encode(), accuPrefix.encode(), C.byref(r))); return r.value

    def records(self):
        """of the last update -> (kept, decision, auxOld, auxNew, descLen), each [G][nBlocks]"""
        nB = max(self.sat.num_blocks(), 1); k = np.zeros((self.G, nB), np.int32); d = np.zeros((self.G, nB), np.int32); ao = np.zeros((self.G, nB)); an = np.zeros((self.G, nB))
        dl = np.zeros((self.G, nB), np.int32)
        check(_core._lib.dsr_fsat_get_records(self.h, _ptr(k), _ptr(d), _ptr(ao), _ptr(an), _ptr(dl))); return k, d, ao, an, dl

    def solution(self):
        return self.sat.solution()

    def gaussian_status(self, g):
        return self.sat.gaussian_status(g)

    def set_timing(self, on=True):
        self.sat.set_timing(on)

    def kernel_ms(self):
        ms = (C.c_float * 3)(); check(_core._lib.dsr_fsat_kernel_ms(self.h, ms)); return ms[0], ms[1], ms[2]
