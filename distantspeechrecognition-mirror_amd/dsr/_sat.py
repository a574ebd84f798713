"""Speaker-adaptive training through the C-ABI (include/dsr.h section 14): the speaker list, the handle that accumulates the SAT mean and
variance statistics of S speaker slots at once and re-estimates the canonical model (csrc/sat_kernels.hip, csrc/sat.cpp).  Built on
dsr._capi._core (the common handle base); dsr._capi re-exports Sat, speaker_list_read, sat_check and the constants.  Importing this module
imports neither torch nor the library."""
import ctypes as C

import numpy as np

from ._capi import _core
from ._capi._core import Handle, check, cur_stream, load, _np, _ptr

SAT_MEAN, SAT_VARIANCE = 1, 2
SAT_MLLR, SAT_APT = 1, 2
SAT_LEFT, SAT_UPDATED, SAT_KEPT_OLD, SAT_ZEROED, SAT_FLAGGED, SAT_NAN = range(6)


def speaker_list_read(fileName):
    """SpeakerList (asr/adapt/transform.cc:1989-1998) -> the labels, in file order"""
    L = load(); n = C.c_int(0); nb = C.c_int(0)
    check(L.dsr_speaker_list_read(fileName.encode(), None, 0, C.byref(n), C.byref(nb)))
    buf = C.create_string_buffer(max(nb.value, 1))
    check(L.dsr_speaker_list_read(fileName.encode(), buf, nb.value, C.byref(n), C.byref(nb)))
    return buf.raw[:nb.value].decode().split("\n")[:n.value]


def sat_check(meanLen, featLen, lhoodThreshold=0.0, accKind=0):
    """the options of SAT<Type>(...) this library takes; raises DsrError otherwise.  accKind 0 MeanAcc, 1 VarianceAcc, 2 FastAcc, 3 RegClassAcc, 4 MMI"""
    check(load().dsr_sat_check(int(meanLen), int(featLen), float(lhoodThreshold), int(accKind)))


class Sat(Handle):
    """ML-SAT over a Trainer's model: S speaker slots of statistics and transforms, accumulated a batch, then the mean or variance update."""

    _destroy = "dsr_sat_destroy"

    def __init__(self, trainer, S=1, massThreshold=0.0, nParts=1, part=1):
        L = load(); self.trainer = trainer; self.gmm = trainer.gmm; self.D = self.gmm.D; self.G = trainer.G
        self._create(L.dsr_sat_create, trainer.h, int(S), float(massThreshold), int(nParts), int(part)); self.S = L.dsr_sat_num_slots(self.h)

    def num_blocks(self):
        return _core._lib.dsr_sat_num_blocks(self.h)

    def set_apt_sub_features(self, nSubFeat):
        check(_core._lib.dsr_sat_set_apt_sub_features(self.h, int(nSubFeat)))

    def zero(self):
        check(_core._lib.dsr_sat_zero(self.h))

    def set_stats(self, s, trainer=None, c=None, sumO=None, sumOsq=None):
        """the statistics of slot s: a Trainer (device to device) or host arrays c [G], sumO, sumOsq [G][D]"""
        if trainer is not None:
            check(_core._lib.dsr_sat_set_stats(self.h, int(s), trainer.h)); return
        c = _np(c, np.float64); sumO = _np(sumO, np.float64); sumOsq = _np(sumOsq, np.float64)
        assert c.shape == (self.G,) and sumO.shape == (self.G, self.D) and sumOsq.shape == (self.G, self.D)
        check(_core._lib.dsr_sat_set_stats_arrays(self.h, int(s), _ptr(c), _ptr(sumO), _ptr(sumOsq)))

    def set_tree(self, s, tree):
        check(_core._lib.dsr_sat_set_tree(self.h, int(s), tree.h))

    def set_apt(self, s, apt, aptSlot=0):
        check(_core._lib.dsr_sat_set_apt(self.h, int(s), apt.h, int(aptSlot)))

    def set_transform(self, s, rc, kind, A, b=None):
        """A [nBlocks][bl][bl] (or [D][D] for one block), b [D] or None"""
        A = _np(A, np.float64); A = A[None] if A.ndim == 2 else A; assert A.ndim == 3 and A.shape[1] == A.shape[2] and A.shape[0] * A.shape[1] == self.D
        b = _np(b, np.float64) if b is not None else None; assert b is None or b.shape == (self.D,)
        check(_core._lib.dsr_sat_set_transform(self.h, int(s), int(rc), int(kind), A.shape[0], _ptr(A), _ptr(b) if b is not None else None))

    def slot_classes(self, s):
        n = _core._lib.dsr_sat_slot_classes(self.h, int(s), None, 0); a = np.zeros(n, np.uint32)
        _core._lib.dsr_sat_slot_classes(self.h, int(s), _ptr(a), n); return [int(x) for x in a]

    def get_transform(self, s, rc):
        """-> (kind, A [nBlocks][bl][bl], b [D], bSize)"""
        k = C.c_int(0); nb = C.c_int(0); bs = C.c_int(0)
        check(_core._lib.dsr_sat_get_transform(self.h, int(s), int(rc), C.byref(k), C.byref(nb), C.byref(bs), None, None))
        bl = self.D // nb.value; A = np.zeros((nb.value, bl, bl)); b = np.zeros(self.D)
        check(_core._lib.dsr_sat_get_transform(self.h, int(s), int(rc), None, None, None, _ptr(A), _ptr(b))); return k.value, A, b, bs.value

    def clear_slot(self, s):
        check(_core._lib.dsr_sat_clear_slot(self.h, int(s)))

    def accumulate(self, what, nSlots=None):
        check(_core._lib.dsr_sat_accumulate(self.h, int(what), int(self.S if nSlots is None else nSlots), cur_stream()))

    def update(self, what):
        """-> dict(info [4], totals [2], aux, status): the counters are filled in even when the call reports flagged Gaussians (status != 0)"""
        info = np.zeros(4, np.uint32); tot = np.zeros(2, np.uint32); aux = C.c_double(0.0)
        st = _core._lib.dsr_sat_update(self.h, int(what), _ptr(info), _ptr(tot), C.byref(aux))
        self.last = dict(info=[int(x) for x in info], totals=[int(x) for x in tot], aux=aux.value, status=st)
        check(st); return self.last

    def estimate_files(self, what, speakerList, paramPrefix, accuPrefix):
        r = C.c_double(0.0)
        check(_core._lib.dsr_sat_estimate_files(self.h, int(what), speakerList.encode(), paramPrefix.encode(), accuPrefix.encode(), C.byref(r))); return r.value

    def mean_accu(self, g, block=0):
        """-> (mat [bl][bl], vec [bl], scalar, occ)"""
        check(_core._lib.dsr_sat_get_mean_accus(self.h, None, None, None))
        bl = self.D // self.num_blocks(); mat = np.zeros((bl, bl)); vec = np.zeros(bl); sc = C.c_double(0.0); occ = C.c_double(0.0)
        check(_core._lib.dsr_sat_get_mean_accu(self.h, int(g), int(block), _ptr(mat), _ptr(vec), C.byref(sc), C.byref(occ))); return mat, vec, sc.value, occ.value

    def mean_accus(self):
        """-> (mat [G][nB][bl][bl], vec [G][nB][bl], scalar [G][nB], occ [G], has [G])"""
        check(_core._lib.dsr_sat_get_mean_accus(self.h, None, None, None))                      # refused before the first mean accumulation
        nB = self.num_blocks(); bl = self.D // nB; a = np.zeros((self.G, nB, bl * bl + bl + 1)); occ = np.zeros(self.G); has = np.zeros(self.G, np.int32)
        check(_core._lib.dsr_sat_get_mean_accus(self.h, _ptr(a), _ptr(occ), _ptr(has)))
        return a[:, :, :bl * bl].reshape(self.G, nB, bl, bl).copy(), a[:, :, bl * bl:bl * bl + bl].copy(), a[:, :, -1].copy(), occ, has

    def var_accu(self, g):
        vec = np.zeros(self.D); occ = C.c_double(0.0); check(_core._lib.dsr_sat_get_var_accu(self.h, int(g), _ptr(vec), C.byref(occ))); return vec, occ.value

    def var_accus(self):
        vec = np.zeros((self.G, self.D)); occ = np.zeros(self.G); check(_core._lib.dsr_sat_get_var_accus(self.h, _ptr(vec), _ptr(occ))); return vec, occ

    def keep_transformed(self, on=True):
        check(_core._lib.dsr_sat_keep_transformed(self.h, int(on)))

    def transformed(self, s):
        m = np.zeros((self.G, self.D), np.float32); check(_core._lib.dsr_sat_get_transformed(self.h, int(s), _ptr(m))); return m

    def records(self):
        """of the last mean update -> (kept, decision, auxOld, auxNew), each [G][nBlocks]"""
        nB = max(self.num_blocks(), 1); k = np.zeros((self.G, nB), np.int32); d = np.zeros((self.G, nB), np.int32); ao = np.zeros((self.G, nB)); an = np.zeros((self.G, nB))
        check(_core._lib.dsr_sat_get_records(self.h, _ptr(k), _ptr(d), _ptr(ao), _ptr(an))); return k, d, ao, an

    def solution(self):
        """the solved means of the last mean update in double [G][D], before the decision and the store to float"""
        x = np.zeros((self.G, self.D)); check(_core._lib.dsr_sat_get_solution(self.h, _ptr(x))); return x

    def gaussian_status(self, g):
        return _core._lib.dsr_sat_gaussian_status(self.h, int(g))

    def set_timing(self, on=True):
        check(_core._lib.dsr_sat_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 3)(); check(_core._lib.dsr_sat_kernel_ms(self.h, ms)); return ms[0], ms[1], ms[2]
