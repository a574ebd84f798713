"""asr/adapt: MLLR, feature-space adaptation, STC and LDA."""
import ctypes as C

import numpy as np

from . import _core
from ._core import (DsrError, Handle, check, cur_stream, load, torch, vp, E_INDEX, _np, _ptr, _dev)


def is_ancestor(ancestor, child):
    r = C.c_int(0); load(); check(_core._lib.dsr_is_ancestor(int(ancestor), int(child), C.byref(r))); return bool(r.value)


class ParamTree(Handle):
    """ParamTree of MLLR parameters (asr/adapt/transform.cc:789-950; include/dsr.h section 10).  Host only."""

    _destroy = "dsr_param_tree_destroy"

    def __init__(self, fileName="", handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle; return
        self._create(L.dsr_param_tree_create, fileName.encode())

    def clear(self):
        check(_core._lib.dsr_param_tree_clear(self.h))

    def read(self, fileName):
        check(_core._lib.dsr_param_tree_read(self.h, fileName.encode()))

    def write(self, fileName):
        check(_core._lib.dsr_param_tree_write(self.h, fileName.encode()))

    def copy_from(self, other):
        check(_core._lib.dsr_param_tree_copy(self.h, other.h))

    def type(self):
        return _core._lib.dsr_param_tree_type(self.h)

    def hasIndex(self, rc):
        return bool(_core._lib.dsr_param_tree_has_index(self.h, int(rc)))

    def indices(self):
        n = _core._lib.dsr_param_tree_indices(self.h, None, 0); a = np.zeros(n, np.uint32)
        _core._lib.dsr_param_tree_indices(self.h, _ptr(a), n); return [int(x) for x in a]

    def _W(self, rc, size):
        W = np.zeros((size, size + 1)); check(_core._lib.dsr_param_tree_get(self.h, int(rc), _ptr(W))); return W

    def find(self, rc, useAncestor=True):
        """-> W [size][size + 1] of the class, inserted as a copy of its nearest ancestor when missing"""
        n = C.c_int(0); check(_core._lib.dsr_param_tree_find(self.h, int(rc), int(useAncestor), 0, C.byref(n))); return self._W(rc, n.value)

    def findMLLR(self, rc, useAncestor=True):
        n = C.c_int(0); check(_core._lib.dsr_param_tree_find(self.h, int(rc), int(useAncestor), 1, C.byref(n))); return self._W(rc, n.value)

    def set(self, rc, W):
        W = _np(W, np.float64); assert W.ndim == 2 and W.shape[1] == W.shape[0] + 1
        check(_core._lib.dsr_param_tree_set(self.h, int(rc), W.shape[0], _ptr(W)))


class Mllr(Handle):
    """MLLR mean transforms for S speakers at once (csrc/k_mllr.hip; include/dsr.h section 10): statistics on fp64 MFMA, back-off on the host,
    Jacobi solves and the transformed means on the device.  Made from a Gmm with regression classes (Gmm.set_reg_classes or a codebook file
    that carries the table); the handle keeps that model's means as the originals."""

    _destroy = "dsr_mllr_destroy"

    def __init__(self, gmm, S=1):
        L = load(); self.gmm = gmm; self.D = gmm.D; self.G = gmm.G
        self._create(L.dsr_mllr_create, gmm.h, int(S)); self.S = L.dsr_mllr_num_speakers(self.h)

    def set_stats(self, s, trainer=None, c=None, sumO=None):
        """the statistics of slot s: a Trainer (count - denCount and sumO, device to device) or host arrays c [G], sumO [G][D]"""
        if trainer is not None:
            check(_core._lib.dsr_mllr_set_stats(self.h, int(s), trainer.h)); return
        c = _np(c, np.float64); sumO = _np(sumO, np.float64); assert c.shape == (self.G,) and sumO.shape == (self.G, self.D)
        check(_core._lib.dsr_mllr_set_stats_arrays(self.h, int(s), _ptr(c), _ptr(sumO)))

    def estimate(self, threshold=1500.0):
        check(_core._lib.dsr_mllr_estimate(self.h, float(threshold), cur_stream()))

    def speaker_status(self, s):
        return _core._lib.dsr_mllr_speaker_status(self.h, int(s))

    def plan(self):
        """the steps of the last estimate: rows (speaker, node, leaf, copy)"""
        n = C.c_int(0); check(_core._lib.dsr_mllr_get_plan(self.h, C.byref(n), None))
        a = np.zeros((n.value, 4), np.int32); check(_core._lib.dsr_mllr_get_plan(self.h, C.byref(n), _ptr(a))); return a

    def nodes(self):
        n = C.c_int(0); check(_core._lib.dsr_mllr_get_nodes(self.h, C.byref(n), None, None))
        a = np.zeros(n.value, np.uint32); leaf = np.zeros(n.value, np.int32); check(_core._lib.dsr_mllr_get_nodes(self.h, C.byref(n), _ptr(a), _ptr(leaf)))
        return [int(x) for x in a], [bool(x) for x in leaf]

    def stats(self, s, node, row):
        """-> G_i [D + 1][D + 1], z_i [D + 1] of the last estimate"""
        n = self.D + 1; Gi = np.zeros((n, n)); z = np.zeros(n)
        check(_core._lib.dsr_mllr_get_stats(self.h, int(s), int(node), int(row), _ptr(Gi), _ptr(z))); return Gi, z

    def ttl_frames(self, s, node):
        t = C.c_double(0.0); check(_core._lib.dsr_mllr_ttl_frames(self.h, int(s), int(node), C.byref(t))); return t.value

    def tree(self, s):
        h = _core._lib.dsr_mllr_tree(self.h, int(s))
        if not h:
            raise DsrError(E_INDEX, "speaker %d of %d" % (s, self.S))
        return ParamTree(handle=vp(h), owner=self)

    def transform(self, s, rc):
        W = np.zeros((self.D, self.D + 1)); check(_core._lib.dsr_mllr_get_transform(self.h, int(s), int(rc), _ptr(W))); return W

    def write(self, s, fileName):
        check(_core._lib.dsr_mllr_write(self.h, int(s), fileName.encode()))

    def read(self, s, fileName):
        check(_core._lib.dsr_mllr_read(self.h, int(s), fileName.encode()))

    def adapt(self, s, target=None):
        check(_core._lib.dsr_mllr_adapt(self.h, int(s), (target or self.gmm).h))

    def adapt_all(self, out=None):
        """-> cuda float32 [S][G][D]: every speaker's transformed means"""
        if out is None:
            out = torch.empty((self.S, self.G, self.D), dtype=torch.float32, device="cuda")
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (self.S, self.G, self.D)
        check(_core._lib.dsr_mllr_adapt_all(self.h, _dev(out), cur_stream())); return out

    def reset_mean(self, target=None):
        check(_core._lib.dsr_mllr_reset_mean(self.h, (target or self.gmm).h))

    def set_timing(self, on=True):
        check(_core._lib.dsr_mllr_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 3)(); check(_core._lib.dsr_mllr_kernel_ms(self.h, ms)); return ms[0], ms[1], ms[2]


class Fsa(Handle):
    """Feature-space adaptation (constrained MLLR) for several accumulators and transformations (csrc/k_fsa.hip, csrc/fsa.cpp; include/dsr.h
    section 11): statistics on fp64 MFMA, Jacobi pseudo-inverses and the row updates on the device, the transform bit-exact.
    Made from a Gmm, or around the handle a FeatureSpaceAdaptationFeature stream owns (handle=, owner=)."""

    _destroy = "dsr_fsa_destroy"

    def __init__(self, gmm=None, nAccu=1, nTran=1, handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle
        else:
            self._create(L.dsr_fsa_create, gmm.h, int(nAccu), int(nTran))
        self.gmm = gmm; self.D = L.dsr_fsa_dim(self.h); self.nAccu = L.dsr_fsa_num_accus(self.h); self.nTran = L.dsr_fsa_num_transforms(self.h)

    def add(self, dsX):
        check(_core._lib.dsr_fsa_add(self.h, int(dsX)))

    def add_all(self):
        check(_core._lib.dsr_fsa_add_all(self.h))

    def set_top_n(self, topN):
        check(_core._lib.dsr_fsa_set_top_n(self.h, int(topN)))

    def top_n(self):
        return _core._lib.dsr_fsa_top_n(self.h)

    def set_shift(self, shift):
        check(_core._lib.dsr_fsa_set_shift(self.h, float(shift)))

    def shift(self):
        return _core._lib.dsr_fsa_shift(self.h)

    def count(self, accuX=0):
        c = C.c_double(0.0); check(_core._lib.dsr_fsa_count(self.h, int(accuX), C.byref(c))); return c.value

    def _frames(self, xScore, xSrc):
        xSrc = xScore if xSrc is None else xSrc
        for x in (xScore, xSrc):
            assert x.is_cuda and x.is_contiguous() and x.dtype.is_floating_point and x.element_size() == 4 and x.shape[1] == self.D
        assert xScore.shape[0] == xSrc.shape[0]
        return xScore, xSrc

    def accumulate(self, xScore, frame, dist, gamma, accu, xSrc=None, want_nearest=False):
        """xScore, xSrc: cuda float32 [N][D] (xSrc None: the same frames); frame, dist, gamma, accu: host arrays [M] -> accepted items [nAccu]
        (with want_nearest also the Gaussian each item chose inside its codebook, -1 for a distribution that is not switched on)"""
        xScore, xSrc = self._frames(xScore, xSrc)
        fr = _np(frame, np.int32); ds = _np(dist, np.int32); ga = _np(gamma, np.float32); ac = _np(accu, np.int32); M = len(fr)
        assert len(ds) == M and len(ga) == M and len(ac) == M
        acc = np.zeros(self.nAccu, np.int64); near = np.full(M, -1, np.int32) if want_nearest else None
        check(_core._lib.dsr_fsa_accumulate(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(fr), _ptr(ds), _ptr(ga), _ptr(ac), M, _ptr(acc),
                                      _ptr(near) if want_nearest else None, cur_stream()))
        return (acc, near) if want_nearest else acc

    def accumulate_path(self, xScore, distIds, accuX=0, factor=1.0, xSrc=None):
        """distIds: one distribution per frame, negative for a name the set does not know -> the frames the reference reports"""
        xScore, xSrc = self._frames(xScore, xSrc); ids = _np(distIds, np.int32); n = C.c_uint(0)
        check(_core._lib.dsr_fsa_accumulate_path(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(ids), len(ids), int(accuX), float(factor), C.byref(n), cur_stream()))
        return n.value

    def accumulate_lattice(self, lattice, xScore, accuX=0, factor=1.0, xSrc=None):
        """lattice: a Lattice (after gammaProbs) -> the number of links accumulated"""
        xScore, xSrc = self._frames(xScore, xSrc); n = C.c_uint(0)
        check(_core._lib.dsr_fsa_accumulate_lattice(self.h, lattice.h, _dev(xScore), _dev(xSrc), xScore.shape[0], int(accuX), float(factor), C.byref(n), cur_stream()))
        return n.value

    def zero(self, accuX=0):
        check(_core._lib.dsr_fsa_zero(self.h, int(accuX)))

    def scale(self, scale, accuX=0):
        check(_core._lib.dsr_fsa_scale(self.h, float(scale), int(accuX)))

    def add_accu(self, accuX, accuY, factor=1.0):
        check(_core._lib.dsr_fsa_add_accu(self.h, int(accuX), int(accuY), float(factor)))

    def get_accu(self, accuX=0):
        """-> dict(count, beta (float32), z [D][D + 1], G [D][D + 1][D + 1] with the triangle as the reference holds it)"""
        D = self.D; c = C.c_double(0.0); b = C.c_float(0.0); z = np.zeros((D, D + 1)); G = np.zeros((D, D + 1, D + 1))
        check(_core._lib.dsr_fsa_get_accu(self.h, int(accuX), C.byref(c), C.byref(b), _ptr(z), _ptr(G)))
        return dict(count=c.value, beta=np.float32(b.value), z=z, G=G)

    def set_accu(self, accuX=0, count=None, beta=None, z=None, G=None):
        D = self.D
        c = C.byref(C.c_double(float(count))) if count is not None else None
        b = C.byref(C.c_float(float(beta))) if beta is not None else None
        if z is not None:
            z = _np(z, np.float64); assert z.shape == (D, D + 1)
        if G is not None:
            G = _np(G, np.float64); assert G.shape == (D, D + 1, D + 1)
        check(_core._lib.dsr_fsa_set_accu(self.h, int(accuX), c, b, _ptr(z) if z is not None else None, _ptr(G) if G is not None else None))

    def save_accu(self, fileName, accuX=0):
        check(_core._lib.dsr_fsa_save_accu(self.h, fileName.encode(), int(accuX)))

    def load_accu(self, fileName, accuX=0, factor=1.0):
        check(_core._lib.dsr_fsa_load_accu(self.h, fileName.encode(), int(accuX), float(factor)))

    def estimate(self, iterN=1, accuX=0, tranX=0):
        """accuX, tranX: ints or equally long lists: the pairs are estimated concurrently"""
        a = _np(np.atleast_1d(accuX), np.int32); t = _np(np.atleast_1d(tranX), np.int32); assert len(a) == len(t)
        check(_core._lib.dsr_fsa_estimate(self.h, int(iterN), _ptr(a), _ptr(t), len(a), cur_stream()))

    def transform_status(self, tranX=0):
        return _core._lib.dsr_fsa_transform_status(self.h, int(tranX))

    def transform(self, tranX=0):
        W = np.zeros((self.D, self.D + 1)); check(_core._lib.dsr_fsa_get_transform(self.h, int(tranX), _ptr(W))); return W

    def set_transform(self, W, tranX=0):
        W = _np(W, np.float64); assert W.shape == (self.D, self.D + 1)
        check(_core._lib.dsr_fsa_set_transform(self.h, int(tranX), _ptr(W)))

    def clear(self, tranX=0):
        check(_core._lib.dsr_fsa_clear(self.h, int(tranX)))

    def compare(self, tranX, tranY):
        s = C.c_float(0.0); check(_core._lib.dsr_fsa_compare(self.h, int(tranX), int(tranY), C.byref(s))); return np.float32(s.value)

    def save(self, fileName, tranX=0):
        check(_core._lib.dsr_fsa_save(self.h, fileName.encode(), int(tranX)))

    def load(self, fileName, tranX=0):
        check(_core._lib.dsr_fsa_load(self.h, fileName.encode(), int(tranX)))

    def apply(self, x, tranOfRow=None, shift=1.0, out=None):
        """x: cuda float32 [N][D]; tranOfRow: cuda int32 [N] or None (transformation 0) -> cuda float32 [N][D]"""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.D
        if out is None:
            out = torch.empty_like(x)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == x.shape
        if tranOfRow is not None:
            assert tranOfRow.is_cuda and tranOfRow.is_contiguous() and tranOfRow.dtype == torch.int32 and tranOfRow.shape[0] == x.shape[0]
        check(_core._lib.dsr_fsa_apply(self.h, _dev(x), x.shape[0], _dev(tranOfRow) if tranOfRow is not None else None, float(shift), _dev(out), cur_stream()))
        return out

    def set_timing(self, on=True):
        check(_core._lib.dsr_fsa_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 5)(); check(_core._lib.dsr_fsa_kernel_ms(self.h, ms)); return tuple(ms)


class _Estimators(Handle):
    """what Stc and Lda share: frames, items, timing"""

    def _frames(self, xScore, xSrc):
        xSrc = xScore if xSrc is None else xSrc
        for x in (xScore, xSrc):
            assert x.is_cuda and x.is_contiguous() and x.dtype.is_floating_point and x.element_size() == 4 and x.shape[1] == self.D
        assert xScore.shape[0] == xSrc.shape[0]
        return xScore, xSrc

    def _items(self, fn, xScore, frame, dist, factor, est, xSrc, want):
        xScore, xSrc = self._frames(xScore, xSrc)
        fr = _np(frame, np.int32); ds = _np(dist, np.int32); fa = _np(factor, np.float32); es = _np(est, np.int32); M = len(fr)
        assert len(ds) == M and len(fa) == M and len(es) == M
        near = np.full(M, -1, np.int32); score = np.zeros(M, np.float32)
        check(fn(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(fr), _ptr(ds), _ptr(fa), _ptr(es), M, _ptr(near), _ptr(score), cur_stream()))
        return (near, score) if want else None

    def _mat(self, M, shape):
        M = _np(M, np.float64); assert M.shape == shape
        return M

    def kernel_ms(self):
        ms = (C.c_float * 5)(); check(self._kernel_ms(self.h, ms)); return tuple(ms)


class Stc(_Estimators):
    """Semi-tied covariance transforms for nEst estimators over one Gmm (csrc/k_stc.hip, csrc/stc.cpp; include/dsr.h section 12): statistics
    on fp64 MFMA, makePosDef's eigenvalues, the inverses and the row updates on the device, the transform bit-exact.  Made from a Gmm, as a
    bare transformer (dimN=), or around the handle an STCTransformer stream owns (handle=, owner=)."""

    _destroy = "dsr_stc_destroy"

    def __init__(self, gmm=None, nEst=1, cascade=False, mmiEstimation=False, dimN=None, handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle
        elif gmm is not None:
            self._create(L.dsr_stc_create, gmm.h, int(nEst), int(bool(cascade)), int(bool(mmiEstimation)))
        else:
            self._create(L.dsr_stc_create_transformer, int(dimN))
        self.gmm = gmm; self.D = L.dsr_stc_dim(self.h); self.nEst = L.dsr_stc_num_estimators(self.h); self._kernel_ms = L.dsr_stc_kernel_ms

    def accumulate(self, xScore, frame, dist, factor, est, xSrc=None, want_nearest=False):
        """xScore, xSrc: cuda float32 [N][D] (xSrc None: the same frames); frame, dist, factor, est: host arrays [M]; with want_nearest ->
        (the Gaussian each item chose inside its codebook, the distribution's score of each item)"""
        return self._items(_core._lib.dsr_stc_accumulate, xScore, frame, dist, factor, est, xSrc, want_nearest)

    def accumulate_path(self, xScore, distIds, estX=0, factor=1.0, xSrc=None):
        """distIds: one distribution per frame -> the number of frames"""
        xScore, xSrc = self._frames(xScore, xSrc); ids = _np(distIds, np.int32); n = C.c_uint(0)
        check(_core._lib.dsr_stc_accumulate_path(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(ids), len(ids), int(estX), float(factor), C.byref(n), cur_stream()))
        return n.value

    def increment(self, totalPr, totalT=0, estX=0):
        check(_core._lib.dsr_stc_increment(self.h, int(estX), float(totalPr), int(totalT)))

    def zero(self, estX=0):
        check(_core._lib.dsr_stc_zero(self.h, int(estX)))

    def get_accu(self, estX=0, through_accessor=False):
        """-> dict(count, denCount, totalPr, totalT, sumOsq [D][D][D], regSq [D][D][D]); through_accessor: after copyUpperTriangle, as the
        reference's sumOsq() / regSq() return them (and leave them); else the triangle as accumulation left it"""
        D = self.D; c = C.c_double(0.0); dc = C.c_double(0.0); pr = C.c_double(0.0); T = C.c_uint(0); S = np.zeros((D, D, D)); R = np.zeros((D, D, D))
        check(_core._lib.dsr_stc_get_accu(self.h, int(estX), int(bool(through_accessor)), C.byref(c), C.byref(dc), C.byref(pr), C.byref(T), _ptr(S), _ptr(R)))
        return dict(count=c.value, denCount=dc.value, totalPr=pr.value, totalT=T.value, sumOsq=S, regSq=R)

    def set_accu(self, estX=0, count=None, denCount=None, totalPr=None, totalT=None, sumOsq=None, regSq=None):
        D = self.D; dbl = lambda v: C.byref(C.c_double(float(v))) if v is not None else None      # noqa: E731
        S = self._mat(sumOsq, (D, D, D)) if sumOsq is not None else None; R = self._mat(regSq, (D, D, D)) if regSq is not None else None
        check(_core._lib.dsr_stc_set_accu(self.h, int(estX), dbl(count), dbl(denCount), dbl(totalPr), C.byref(C.c_uint(int(totalT))) if totalT is not None else None,
                                    _ptr(S) if S is not None else None, _ptr(R) if R is not None else None))

    def save_accu(self, fileName, estX=0):
        check(_core._lib.dsr_stc_save_accu(self.h, fileName.encode(), int(estX)))

    def load_accu(self, fileName, estX=0):
        check(_core._lib.dsr_stc_load_accu(self.h, fileName.encode(), int(estX)))

    def estimate(self, estX=0, minE=1.0, multE=1.0):
        """estX: an int or a list: the estimators are estimated concurrently"""
        e = _np(np.atleast_1d(estX), np.int32)
        check(_core._lib.dsr_stc_estimate(self.h, _ptr(e), len(e), float(minE), float(multE), cur_stream()))

    def status(self, estX=0):
        return _core._lib.dsr_stc_status(self.h, int(estX))

    def E(self, estX=0):
        e = C.c_double(0.0); check(_core._lib.dsr_stc_E(self.h, int(estX), C.byref(e))); return e.value

    def aux(self, estX=0, A=None, E=None):
        """the auxiliary function the row update maximises, of A (None: the estimator's matrix) at E (None: the last estimate's)"""
        q = C.c_double(0.0); A = self._mat(A, (self.D, self.D)) if A is not None else None
        check(_core._lib.dsr_stc_aux(self.h, int(estX), _ptr(A) if A is not None else None, float(self.E(estX) if E is None else E), C.byref(q))); return q.value

    def transform(self, estX=0):
        A = np.zeros((self.D, self.D)); check(_core._lib.dsr_stc_get_transform(self.h, int(estX), _ptr(A), None)); return A

    def inverse(self, estX=0):
        A = np.zeros((self.D, self.D)); check(_core._lib.dsr_stc_get_transform(self.h, int(estX), None, _ptr(A))); return A

    def set_transform(self, A, estX=0):
        check(_core._lib.dsr_stc_set_transform(self.h, int(estX), _ptr(self._mat(A, (self.D, self.D)))))

    def trans_matrix(self, estX=0):
        T = np.zeros((self.D, self.D), np.float32); check(_core._lib.dsr_stc_trans_matrix(self.h, int(estX), _ptr(T))); return T

    def save(self, fileName, estX=0):
        check(_core._lib.dsr_stc_save(self.h, fileName.encode(), int(estX)))

    def load(self, fileName, estX=0):
        check(_core._lib.dsr_stc_load(self.h, fileName.encode(), int(estX)))

    def save_float(self, fileName, trans=None, estX=0):
        if trans is not None:
            trans = _np(trans, np.float32); assert trans.shape == (self.D, self.D)
        check(_core._lib.dsr_stc_save_float(self.h, fileName.encode(), int(estX), _ptr(trans) if trans is not None else None))

    def apply(self, x, estX=0, out=None):
        """x: cuda float32 [N][D] -> cuda float32 [N][D]"""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.D
        if out is None:
            out = torch.empty_like(x)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == x.shape
        check(_core._lib.dsr_stc_apply(self.h, _dev(x), x.shape[0], int(estX), _dev(out), cur_stream()))
        return out

    def set_timing(self, on=True):
        check(_core._lib.dsr_stc_set_timing(self.h, int(on)))


class Lda(_Estimators):
    """LDA matrices for nEst estimators over one Gmm (csrc/k_stc.hip, csrc/stc.cpp; include/dsr.h section 12): the three scatter matrices on
    fp64 MFMA, the simultaneous diagonalisation by Jacobi on the device.  globalGmm: a Gmm whose codebook 0 is the global codebook.  Made
    from two Gmms, as a bare transformer (dimN=), or around the handle an LDATransformer stream owns (handle=, owner=)."""

    _destroy = "dsr_lda_destroy"

    def __init__(self, gmm=None, globalGmm=None, nEst=1, dimN=None, handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle
        elif gmm is not None:
            self._create(L.dsr_lda_create, gmm.h, globalGmm.h, int(nEst))
        else:
            self._create(L.dsr_lda_create_transformer, int(dimN))
        self.gmm, self.globalGmm = gmm, globalGmm; self.D = L.dsr_lda_dim(self.h); self.nEst = L.dsr_lda_num_estimators(self.h); self._kernel_ms = L.dsr_lda_kernel_ms

    def accumulate(self, xScore, frame, dist, factor, est, xSrc=None, want_nearest=False):
        return self._items(_core._lib.dsr_lda_accumulate, xScore, frame, dist, factor, est, xSrc, want_nearest)

    def accumulate_path(self, xScore, distIds, estX=0, factor=1.0, xSrc=None):
        """-> the summed score of the path's distributions"""
        xScore, xSrc = self._frames(xScore, xSrc); ids = _np(distIds, np.int32); s = C.c_double(0.0)
        check(_core._lib.dsr_lda_accumulate_path(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(ids), len(ids), int(estX), float(factor), C.byref(s), cur_stream()))
        return s.value

    def zero(self, estX=0):
        check(_core._lib.dsr_lda_zero(self.h, int(estX)))

    def get_accu(self, estX=0, through_accessor=False):
        """-> dict(count, within, between, mixture [D][D])"""
        D = self.D; c = C.c_double(0.0); W = np.zeros((D, D)); B = np.zeros((D, D)); M = np.zeros((D, D))
        check(_core._lib.dsr_lda_get_accu(self.h, int(estX), int(bool(through_accessor)), C.byref(c), _ptr(W), _ptr(B), _ptr(M)))
        return dict(count=c.value, within=W, between=B, mixture=M)

    def set_accu(self, estX=0, count=None, within=None, between=None, mixture=None):
        D = self.D; m = [self._mat(x, (D, D)) if x is not None else None for x in (within, between, mixture)]
        check(_core._lib.dsr_lda_set_accu(self.h, int(estX), C.byref(C.c_double(float(count))) if count is not None else None,
                                    *[_ptr(x) if x is not None else None for x in m]))

    def save_accu(self, fileName, estX=0):
        check(_core._lib.dsr_lda_save_accu(self.h, fileName.encode(), int(estX)))

    def load_accu(self, fileName, estX=0):
        check(_core._lib.dsr_lda_load_accu(self.h, fileName.encode(), int(estX)))

    def estimate(self, estX=0):
        e = _np(np.atleast_1d(estX), np.int32)
        check(_core._lib.dsr_lda_estimate(self.h, _ptr(e), len(e), cur_stream()))

    def status(self, estX=0):
        return _core._lib.dsr_lda_status(self.h, int(estX))

    def eigenvalues(self, estX=0):
        """-> (eigenvalues of within as found, eigenvalues of the whitened between, descending) of the last estimate"""
        w = np.zeros(self.D); b = np.zeros(self.D); check(_core._lib.dsr_lda_eigenvalues(self.h, int(estX), _ptr(w), _ptr(b))); return w, b

    def transform(self, estX=0):
        L = np.zeros((self.D, self.D)); check(_core._lib.dsr_lda_get_transform(self.h, int(estX), _ptr(L))); return L

    def set_transform(self, L, estX=0):
        check(_core._lib.dsr_lda_set_transform(self.h, int(estX), _ptr(self._mat(L, (self.D, self.D)))))

    def save(self, fileName, estX=0):
        check(_core._lib.dsr_lda_save(self.h, fileName.encode(), int(estX)))

    def load(self, fileName, estX=0):
        check(_core._lib.dsr_lda_load(self.h, fileName.encode(), int(estX)))

    def apply(self, x, outDim=None, estX=0, out=None):
        """x: cuda float32 [N][D] -> cuda float32 [N][outDim]: the first outDim rows of the matrix"""
        outDim = self.D if outDim is None else int(outDim)
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.D
        if out is None:
            out = torch.empty((x.shape[0], outDim), dtype=torch.float32, device=x.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (x.shape[0], outDim)
        check(_core._lib.dsr_lda_apply(self.h, _dev(x), x.shape[0], int(estX), outDim, _dev(out), cur_stream()))
        return out

    def set_timing(self, on=True):
        check(_core._lib.dsr_lda_set_timing(self.h, int(on)))
