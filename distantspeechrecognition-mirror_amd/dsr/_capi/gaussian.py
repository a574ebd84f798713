"""asr/gaussian and asr/train: the GMM and its training."""
import ctypes as C

import numpy as np

from . import _core
from ._core import (Handle, check, cur_stream, load, torch, _np, _ptr, _dev)


class Gmm(Handle):
    _destroy = "dsr_gmm_destroy"

    def __init__(self, refN=None, mean=None, ivar=None, det=None, val=None, scale=None, files=None):
        L = load()
        if files is not None:
            self._create(L.dsr_gmm_load, files[0].encode(), files[1].encode())
        else:
            r = _np(refN, np.int32); m = _np(mean, np.float32); iv = _np(ivar, np.float32); d = _np(det, np.float32); v = _np(val, np.float32)
            s = _np(scale, np.float32) if scale is not None else None
            self._create(L.dsr_gmm_create, len(r), m.shape[1], _ptr(r), _ptr(m), _ptr(iv), _ptr(d), _ptr(v), _ptr(s) if s is not None else None)
        self.K = L.dsr_gmm_num_dists(self.h); self.D = L.dsr_gmm_dim(self.h)

    def save(self, cbFile, dsFile):
        check(_core._lib.dsr_gmm_save(self.h, cbFile.encode(), dsFile.encode()))

    def score(self, x, mode=0, want_argmin=True):
        """x: cuda float32 [N][D] -> (score [N][K] float32, argmin [N][K] uint8)"""
        N = x.shape[0]
        sc = torch.empty((N, self.K), dtype=torch.float32, device=x.device)
        am = torch.zeros((N, self.K), dtype=torch.uint8, device=x.device) if want_argmin and mode != 1 else None
        check(_core._lib.dsr_gmm_score(self.h, _dev(x), N, mode, _dev(sc), _dev(am) if am is not None else None, cur_stream()))
        return sc, am

    @property
    def G(self):
        return _core._lib.dsr_gmm_num_gaussians(self.h)

    def set_reg_classes(self, classes):
        """one regression class per Gaussian [G], or one class for every Gaussian (CodebookSetBasic::setRegClasses)"""
        if np.isscalar(classes):
            check(_core._lib.dsr_gmm_set_reg_class_all(self.h, int(classes)))
        else:
            c = _np(classes, np.uint16); assert c.shape == (self.G,)
            check(_core._lib.dsr_gmm_set_reg_classes(self.h, _ptr(c)))

    def reg_classes(self):
        """the classes [G] (0 where there is none), or None for a model without the table"""
        c = np.zeros(self.G, np.uint16); present = C.c_int(0)
        check(_core._lib.dsr_gmm_get_reg_classes(self.h, _ptr(c), C.byref(present)))
        return c if present.value else None

    def params(self):
        """the model's host parameters as the training updates left them: refN [K], mean, cv [G][D], det, val, count [G]"""
        r = np.zeros(self.K, np.int32); check(_core._lib.dsr_gmm_get_params(self.h, _ptr(r), None, None, None, None, None))
        G = int(r.sum())
        d = dict(refN=r, mean=np.zeros((G, self.D), np.float32), cv=np.zeros((G, self.D), np.float32), det=np.zeros(G, np.float32),
                 val=np.zeros(G, np.float32), count=np.zeros(G, np.float32))
        check(_core._lib.dsr_gmm_get_params(self.h, None, *[_ptr(d[k]) for k in ("mean", "cv", "det", "val", "count")]))
        return d


class Trainer(Handle):
    """CodebookSetTrain + DistribSetTrain over one Gmm (asr/train/codebookTrain.cc, distribTrain.cc; include/dsr.h section 9): accumulation on
    the device, updates and accumulator files on the host.  The Gmm is changed by update / split and must outlive the trainer (kept here)."""

    NAMES = ("count", "den", "sumO", "sumOsq", "dcount", "dden")

    _destroy = "dsr_train_destroy"

    def __init__(self, gmm, massThreshold=5.0):
        L = load(); self.gmm = gmm
        self._create(L.dsr_train_create, gmm.h, float(massThreshold))

    @property
    def G(self):
        return _core._lib.dsr_train_num_gaussians(self.h)

    def zero(self, what=3, nParts=1, part=1):
        check(_core._lib.dsr_train_zero(self.h, int(what), int(nParts), int(part)))

    def accumulate(self, x, frame, dist, factor, want_score=True):
        """x: cuda float32 [N][D]; frame, dist, factor: host arrays [M] -> float32 scores [M] (or None)"""
        fr = _np(frame, np.int32); ds = _np(dist, np.int32); fa = _np(factor, np.float32); M = len(fr)
        assert len(ds) == M and len(fa) == M and x.dtype.is_floating_point and x.element_size() == 4 and x.is_contiguous() and x.shape[1] == self.gmm.D
        sc = np.zeros(M, np.float32) if want_score else None
        check(_core._lib.dsr_train_accumulate(self.h, _dev(x), x.shape[0], _ptr(fr), _ptr(ds), _ptr(fa), M, _ptr(sc) if want_score else None, cur_stream()))
        return sc

    def accumulate_path(self, x, distIds, factor=1.0):
        ids = _np(distIds, np.int32); s = C.c_double(0.0)
        assert x.is_contiguous() and x.shape[1] == self.gmm.D and x.shape[0] >= len(ids)
        check(_core._lib.dsr_train_accumulate_path(self.h, _dev(x), len(ids), _ptr(ids), float(factor), C.byref(s), cur_stream()))
        return s.value

    def accumulate_lattice(self, lattice, x, factor=1.0):
        """lattice: a Lattice (after gammaProbs) -> the number of links accumulated"""
        n = C.c_uint(0); assert x.is_contiguous() and x.shape[1] == self.gmm.D
        check(_core._lib.dsr_train_accumulate_lattice(self.h, lattice.h, _dev(x), x.shape[0], float(factor), C.byref(n), cur_stream()))
        return n.value

    def get(self):
        G, D = self.G, self.gmm.D
        d = dict(count=np.zeros(G), den=np.zeros(G), sumO=np.zeros((G, D)), sumOsq=np.zeros((G, D)), dcount=np.zeros(G), dden=np.zeros(G))
        check(_core._lib.dsr_train_get(self.h, *[_ptr(d[k]) for k in self.NAMES]))
        return d

    def set(self, **kw):
        G, D = self.G, self.gmm.D; a = []
        for k in self.NAMES:
            v = kw.get(k)
            if v is not None:
                v = _np(v, np.float64); assert v.shape == ((G, D) if k in ("sumO", "sumOsq") else (G,)), k
            a.append(v)
        check(_core._lib.dsr_train_set(self.h, *[_ptr(v) if v is not None else None for v in a]))

    def add(self, other, factor=1.0):
        check(_core._lib.dsr_train_add(self.h, other.h, float(factor)))

    def save_codebook_accus(self, fileName, totalPr=0.0, totalT=0, countsOnly=False):
        check(_core._lib.dsr_train_save_codebook_accus(self.h, fileName.encode(), float(totalPr), int(totalT), int(countsOnly)))

    def load_codebook_accus(self, fileName, factor=1.0, nParts=1, part=1):
        pr = C.c_float(0.0); tt = C.c_uint(0)
        check(_core._lib.dsr_train_load_codebook_accus(self.h, fileName.encode(), C.byref(pr), C.byref(tt), float(factor), int(nParts), int(part)))
        return pr.value, tt.value

    def save_distrib_accus(self, fileName):
        check(_core._lib.dsr_train_save_distrib_accus(self.h, fileName.encode()))

    def load_distrib_accus(self, fileName, factor=1.0, nParts=1, part=1):
        check(_core._lib.dsr_train_load_distrib_accus(self.h, fileName.encode(), float(factor), int(nParts), int(part)))

    def update(self, what=3, nParts=1, part=1):
        check(_core._lib.dsr_train_update(self.h, int(what), int(nParts), int(part)))

    def update_mmi(self, what=3, E=1.0, merialdo=False, nParts=1, part=1):
        check(_core._lib.dsr_train_update_mmi(self.h, int(what), float(E), int(merialdo), int(nParts), int(part)))

    def floor_variances(self, nParts=1, part=1):
        t = C.c_uint(0); f = C.c_uint(0)
        check(_core._lib.dsr_train_floor_variances(self.h, int(nParts), int(part), C.byref(t), C.byref(f)))
        return t.value, f.value

    def fix_gconsts(self, nParts=1, part=1):
        check(_core._lib.dsr_train_fix_gconsts(self.h, int(nParts), int(part)))

    def invert_variances(self, nParts=1, part=1):
        check(_core._lib.dsr_train_invert_variances(self.h, int(nParts), int(part)))

    def split(self, distX, minCount=0.0, splitFactor=0.2):
        r = C.c_uint(0); check(_core._lib.dsr_train_split(self.h, int(distX), float(minCount), float(splitFactor), C.byref(r)))
        return r.value

    def set_timing(self, on=True):
        check(_core._lib.dsr_train_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 2)(); check(_core._lib.dsr_train_kernel_ms(self.h, ms)); return ms[0], ms[1]
