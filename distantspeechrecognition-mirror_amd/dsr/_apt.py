"""All-pass transform speaker adaptation through the C-ABI (include/dsr.h section 13): the RAPT / SLAPT parameters of a speaker and their text
files, the line search, and the handle that estimates and applies the bilinear transform (BLT) or the sine-log all-pass transform (SLAPT) of
the cepstral means for S speakers at once.  Built on dsr._capi._core (the common handle base); dsr._capi re-exports AptParams, Apt,
apt_line_search and the constants.  Importing this module imports neither torch nor the library."""
import ctypes as C

import numpy as np

from ._capi import _core
from ._capi._core import DsrError, Handle, check, cur_stream, load, torch, vp, E_INDEX, _np, _ptr, _dev


class AptParams(Handle):
    """The RAPT or SLAPT parameters of one speaker (asr/adapt/transform.cc:410-551, 862-896; include/dsr.h section 13).  Host only."""

    _destroy = "dsr_apt_params_destroy"

    def __init__(self, fileName="", handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle; return
        self._create(L.dsr_apt_params_create, fileName.encode())

    def clear(self):
        check(_core._lib.dsr_apt_params_clear(self.h))

    def read(self, fileName):
        check(_core._lib.dsr_apt_params_read(self.h, fileName.encode()))

    def write(self, fileName):
        check(_core._lib.dsr_apt_params_write(self.h, fileName.encode()))

    def copy_from(self, other):
        check(_core._lib.dsr_apt_params_copy(self.h, other.h))

    def type(self):
        return _core._lib.dsr_apt_params_type(self.h)

    def indices(self):
        n = _core._lib.dsr_apt_params_indices(self.h, None, 0); a = np.zeros(n, np.uint32)
        _core._lib.dsr_apt_params_indices(self.h, _ptr(a), n); return [int(x) for x in a]

    def findAPT(self, rc, typ, useAncestor=True):
        """-> (conf float64, bias float32) of the class, inserted as a copy of its nearest ancestor when missing"""
        nc = C.c_int(0); nb = C.c_int(0)
        check(_core._lib.dsr_apt_params_find(self.h, int(rc), int(typ), int(useAncestor), C.byref(nc), C.byref(nb)))
        conf = np.zeros(nc.value); bias = np.zeros(nb.value, np.float32)
        check(_core._lib.dsr_apt_params_get(self.h, int(rc), _ptr(conf), _ptr(bias))); return conf, bias

    def set(self, rc, typ, conf, bias=()):
        conf = _np(np.atleast_1d(conf), np.float64); bias = _np(np.atleast_1d(bias), np.float32)
        check(_core._lib.dsr_apt_params_set(self.h, int(rc), int(typ), len(conf), _ptr(conf), len(bias), _ptr(bias)))


def apt_line_search(kind, lhood):
    """EstimatorBase::bracket + brentsMethod replayed on the values found so far -> (state, point, points): state 0 needs `point`, 1 done
    at `point`, 2 failed"""
    load(); v = _np(np.atleast_1d(lhood), np.float64) if len(lhood) else np.zeros(0); st = C.c_int(0); x = C.c_double(0.0); n = C.c_int(0)
    pts = np.zeros(len(v) + 1)
    check(_core._lib.dsr_apt_line_search(int(kind), _ptr(v) if len(v) else None, len(v), C.byref(st), C.byref(x), C.byref(n), _ptr(pts)))
    return st.value, x.value, pts[:n.value]


def apt_transform_rows(kind, subFeatLen, nSubFeat, conf, bias=(), rows=None):
    """a transformer on its own: -> (A [subFeatLen][subFeatLen], the transformed rows float32 [N][subFeatLen nSubFeat]), both made on the device"""
    load(); conf = _np(np.atleast_1d(conf), np.float64); bias = _np(np.atleast_1d(bias), np.float32); D = int(subFeatLen) * int(nSubFeat)
    rows = np.zeros((0, D), np.float32) if rows is None else _np(np.atleast_2d(rows), np.float32); assert rows.shape[1] == D
    A = np.zeros((int(subFeatLen), int(subFeatLen))); out = np.zeros_like(rows)
    check(_core._lib.dsr_apt_transform_rows(int(kind), int(subFeatLen), int(nSubFeat), len(conf), _ptr(conf), len(bias), _ptr(bias), _ptr(rows), len(rows),
                                          _ptr(A), _ptr(out)))
    return A, out


APT_RAPT, APT_SLAPT = 1, 2
APT_BIAS = {"NONE": 0, "None": 0, None: 0, "CEPSTRAONLY": 1, "CepstraOnly": 1, "ALLCOMPONENTS": 2, "AllComponents": 2}


class Apt(Handle):
    """All-pass transform adaptation of the means for S speakers at once (csrc/apt_kernels.hip, csrc/apt.cpp; include/dsr.h section 13): the
    bilinear transform (kind APT_RAPT) or the sine-log all-pass transform (APT_SLAPT), one estimated parameter per regression class.  Series
    and matrices, likelihoods and the transformed means on the device; the line searches on the host, one round of launches for all of them."""

    _destroy = "dsr_apt_destroy"

    def __init__(self, gmm, S=1, kind=APT_SLAPT, subFeatLen=None, nSubFeat=1, biasType=0):
        L = load(); self.gmm = gmm; self.D = gmm.D; self.G = gmm.G; self.kind = int(kind); self.nSub = int(nSubFeat)
        self.L = int(subFeatLen) if subFeatLen is not None else gmm.D // self.nSub
        bt = APT_BIAS[biasType] if not isinstance(biasType, int) else biasType
        self._create(L.dsr_apt_create, gmm.h, int(S), self.kind, self.L, self.nSub, int(bt)); self.S = L.dsr_apt_num_speakers(self.h)
        self.bSize = (0, self.L, self.D)[bt]

    def set_param_n(self, paramN):
        check(_core._lib.dsr_apt_set_param_n(self.h, int(paramN)))

    def set_stats(self, s, trainer=None, c=None, sumO=None):
        """the statistics of slot s: a Trainer (count - denCount and sumO, device to device) or host arrays c [G], sumO [G][D]"""
        if trainer is not None:
            check(_core._lib.dsr_apt_set_stats(self.h, int(s), trainer.h)); return
        c = _np(c, np.float64); sumO = _np(sumO, np.float64); assert c.shape == (self.G,) and sumO.shape == (self.G, self.D)
        check(_core._lib.dsr_apt_set_stats_arrays(self.h, int(s), _ptr(c), _ptr(sumO)))

    def store(self, s):
        h = _core._lib.dsr_apt_store(self.h, int(s))
        if not h:
            raise DsrError(E_INDEX, "speaker %d of %d" % (s, self.S))
        return AptParams(handle=vp(h), owner=self)

    def set_params(self, s, rc, conf, bias=()):
        conf = _np(np.atleast_1d(conf), np.float64); bias = _np(np.atleast_1d(bias), np.float32)
        check(_core._lib.dsr_apt_set_params(self.h, int(s), int(rc), len(conf), _ptr(conf), len(bias), _ptr(bias)))

    def get_params(self, s, rc):
        """-> (conf float64, bias float32)"""
        nc = C.c_int(0); nb = C.c_int(0); check(_core._lib.dsr_apt_get_params(self.h, int(s), int(rc), C.byref(nc), None, C.byref(nb), None))
        conf = np.zeros(nc.value); bias = np.zeros(nb.value, np.float32)
        check(_core._lib.dsr_apt_get_params(self.h, int(s), int(rc), C.byref(nc), _ptr(conf), C.byref(nb), _ptr(bias))); return conf, bias

    def estimate(self, threshold=1500.0):
        check(_core._lib.dsr_apt_estimate(self.h, float(threshold), cur_stream()))

    def speaker_status(self, s):
        return _core._lib.dsr_apt_speaker_status(self.h, int(s))

    def rounds(self):
        return _core._lib.dsr_apt_rounds(self.h)

    def plan(self):
        """the steps of the last estimate: rows (speaker, node, leaf)"""
        n = C.c_int(0); check(_core._lib.dsr_apt_get_plan(self.h, C.byref(n), None))
        a = np.zeros((n.value, 3), np.int32); check(_core._lib.dsr_apt_get_plan(self.h, C.byref(n), _ptr(a))); return a

    def nodes(self):
        n = C.c_int(0); check(_core._lib.dsr_apt_get_nodes(self.h, C.byref(n), None, None))
        a = np.zeros(n.value, np.uint32); leaf = np.zeros(n.value, np.int32); check(_core._lib.dsr_apt_get_nodes(self.h, C.byref(n), _ptr(a), _ptr(leaf)))
        return [int(x) for x in a], [bool(x) for x in leaf]

    def ttl_frames(self, s, node):
        t = C.c_double(0.0); check(_core._lib.dsr_apt_ttl_frames(self.h, int(s), int(node), C.byref(t))); return t.value

    def trace(self, s, node):
        """-> (points, logLhoods, biases [n][bias size]) the last estimate evaluated for (slot, node), in order"""
        n = C.c_int(0); check(_core._lib.dsr_apt_get_trace(self.h, int(s), int(node), C.byref(n), None, None, None))
        x = np.zeros(n.value); v = np.zeros(n.value); b = np.zeros((n.value, self.bSize), np.float32)
        check(_core._lib.dsr_apt_get_trace(self.h, int(s), int(node), C.byref(n), _ptr(x), _ptr(v), _ptr(b))); return x, v, b

    def matrix(self, s, rc):
        A = np.zeros((self.L, self.L)); check(_core._lib.dsr_apt_get_matrix(self.h, int(s), int(rc), _ptr(A))); return A

    def write(self, s, fileName):
        check(_core._lib.dsr_apt_write(self.h, int(s), fileName.encode()))

    def read(self, s, fileName):
        check(_core._lib.dsr_apt_read(self.h, int(s), fileName.encode()))

    def adapt(self, s, target=None):
        check(_core._lib.dsr_apt_adapt(self.h, int(s), (target or self.gmm).h))

    def adapt_all(self, out=None):
        """-> cuda float32 [S][G][D]: every speaker's transformed means"""
        if out is None:
            out = torch.empty((self.S, self.G, self.D), dtype=torch.float32, device="cuda")
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (self.S, self.G, self.D)
        check(_core._lib.dsr_apt_adapt_all(self.h, _dev(out), cur_stream())); return out

    def reset_mean(self, target=None):
        check(_core._lib.dsr_apt_reset_mean(self.h, (target or self.gmm).h))

    def set_timing(self, on=True):
        check(_core._lib.dsr_apt_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 3)(); check(_core._lib.dsr_apt_kernel_ms(self.h, ms)); return ms[0], ms[1], ms[2]
