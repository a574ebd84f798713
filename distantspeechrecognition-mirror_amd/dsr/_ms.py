"""Multi-stream decoding through the C-ABI (include/dsr.h section 8b): DistribMap (asr/gaussian/distribBasic.h:390-408) and the combiner of two
models' score matrices, DistribMultiStream::_score (distribBasic.h:148-152) for every (frame, state) at once.  Built on dsr._capi._core; importing
this module imports neither torch nor the library."""
import ctypes as C

import numpy as np

from ._capi import _core
from ._capi._core import DsrError, Handle, check, cur_stream, load, torch, _ptr, _dev

VECTOR_LDS, SCALAR_LDS, GATHER = 0, 1, 2
LDS_BUDGET = 32768                                     # DSR_MS_LDS_BUDGET


def combine_path(KA, KV, aligned16=True):
    """-> (path, rowsPerTile, ldsBytes) of the kernel a combine of these shapes launches; needs no device"""
    p, r, b = C.c_int(), C.c_int(), C.c_int64()
    check(load().dsr_ms_combine_path(int(KA), int(KV), int(bool(aligned16)), C.byref(p), C.byref(r), C.byref(b)))
    return p.value, r.value, b.value


class DistribMap(Handle):
    """names of the first model -> names of the second; host only"""

    _destroy = "dsr_distribmap_destroy"

    def __init__(self, pairs=None):
        self._create(load().dsr_distribmap_create)
        for f, t in (pairs.items() if hasattr(pairs, "items") else pairs or ()):
            self.add(f, t)

    def add(self, fromName, toName):
        check(_core._lib.dsr_distribmap_add(self.h, fromName.encode(), toName.encode()))

    def mapped(self, name):
        to = C.c_char_p(); check(_core._lib.dsr_distribmap_mapped(self.h, name.encode(), C.byref(to))); return to.value.decode()

    def __len__(self):
        return _core._lib.dsr_distribmap_size(self.h)

    def read(self, fileName):
        check(_core._lib.dsr_distribmap_read(self.h, str(fileName).encode()))

    def write(self, fileName):
        check(_core._lib.dsr_distribmap_write(self.h, str(fileName).encode()))


class MultiStream(Handle):
    """The combiner of two Gmm models: out[n][k] = float(audioWeight * double(sA[n][k]) + videoWeight * double(sV[n][table[k]])), table[k] the
    video state named like audio state k, or like mapping.mapped(name of k)."""

    _destroy = "dsr_ms_destroy"

    def __init__(self, gmmA, gmmV, mapping=None, audioWeight=0.95, videoWeight=0.05):
        L = load(); self.gmmA, self.gmmV, self.mapping = gmmA, gmmV, mapping
        self._create(L.dsr_ms_create, gmmA.h, gmmV.h, mapping.h if mapping is not None else None, float(audioWeight), float(videoWeight))
        self.KA, self.KV = gmmA.K, gmmV.K

    def setWeights(self, audioWeight, videoWeight):
        check(_core._lib.dsr_ms_set_weights(self.h, float(audioWeight), float(videoWeight)))

    def weights(self):
        a, v = C.c_double(), C.c_double(); check(_core._lib.dsr_ms_get_weights(self.h, C.byref(a), C.byref(v))); return a.value, v.value

    @property
    def table(self):
        """the resolved video state index of every audio state, int32 [KA]"""
        t = np.zeros(self.KA, np.int32); check(_core._lib.dsr_ms_table(self.h, _ptr(t))); return t

    def path(self, aligned16=True):
        return combine_path(self.KA, self.KV, aligned16)

    def combine(self, sA, sV, out=None):
        """sA: cuda float32 [N][KA], sV: [N][KV] -> out [N][KA] (a new tensor; out=sA combines in place).  sV may hold more rows than sA; all three are
        contiguous, and any 4-byte alignment is accepted (16-byte aligned sA and out take the vector path)."""
        if sA.dtype != torch.float32 or sV.dtype != torch.float32 or sA.dim() != 2 or sV.dim() != 2:
            raise DsrError(5, "the score matrices are float32 [N][K]")
        if sA.shape[1] != self.KA or sV.shape[1] != self.KV or sV.shape[0] < sA.shape[0]:
            raise DsrError(5, "score matrices of %s and %s for %d and %d states" % (tuple(sA.shape), tuple(sV.shape), self.KA, self.KV))
        if not sA.is_contiguous() or not sV.is_contiguous():
            raise DsrError(5, "the score matrices must be contiguous")
        if out is None:
            out = torch.empty_like(sA)
        elif out.shape != sA.shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise DsrError(5, "out must be a contiguous float32 tensor shaped like sA")
        if sA.shape[0]:
            check(_core._lib.dsr_ms_combine(self.h, _dev(sA), _dev(sV), sA.shape[0], _dev(out), cur_stream()))
        return out

    def score(self, xA, xV, modeA=0, modeV=0):
        """xA: cuda float32 [N][dimA], xV: [N'][dimV] features -> the combined costs of the first min(N, N') frames, [min][KA]: both models scored
        on the device, combined in place"""
        N = min(xA.shape[0], xV.shape[0])
        sA = self.gmmA.score(xA[:N].contiguous(), mode=modeA, want_argmin=False)[0]
        sV = self.gmmV.score(xV[:N].contiguous(), mode=modeV, want_argmin=False)[0]
        return self.combine(sA, sV, out=sA)
