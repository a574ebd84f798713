"""Sample-rate conversion through the C-ABI (include/dsr.h section 6d): band-limited interpolation with a Kaiser-windowed sinc ("fastest", "medium",
"best"), zero-order hold and linear interpolation for a batch [U][C][samples], one-shot or block by block with carried state.  It stands for the
reference's SamplerateConversionFeature, a libsamplerate wrapper, and does not reproduce libsamplerate's bits.  Built on dsr._capi._core (the
common handle base); dsr._capi re-exports SampleRateConverter.  Importing this module imports neither torch nor the library."""
import ctypes as C

import numpy as np

from ._capi import _core
from ._capi._core import DsrError, Handle, check, cur_stream, load, torch, _dev, _state

SRC_TABLE_LDS, SRC_TABLE_MEM, SRC_TABLE_UNIFORM, SRC_TABLE_NONE = 0, 1, 2, 3
SRC_INPUT_LDS, SRC_INPUT_DIRECT = 0, 1
SRC_TABLE_NAMES = ("lds", "mem", "uniform", "none")


class SampleRateConverter(Handle):
    """One ratio and one method.  apply() is the one-shot call; state() makes the carried state block() continues from."""

    _destroy = "dsr_src_destroy"

    def __init__(self, srcRate, dstRate, method="fastest"):
        L = load()
        self.srcRate, self.dstRate, self.method = int(srcRate), int(dstRate), method
        if self.srcRate < 0 or self.dstRate < 0:
            raise DsrError(_core.E_PARAMETER, "sample rates must be positive (%d -> %d)" % (self.srcRate, self.dstRate))
        self._create(L.dsr_src_create, self.srcRate, self.dstRate, method.encode() if isinstance(method, str) else method)
        r = (C.c_int32 * 3)(); check(L.dsr_src_ratio(self.h, r))
        self.L, self.M, self.K = tuple(r)

    def out_samples(self, nIn):
        """floor(nIn L / M)"""
        return int(_core._lib.dsr_src_out_samples(self.h, int(nIn)))

    def block_out_bound(self, nIn):
        """the most outputs one block of nIn samples can release"""
        return int(_core._lib.dsr_src_block_out_bound(self.h, int(nIn)))

    def table(self):
        """the fp32 table [L][2K] of a sinc method, row p = phase p"""
        t = np.zeros((self.L, 2 * self.K), np.float32); check(_core._lib.dsr_src_table(self.h, t.ctypes.data_as(C.c_void_p)))
        return t

    def path(self):
        """-> (table, input, outputs of a tile, dynamic LDS, lane pitch): the cell apply takes now (DSR_SRC_TABLE=mem is read on every call); needs no device"""
        p = (C.c_int32 * 5)(); check(_core._lib.dsr_src_path(self.h, p))
        return tuple(p)

    def state(self, U, C_, device):
        """a zeroed carried state for U utterances of C_ channels; the handle notes the shape"""
        st = _state(int(_core._lib.dsr_src_state_bytes(self.h, U, C_)), device)
        check(_core._lib.dsr_src_state_init(self.h, _dev(st), U, C_, cur_stream()))
        return st

    def set_timing(self, on=True):
        check(_core._lib.dsr_src_set_timing(self.h, int(bool(on))))

    def kernel_ms(self):
        ms = C.c_double(); check(_core._lib.dsr_src_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def _call(self, x, nsamp, state, flush, y, outStride):
        if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
            raise DsrError(_core.E_DIMENSION, "x must be contiguous float32 [U][C][samples]")
        U, Cn, N = x.shape
        if nsamp is not None and (nsamp.dtype != torch.int32 or nsamp.numel() != U or not nsamp.is_contiguous()):
            raise DsrError(_core.E_DIMENSION, "nsamp must be int32 [%d]" % U)
        if y is None:
            y = torch.empty((U, Cn, outStride), dtype=torch.float32, device=x.device)
        elif y.dim() != 3 or tuple(y.shape[:2]) != (U, Cn) or y.dtype != torch.float32 or not y.is_contiguous():
            raise DsrError(_core.E_DIMENSION, "y must be contiguous float32 [%d][%d][samples]" % (U, Cn))
        nout = torch.zeros((U,), dtype=torch.int32, device=x.device)
        check(_core._lib.dsr_src_apply(self.h, _dev(x), _dev(nsamp) if nsamp is not None else None, U, Cn, N, _dev(state) if state is not None else None,
                                       int(bool(flush)), _dev(y), _dev(nout), y.shape[2], cur_stream()))
        return y, nout

    def apply(self, x, nsamp=None, y=None):
        """x cuda float32 [U][C][N], nsamp cuda int32 [U] (None: N each) -> (y [U][C][floor(N L / M)], nout int32 [U]); a row is zero past its count"""
        return self._call(x, nsamp, None, True, y, self.out_samples(x.shape[2]))

    def block(self, state, x, nsamp=None, flush=False, y=None):
        """the next block of every stream of `state` -> (y [U][C][block_out_bound(N)], nout): the outputs this block releases"""
        return self._call(x, nsamp, state, flush, y, self.block_out_bound(x.shape[2]))
