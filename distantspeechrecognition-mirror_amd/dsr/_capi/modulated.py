"""btk/modulated: the filter banks and what they carry between blocks."""

import numpy as np

from . import _core
from ._core import (DsrError, Handle, check, cur_stream, load, torch, E_DIMENSION, _np, _ptr, _dev, _counts)


class FilterBank(Handle):
    """OverSampledDFTAnalysisBank / OverSampledDFTSynthesisBank plan (btk/modulated/modulated.h:291-360)."""

    _destroy = "dsr_fb_destroy"

    def __init__(self, prototype, M, m, r, synthesis=False, delayCompensationType=0, gainFactor=1):
        L = load()
        p = _np(prototype, np.float64)
        if p.size != M * m:
            raise DsrError(4, "Prototype sizes do not match (%d vs. %d)." % (p.size, M * m))   # modulated.cc:268-270
        self._create(L.dsr_fb_create, _ptr(p), M, m, r, int(synthesis), delayCompensationType, gainFactor)
        self.M, self.m, self.r, self.D, self.synthesis = M, m, r, M >> r, synthesis
        self.pd = L.dsr_fb_processing_delay(self.h)
        self.laN = (m << r) // 2 - 1 if (delayCompensationType == 2 and not synthesis) else 0      # look-ahead in blocks of D (modulated.cc:289)

    def frames(self, nsamp):
        return _core._lib.dsr_fb_analysis_frames(self.h, int(nsamp))

    def blocks(self, nframes):
        return _core._lib.dsr_fb_synthesis_blocks(self.h, int(nframes))

    def analysis(self, x, nsamp=None):
        """x: cuda float32 [U][C][N] -> complex64 [U][C][Tmax][M/2+1]"""
        U, Cn, N = x.shape
        nsamp = _counts(nsamp, U, N, x.device)
        Tmax = max(1, max(self.frames(int(n)) for n in nsamp.tolist()))
        X = torch.empty((U, Cn, Tmax, self.M // 2 + 1, 2), dtype=torch.float32, device=x.device)
        check(_core._lib.dsr_fb_analysis(self.h, _dev(x), _dev(nsamp), U, Cn, N, Tmax, _dev(X), cur_stream()))
        return torch.view_as_complex(X)

    def analysis_beamform(self, bf, x, nsamp=None):
        """analysis bank + fixed-weight beamformer in one pass (dsr_fb_analysis_beamform): x cuda float32 [U][C][N] -> complex64 [U][Tmax][M/2+1]"""
        U, Cn, N = x.shape
        nsamp = _counts(nsamp, U, N, x.device)
        Tmax = max(1, max(self.frames(int(n)) for n in nsamp.tolist()))
        Y = torch.empty((U, Tmax, self.M // 2 + 1, 2), dtype=torch.float32, device=x.device)
        check(_core._lib.dsr_fb_analysis_beamform(self.h, bf.h, _dev(x), _dev(nsamp), U, Cn, N, Tmax, _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)

    def analysis_beamform_supported(self, bf):
        return bool(_core._lib.dsr_fb_analysis_beamform_supported(self.h, bf.h))

    def synthesis_run(self, Y, nframes=None):
        """Y: cuda complex64 [U][Tmax][M/2+1] -> float32 [U][nblocks*D]"""
        U, Tmax, F = Y.shape
        nframes = _counts(nframes, U, Tmax, Y.device)
        nb = max(1, max(self.blocks(int(n)) for n in nframes.tolist()))
        y = torch.zeros((U, nb * self.D), dtype=torch.float32, device=Y.device)
        Yr = torch.view_as_real(Y.contiguous())
        check(_core._lib.dsr_fb_synthesis(self.h, _dev(Yr), _dev(nframes), U, Tmax, nb * self.D, _dev(y), cur_stream()))
        return y


class FilterBankState(Handle):
    """what a filter bank carries from one block of a long stream to the next (dsr_fb_state): m*M - D samples per (stream, channel) for an
    analysis plan, R*m - 1 subband frames per stream for a synthesis plan."""

    _destroy = "dsr_fb_state_destroy"

    def __init__(self, fb, U, C=1):
        L = load(); self.fb, self.U, self.C = fb, U, C
        self._started = False
        self._create(L.dsr_fb_state_create, fb.h, U, C)

    def reset(self):
        check(_core._lib.dsr_fb_state_reset(self.h))
        self._started = False

    def analysis_block(self, x, nsamp=None, last=False):
        """x: cuda float32 [U][C][N] = the block's new samples -> complex64 [U][C][T][M/2+1], T = the frames this block yields"""
        U, Cn, N = x.shape
        ns = [N] * U if nsamp is None else [int(v) for v in nsamp]
        # include/dsr.h: the look-ahead of delayCompensationType 2 is spent inside a stream's first block, which must hold it
        if not self._started and not last and min(ns) < self.fb.laN * self.fb.D:
            raise DsrError(E_DIMENSION, "the first block of a stream must hold at least %d samples (the look-ahead)" % (self.fb.laN * self.fb.D))
        self._started = True
        nd = torch.tensor(ns, dtype=torch.int32, device=x.device)
        T = max(1, max(_core._lib.dsr_fb_analysis_block_frames(self.fb.h, self.h, n, int(last)) for n in ns))
        X = torch.empty((U, Cn, T, self.fb.M // 2 + 1, 2), dtype=torch.float32, device=x.device)
        check(_core._lib.dsr_fb_analysis_block(self.fb.h, self.h, _dev(x), _dev(nd), U, Cn, N, int(last), T, _dev(X), cur_stream()))
        return torch.view_as_complex(X)

    def synthesis_block(self, Y, nframes=None):
        """Y: cuda complex64 [U][T][M/2+1] = the block's new subband frames -> float32 [U][nblocks * D]"""
        U, T, F = Y.shape
        nf = [T] * U if nframes is None else [int(v) for v in nframes]
        nd = torch.tensor(nf, dtype=torch.int32, device=Y.device)
        nb = max(1, max(_core._lib.dsr_fb_synthesis_block_blocks(self.fb.h, self.h, n) for n in nf))
        y = torch.zeros((U, nb * self.fb.D), dtype=torch.float32, device=Y.device)
        Yr = torch.view_as_real(Y.contiguous())
        check(_core._lib.dsr_fb_synthesis_block(self.fb.h, self.h, _dev(Yr), _dev(nd), max(nf), U, T, nb * self.fb.D, _dev(y), cur_stream()))
        return y


class PrFilterBank(Handle):
    """PerfectReconstructionFFTAnalysisBank / SynthesisBank (modulated.cc:686-970), prototype of length 2M*m."""

    _destroy = "dsr_prfb_destroy"

    def __init__(self, prototype, M, m, r=0):
        L = load(); self.M, self.m, self.r = M, m, r
        p = _np(prototype, np.float64)
        if p.size != 2 * M * m:
            raise DsrError(4, "Prototype sizes do not match (%d vs. %d)." % (p.size, 2 * M * m))
        self._create(L.dsr_prfb_create, _ptr(p), M, m, r)

    def analysis(self, x, nsamp=None):
        """x: cuda float32 [U][C][N] -> complex64 [U][C][T][2M]"""
        U, Cn, N = x.shape
        nsamp = _counts(nsamp, U, N, x.device)
        T = max(1, max(_core._lib.dsr_prfb_analysis_frames(self.h, int(n)) for n in nsamp.tolist()))
        X = torch.zeros((U, Cn, T, 2 * self.M), dtype=torch.complex64, device=x.device)
        check(_core._lib.dsr_prfb_analysis(self.h, _dev(x), _dev(nsamp), U, Cn, N, T, _dev(X), cur_stream()))
        return X

    def synthesis(self, Y, nframes=None):
        """Y: cuda complex64 [U][T][2M] -> float32 [U][(T-(2m-1))*D]"""
        U, T, M2 = Y.shape
        nframes = _counts(nframes, U, T, Y.device)
        nb = max(1, max(_core._lib.dsr_prfb_synthesis_blocks(self.h, int(n)) for n in nframes.tolist()))
        D = self.M >> self.r
        y = torch.zeros((U, nb * D), dtype=torch.float32, device=Y.device)
        check(_core._lib.dsr_prfb_synthesis(self.h, _dev(Y.contiguous()), _dev(nframes), U, T, nb * D, _dev(y), cur_stream()))
        return y


class NormalFFTBank(Handle):
    """NormalFFTAnalysisBank (modulated.cc:121-257): windowed STFT, windowType 0 rectangle / 1 Hamming / 2 Hanning."""

    _destroy = "dsr_stft_destroy"

    def __init__(self, M, r, windowType=1):
        L = load(); self.M = M
        self._create(L.dsr_stft_create, M, r, windowType)

    def frames(self, nsamp):
        return _core._lib.dsr_stft_frames(self.h, int(nsamp))

    def analysis(self, x, nsamp=None):
        """x: cuda float32 [U][C][N] -> complex64 [U][C][T][M]"""
        U, Cn, N = x.shape
        nsamp = _counts(nsamp, U, N, x.device)
        T = max(1, max(self.frames(int(n)) for n in nsamp.tolist()))
        X = torch.zeros((U, Cn, T, self.M), dtype=torch.complex64, device=x.device)
        check(_core._lib.dsr_stft_analysis(self.h, _dev(x), _dev(nsamp), U, Cn, N, T, _dev(X), cur_stream()))
        return X
