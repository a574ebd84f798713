"""btk/feature and btk/convolution: envelopes, block convolution, the scalar operators, the MFCC front end."""
import ctypes as C

import numpy as np

from . import _core
from ._core import (DsrError, Handle, MfccCfg, check, cur_stream, load, torch, E_DIMENSION, E_PARAMETER, _np, _ptr, _dev, _counts, _batch)


class LpcEnvelope(Handle):
    """WarpMVDR/BurgMVDR (kind 0) and WarpLPC/BurgLPC (kind 1) envelopes of windowed frames, lpc.h:134-195,291-331."""

    _destroy = "dsr_lpc_destroy"

    def __init__(self, dim, order=60, warp=0.0, method=0, kind=0, correlate=0):
        L = load(); self.dim = dim
        self._create(L.dsr_lpc_create, dim, order, correlate, warp, method, kind)

    def run(self, frames):
        """frames: cuda float32 [T][dim] -> float64 [T][dim/2+1]"""
        T, dim = frames.shape
        assert dim == self.dim
        out = torch.zeros((T, dim // 2 + 1), dtype=torch.float64, device=frames.device)
        check(_core._lib.dsr_lpc_run(self.h, _dev(frames), T, _dev(out), cur_stream()))
        return out


class WtMvdrEnvelope(Handle):
    """WarpedTwiceMVDRFeature envelopes of windowed frames, lpc.h:205-246, lpc.cc:212-468."""

    _destroy = "dsr_wtmvdr_destroy"

    def __init__(self, dim, order=60, correlate=0, warp=0.0, warp_factor_fixed=False, sensibility=0.1):
        L = load(); self.dim = dim
        self._create(L.dsr_wtmvdr_create, dim, order, correlate, warp, int(bool(warp_factor_fixed)), sensibility)

    def run(self, frames, warps=None, want_pa=False):
        """frames: cuda float32 [T][dim], warps: cuda float32 [T] (each frame's first-stage warp) or None -> float64 [T][dim/2+1];
        with want_pa also PA float32 [T][dim+1] and rewarp float32 [T]"""
        T, dim = frames.shape
        assert dim == self.dim and frames.dtype == torch.float32 and frames.is_contiguous()
        assert warps is None or (warps.dtype == torch.float32 and warps.numel() == T and warps.is_contiguous())
        out = torch.zeros((T, dim // 2 + 1), dtype=torch.float64, device=frames.device)
        pa = torch.zeros((T, dim + 1), dtype=torch.float32, device=frames.device) if want_pa else None
        rw = torch.zeros((T,), dtype=torch.float32, device=frames.device) if want_pa else None
        check(_core._lib.dsr_wtmvdr_run(self.h, _dev(frames), _dev(warps) if warps is not None else None, T, _dev(out),
                                  _dev(pa) if want_pa else None, _dev(rw) if want_pa else None, cur_stream()))
        return (out, pa, rw) if want_pa else out


def spectral_smoothing(to, frm):
    """SpectralSmoothing::next on a batch (lpc.cc:485-529): to, frm cuda float64 [T][size] -> float64 [T][size]"""
    load()
    if tuple(to.shape) != tuple(frm.shape):
        raise DsrError(E_DIMENSION, "Feature sizes (%d vs. %d) do not match." % (to.shape[-1], frm.shape[-1]))
    assert to.dtype == torch.float64 and frm.dtype == torch.float64 and to.is_contiguous() and frm.is_contiguous()
    T, size = to.shape
    out = torch.zeros_like(to)
    check(_core._lib.dsr_specsmooth_run(_dev(to), _dev(frm), T, size, _dev(out), cur_stream()))
    return out


class BlockConvolver(Handle):
    """OverlapAdd / OverlapSave of btk/convolution on batches (include/dsr.h section 2g): kind "add" or "save", blocks of L samples, C impulse
    responses [C][P] (one source gives C output channels).  OverlapAdd's fp32 buffer is a device tensor of the caller (state) that apply()
    continues from and leaves behind."""
    KINDS = {"add": 0, "save": 1}

    _destroy = "dsr_conv_destroy"

    def __init__(self, kind, L, response, fftLen=0):
        L_ = load()
        if response is None:
            raise DsrError(E_PARAMETER, "null impulse response")
        h = np.ascontiguousarray(np.atleast_2d(np.asarray(response, dtype=np.float64)))
        self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind); self.L = int(L); self.C, self.P = h.shape
        self._create(L_.dsr_conv_create, self.kind, self.L, self.P, int(fftLen), self.C)
        check(L_.dsr_conv_set_response(self.h, _ptr(h)))
        self.size = int(L_.dsr_conv_size(self.h)); self.fftLen = int(L_.dsr_conv_fft_len(self.h))

    def update(self, delta, c=0):
        """OverlapSave::update: delta complex [L], its bins 0..L/2 are added to response c's spectrum"""
        d = np.ascontiguousarray(np.asarray(delta, dtype=np.complex128).reshape(-1))
        if d.size != self.L:
            raise DsrError(E_DIMENSION, "Dimension of udpate vector (%d) does not match frequency response (%d)." % (d.size, self.L))
        check(_core._lib.dsr_conv_update(self.h, int(c), _ptr(d)))

    def state(self, U, device="cuda:0"):
        st = torch.zeros(max(1, int(_core._lib.dsr_conv_state_bytes(self.h, int(U))) // 4), dtype=torch.float32, device=device)
        check(_core._lib.dsr_conv_state_init(self.h, _dev(st), int(U), cur_stream()))
        return st

    def apply(self, x, state=None, nframes=None):
        """x: cuda float32 [U][Tmax][L], nframes: cuda int32 [U] or None, state: from state(U) (OverlapAdd; None starts from zeros and drops
        what is left) -> float32 [U][C][Tmax][size]"""
        U, T, L = x.shape
        assert L == self.L and x.dtype == torch.float32 and x.is_contiguous()
        assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
        if self.kind == 0 and state is None:
            state = self.state(U, x.device)
        y = torch.zeros((U, self.C, T, self.size), dtype=torch.float32, device=x.device)
        check(_core._lib.dsr_conv_apply(self.h, _dev(x), _dev(nframes) if nframes is not None else None, U, T, _dev(state) if state is not None else None,
                                  _dev(y), cur_stream()))
        return y

    def set_timing(self, on=True):
        check(_core._lib.dsr_conv_set_timing(self.h, int(bool(on))))

    def kernel_ms(self):
        """ms of the last apply() in the transform kernel and in the fold"""
        two = (C.c_double * 2)(); check(_core._lib.dsr_conv_kernel_ms(self.h, two))
        return tuple(two)


def fir_frames(x, coeffA, nframes=None):
    """FilterFeature over whole utterances (feature.cc:3206-3313): x cuda float32 [U][Tmax][dim], coeffA odd-length taps, nframes cuda int32 [U] or
    None -> float32 [U][Tmax + (lenA == 1)][dim]; utterance u has fir_frames_count(nframes[u], lenA) frames, the rest are zero"""
    load()
    a = np.ascontiguousarray(np.asarray(coeffA, dtype=np.float64).reshape(-1))
    U, T, dim = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    y = torch.zeros((U, T + (1 if a.size == 1 else 0), dim), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_fir_frames_run(_dev(x), _dev(nframes) if nframes is not None else None, _ptr(a), int(a.size), U, T, dim, _dev(y), cur_stream()))
    return y


def fir_frames_count(T, lenA):
    return int(load().dsr_fir_frames_count(int(T), int(lenA)))


# ---- the scalar feature operators of btk/feature (include/dsr.h section 6c, csrc/k_featops.hip)
def signal_power(x, nframes=None):
    """SignalPowerFeature over whole utterances: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1]"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_signal_power_run(_dev(x), nf, U, T, dim, _dev(y), cur_stream()))
    return y


def zero_crossing_rate(x, nframes=None):
    """ZeroCrossingRateHammingFeature: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1]"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_zcr_hamming_run(_dev(x), nf, U, T, dim, _dev(y), cur_stream()))
    return y


def yin_pitch(x, samplerate=16000, threshold=0.5, nframes=None, return_value=False, return_chunks=False):
    """YINPitchFeature: x cuda float32 [U][Tmax][dim] -> pitch float32 [U][Tmax][1]; return_value adds float32 [U][Tmax], y(tau) at the lag where
    the reference's search returned (y(W-1) where it ran to the end); return_chunks adds int32 [U][Tmax], the chunks of 64 lags evaluated"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    p = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    v = torch.zeros((U, T), dtype=torch.float32, device=x.device) if return_value else None
    c = torch.zeros((U, T), dtype=torch.int32, device=x.device) if return_chunks else None
    check(_core._lib.dsr_yin_pitch_run(_dev(x), nf, U, T, dim, int(samplerate), float(threshold), _dev(p), _dev(v) if return_value else None,
                                 _dev(c) if return_chunks else None, cur_stream()))
    out = (p,) + ((v,) if return_value else ()) + ((c,) if return_chunks else ())
    return out if len(out) > 1 else p


def yin_kernel(dim):
    """frames a workgroup of the YIN kernel a frame length selects (the frame's copies in LDS), 0: the kernel that reads global memory"""
    return int(load().dsr_yin_kernel(int(dim)))


def spike_filter(x, tapN=3, nframes=None):
    """SpikeFilter: the running median of tapN samples within each block; the last tapN-1 samples of a block stay zero as in the reference"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_spike_filter_run(_dev(x), nf, U, T, dim, int(tapN), _dev(y), cur_stream()))
    return y


def spike_filter2_state(U, startslope=100.0, device="cuda:0"):
    """(meanslope float32 [U], count int32 [U]) as SpikeFilter2::reset() leaves them"""
    return torch.full((U,), float(startslope), dtype=torch.float32, device=device), torch.zeros((U,), dtype=torch.int32, device=device)


def spike_filter2(x, width=3, maxslope=7000.0, startslope=100.0, thresh=15.0, alpha=0.2, state=None, nframes=None):
    """SpikeFilter2 over the blocks of each utterance in order: x cuda float32 [U][Tmax][dim] -> (y, (meanslope, count)); state: the pair a
    previous call returned (None: reset())"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    if state is None:
        state = spike_filter2_state(U, startslope, x.device)
    ms, cnt = state
    assert ms.dtype == torch.float32 and cnt.dtype == torch.int32 and ms.numel() == U and cnt.numel() == U
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_spike_filter2_run(_dev(x), nf, U, T, dim, int(width), float(maxslope), float(thresh), float(alpha), _dev(ms), _dev(cnt), _dev(y), cur_stream()))
    return y, (ms, cnt)


def minmax_state(U, device="cuda:0"):
    """(min, max) of ALog / Normalize after nextSpeaker(): float64 [U][2] = (HUGE, -HUGE)"""
    load(); st = torch.zeros((U, 2), dtype=torch.float64, device=device)
    check(_core._lib.dsr_minmax_state_init(_dev(st), U, cur_stream()))
    return st


def alog(x, m=1.0, a=4.0, runon=False, state=None, nframes=None):
    """ALogFeature: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1].  runon: the running (min, max) continue from state (minmax_state) and
    are left there; otherwise they are taken over the whole utterance"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_alog_run(_dev(x), nf, U, T, dim, float(m), float(a), int(bool(runon)), _dev(state) if state is not None else None, _dev(y), cur_stream()))
    return y


def normalize(x, min=0.0, max=1.0, runon=False, state=None, nframes=None):
    """NormalizeFeature: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][dim]; runon and state as in alog"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_normalize_run(_dev(x), nf, U, T, dim, float(min), float(max), int(bool(runon)), _dev(state) if state is not None else None, _dev(y),
                                 cur_stream()))
    return y


def threshold(x, value=0.0, thresh=1.0, mode="upper", nframes=None):
    """ThresholdFeature: mode "upper", "lower" or "both" (any other: a key error)"""
    load(); cmp_ = C.c_int(0)
    check(_core._lib.dsr_threshold_mode(mode.encode() if isinstance(mode, str) else mode, C.byref(cmp_)))
    (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_threshold_run(_dev(x), nf, U, T, dim, float(value), float(thresh), cmp_.value, _dev(y), cur_stream()))
    return y


def amplify(x, amplify=1.0, nframes=None):
    """AmplificationFeature: float(double(x) * amplify)"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_amplify_run(_dev(x), nf, U, T, dim, float(amplify), _dev(y), cur_stream()))
    return y


SPECTRAL_SAMPLE_RATIO = 16.0 / 22.05


def spectral_resample(x, ratio=SPECTRAL_SAMPLE_RATIO, len=0, nframes=None):
    """SpectralResamplingFeature: x cuda float64 [U][Tmax][srcN] -> float64 [U][Tmax][len or srcN]"""
    load(); (U, T, srcN), nf = _batch(x, nframes, torch.float64)
    outN = C.c_int(0)
    check(_core._lib.dsr_spectral_resample_size(srcN, float(ratio), int(len), C.byref(outN)))
    y = torch.zeros((U, T, outN.value), dtype=torch.float64, device=x.device)
    check(_core._lib.dsr_spectral_resample_run(_dev(x), nf, U, T, srcN, float(ratio), int(len), _dev(y), cur_stream()))
    return y


class SphinxMel(Handle):
    """SphinxMelFeature's filter bank: .filters is the host-built [filterN][powerN] fp64 matrix, apply() multiplies frames by it"""

    _destroy = "dsr_sphinx_mel_destroy"

    def __init__(self, fftN=512, powerN=257, sampleRate=16000.0, lowerF=0.0, upperF=0.0, filterN=30):
        L_ = load()
        self._create(L_.dsr_sphinx_mel_create, int(fftN), int(powerN), float(sampleRate), float(lowerF), float(upperF), int(filterN))
        self.powerN, self.filterN = int(powerN), int(filterN)
        self.filters = np.zeros((self.filterN, self.powerN), np.float64)
        check(L_.dsr_sphinx_mel_filters(self.h, _ptr(self.filters)))

    def apply(self, x, nframes=None):
        """x cuda float64 [U][Tmax][powerN] -> float64 [U][Tmax][filterN]"""
        (U, T, dim), nf = _batch(x, nframes, torch.float64)
        assert dim == self.powerN
        y = torch.zeros((U, T, self.filterN), dtype=torch.float64, device=x.device)
        check(_core._lib.dsr_sphinx_mel_apply(self.h, _dev(x), nf, U, T, _dev(y), cur_stream()))
        return y


MFCC_FRAMES_PLAIN, MFCC_FRAMES_W = 0, 1
MFCC_CMN_NONE, MFCC_CMN_PLAIN, MFCC_CMN_LDS = 0, 1, 2
MFCC_LDA_TOO_LARGE, MFCC_LDA_SPLICE, MFCC_LDA_PLAIN, MFCC_LDA_B = -1, 0, 1, 2


def mfcc_cfg_paths(Tmax, **kw):
    """-> ((frames, cmn, lda), dict of the LDS bytes the gates compare) for the configuration Mfcc(**kw) would have; needs no device"""
    L = load()
    cfg = MfccCfg(); L.dsr_mfcc_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    out = (C.c_int * 3)(); lds = (C.c_int64 * 4)()
    check(L.dsr_mfcc_cfg_paths(C.byref(cfg), int(Tmax), out, lds))
    return tuple(out), dict(zip(("ldsW", "ldsC", "ldsB", "lds2"), lds))


class Mfcc(Handle):
    _destroy = "dsr_mfcc_destroy"

    def __init__(self, lda=None, **kw):
        L = load()
        self.cfg = MfccCfg(); L.dsr_mfcc_default_cfg(C.byref(self.cfg))
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        if lda is None and "outDim" not in kw:
            self.cfg.outDim = 0
        a = _np(lda, np.float32) if lda is not None else None
        self._create(L.dsr_mfcc_create, C.byref(self.cfg), _ptr(a) if a is not None else None)
        self.outDim = L.dsr_mfcc_out_dim(self.h)

    def frames(self, nsamp):
        return _core._lib.dsr_mfcc_frames(self.h, int(nsamp))

    def paths(self, Tmax):
        """(frames, cmn, lda) kernels dsr_mfcc_run launches for a batch of Tmax frames: MFCC_FRAMES_*, MFCC_CMN_*, MFCC_LDA_*"""
        out = (C.c_int * 3)()
        check(_core._lib.dsr_mfcc_paths(self.h, int(Tmax), out))
        return tuple(out)

    def run(self, y, nsamp=None, stage=0):
        """y: cuda float32 [U][N] -> float32 [U][Tmax][dim]"""
        U, N = y.shape
        nsamp = _counts(nsamp, U, N, y.device)
        c = self.cfg
        raw = lambda n: ((n + c.shiftLen - 1) // c.shiftLen) if c.padZeros else max(0, -(-(n - c.blockLen) // c.shiftLen))
        Tmax = max(1, max(raw(int(n)) for n in nsamp.tolist()))
        dim = {0: self.outDim, 1: c.ncep, 2: c.ncep, 3: c.filterN, 4: c.powN}[stage]
        out = torch.zeros((U, Tmax, dim), dtype=torch.float32, device=y.device)
        check(_core._lib.dsr_mfcc_run(self.h, _dev(y), _dev(nsamp), U, N, Tmax, stage, _dev(out), cur_stream()))
        return out
