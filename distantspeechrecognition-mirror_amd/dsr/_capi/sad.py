"""btk/sad: speech activity detection (include/dsr.h section 7b, csrc/k_sad.hip)."""
import ctypes as C
import os

import numpy as np

from . import _core
from ._core import (Handle, check, cur_stream, load, torch, f64, _np, _ptr, _dev, _batch)


def _sad_out(U, T, device):
    return torch.zeros((U, T), dtype=torch.float64, device=device), torch.zeros((U, T), dtype=torch.float64, device=device)


def sad_energy_state(U, energiesN=200, initialEnergy=5.0e+07, device="cuda:0"):
    """EnergyVADMetric after nextSpeaker(): (history float64 [U][energiesN] -- a ring --, counters int32 [U][4] = (aboveThresholdN,
    belowThresholdN, recognizing, ring position))"""
    load(); hist = torch.zeros((U, energiesN), dtype=torch.float64, device=device); cnt = torch.zeros((U, 4), dtype=torch.int32, device=device)
    check(_core._lib.dsr_sad_energy_state_init(_dev(hist), _dev(cnt), U, int(energiesN), float(initialEnergy), 0, cur_stream()))
    return hist, cnt


def sad_energy_reset(state):
    """EnergyVADMetric::reset(): the counters are cleared, the history and its ring position stay"""
    hist, cnt = state
    check(load().dsr_sad_energy_state_init(_dev(hist), _dev(cnt), hist.shape[0], hist.shape[1], 0.0, 1, cur_stream()))
    return state


def sad_energy(x, threshold=0.5, headN=4, tailN=10, state=None, initialEnergy=5.0e+07, energiesN=200, nframes=None, return_updates=False):
    """EnergyVADMetric over the blocks of each utterance in order: x cuda float32 [U][Tmax][dim] -> (decision float64 [U][Tmax], score (the
    blocks' energies) float64 [U][Tmax], state).  state: the pair a previous call returned (None: nextSpeaker()); it is updated in place."""
    load(); (U, T, dim), nf = _batch(x, nframes)
    if state is None:
        state = sad_energy_state(U, energiesN, initialEnergy, x.device)
    hist, cnt = state
    assert hist.dtype == torch.float64 and cnt.dtype == torch.int32 and hist.dim() == 2 and hist.shape[0] == U and cnt.numel() == 4 * U
    dec, score = _sad_out(U, T, x.device)
    upd = torch.zeros((U,), dtype=torch.int32, device=x.device) if return_updates else None
    check(_core._lib.dsr_sad_energy_run(_dev(x), nf, U, T, dim, float(threshold), int(headN), int(tailN), int(hist.shape[1]), _dev(hist), _dev(cnt), _dev(dec), _dev(score),
                                  _dev(upd) if return_updates else None, cur_stream()))
    return (dec, score, state) + ((upd,) if return_updates else ())


def sad_energy_percentile(state, percentile=50.0, u=0):
    """EnergyVADMetric::energyPercentile of utterance u's history"""
    h = np.ascontiguousarray(state[0][u].cpu().numpy()); v = f64(0.0)
    check(load().dsr_sad_energy_percentile(_ptr(h), int(h.size), float(percentile), C.byref(v)))
    return v.value


def sad_simple_energy(X, threshold, gamma=0.98, state=None, nframes=None):
    """SimpleEnergyVAD: X cuda complex128 [U][Tmax][fftLen] -> (decision float64 [U][Tmax] (1.0 speech, 0.0 not), score = e / E, state);
    state: E float64 [U] (None: zeros, nextSpeaker()), updated in place"""
    load(); (U, T, N), nf = _batch(X, nframes, torch.complex128)
    if state is None:
        state = torch.zeros((U,), dtype=torch.float64, device=X.device)
    assert state.dtype == torch.float64 and state.numel() == U
    dec, score = _sad_out(U, T, X.device)
    check(_core._lib.dsr_sad_simple_energy_run(_dev(X), nf, U, T, N, float(threshold), float(gamma), _dev(state), _dev(dec), _dev(score), cur_stream()))
    return dec, score, state


def sad_band(fftLen, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0):
    """(lowX, highX, binN) of MultiChannelVADMetric; a cutoff at or above sampleRate / 2 is a dimension error as there"""
    lo, hi, bn = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    check(load().dsr_sad_band(int(fftLen), float(sampleRate), float(lowCutoff), float(highCutoff), C.byref(lo), C.byref(hi), C.byref(bn)))
    return lo.value, hi.value, bn.value


SAD_POWER_RATIO, SAD_ENERGY_RATIO, SAD_TSPS = 0, 1, 2


def sad_power(P, fftLen, kind=SAD_POWER_RATIO, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, E0=None, nframes=None):
    """PowerSpectrumVADMetric (kind 0), NormalizedEnergyMetric (1), TSPSVADMetric (2): P cuda float32 [U][C][Tmax][fftLen/2+1], channel 0 the
    target -> (decision float64 [U][Tmax] +-1, powers float64 [U][Tmax][C], score float64 [U][Tmax])"""
    load()
    assert P.dim() == 4 and P.dtype == torch.float32 and P.is_contiguous() and P.shape[3] == fftLen // 2 + 1
    U, Cn, T, F = P.shape
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    lo, hi, _ = sad_band(fftLen, sampleRate, lowCutoff, highCutoff)
    if E0 is None:
        E0 = 5000.0 if kind == SAD_TSPS else 1.0
    dec, score = _sad_out(U, T, P.device)
    pw = torch.zeros((U, T, Cn), dtype=torch.float64, device=P.device)
    check(_core._lib.dsr_sad_power_run(_dev(P), _dev(nframes) if nframes is not None else None, U, Cn, T, int(fftLen), lo, hi, int(kind), float(E0), _dev(dec), _dev(pw),
                                 _dev(score), cur_stream()))
    return dec, pw, score


def sad_ccc(X, nCand, threshold=0.1, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, band=None, nframes=None, return_candidates=False):
    """CCCVADMetric: X cuda complex64 or complex128 [U][C][Tmax][fftLen], channel 0 the reference -> (decision float64 [U][Tmax] (1.0 where
    score < threshold, else -1.0), score float64 [U][Tmax]).  band = (lowX, highX) overrides the cutoffs."""
    load()
    assert X.dim() == 4 and X.dtype in (torch.complex64, torch.complex128) and X.is_contiguous()
    U, Cn, T, N = X.shape
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    lo, hi = band if band is not None else sad_band(N, sampleRate, lowCutoff, highCutoff)[:2]
    dec, score = _sad_out(U, T, X.device)
    cands = torch.zeros((U, T, int(nCand)), dtype=torch.float64, device=X.device) if return_candidates else None
    check(_core._lib.dsr_sad_ccc_run(_dev(X), 1 if X.dtype == torch.complex128 else 0, _dev(nframes) if nframes is not None else None, U, Cn, T, N, int(lo), int(hi),
                               int(nCand), float(threshold), _dev(dec), _dev(score), _dev(cands) if return_candidates else None, cur_stream()))
    return (dec, score) + ((cands,) if return_candidates else ())


SAD_HANGOVER, SAD_HANGOVER_MI, SAD_HANGOVER_MULTISTAGE = 0, 1, 2


def sad_hangover(decisions, thresholds=(0.5,), headN=4, tailN=10, kind=SAD_HANGOVER, nframes=None):
    """The hangover segmenters' rule over K metrics' decisions: cuda float64 [K][U][Tmax] -> (start, length, consumed int32 [U],
    decisionMetric int32 [U][Tmax])"""
    load()
    assert decisions.dim() == 3 and decisions.dtype == torch.float64 and decisions.is_contiguous()
    K, U, T = decisions.shape
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    thr = _np(list(thresholds) + [0.5] * (K - len(thresholds)), np.float64)
    out = [torch.zeros((U,), dtype=torch.int32, device=decisions.device) for _ in range(3)]
    dm = torch.zeros((U, T), dtype=torch.int32, device=decisions.device)
    check(_core._lib.dsr_sad_hangover_run(_dev(decisions), _dev(nframes) if nframes is not None else None, K, U, T, _ptr(thr), int(headN), int(tailN), int(kind),
                                    _dev(out[0]), _dev(out[1]), _dev(out[2]), _dev(dm), cur_stream()))
    return out[0], out[1], out[2], dm


def sad_gather(x, start, length):
    """the segment's frames packed: x cuda float32 [U][Tmax][dim] -> [U][Tmax][dim], rows start[u] .. start[u] + length[u] - 1 first, zeros after"""
    load(); (U, T, dim), _ = _batch(x, None)
    assert start.dtype == torch.int32 and length.dtype == torch.int32 and start.numel() == U and length.numel() == U
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_sad_gather_run(_dev(x), _dev(start), _dev(length), U, T, dim, _dev(y), cur_stream()))
    return y


SAD_ENERGY_DIFFUSION, SAD_BAND_ENERGY_RATIO, SAD_NEGATIVE_ENTROPY, SAD_SIGNIFICANT_SUBBANDS = 0, 1, 2, 3


def sad_shape(x, op, sampleRate=16000.0, thresh=0.0, nframes=None):
    """The spectral-shape operators of btk/sad/sadFeature.cc: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1].  op: SAD_ENERGY_DIFFUSION,
    SAD_BAND_ENERGY_RATIO (thresh = threshF in Hz, 0: sampleRate / 4), SAD_NEGATIVE_ENTROPY, SAD_SIGNIFICANT_SUBBANDS (thresh on the normalised frame)"""
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_core._lib.dsr_sad_shape_run(_dev(x), nf, U, T, dim, int(op), float(sampleRate), float(thresh), _dev(y), cur_stream()))
    return y


SAD_NEGENTROPY, SAD_MUTUAL_INFORMATION, SAD_LIKELIHOOD_RATIO = 0, 1, 2


def sad_read_shape_factors(directory, fftLen):
    """the per-bin shape factors of the reference's directory of _M-%04d files: float64 [fftLen/2+1]"""
    sf = np.zeros(fftLen // 2 + 1, np.float64)
    check(load().dsr_sad_gg_read_shape_factors(str(directory).encode(), int(fftLen), _ptr(sf)))
    return sf


class SadGG(Handle):
    """The host-side model of NegentropyVADMetric / MutualInformationVADMetric / LikelihoodRatioVADMetric: shapeFactors float64 [fftLen/2+1], a
    directory of _M-%04d files, or None (all 2.0, the Gaussian).  joint: also the matched joint pdfs and the fixed threshold of the mutual
    information (DsrError JNUMERIC where the bisection does not converge in 200 steps)."""

    _destroy = "dsr_sad_gg_destroy"

    def __init__(self, fftLen, shapeFactors=None, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, joint=True):
        load(); self.fftLen = int(fftLen); self.F = self.fftLen // 2 + 1
        if isinstance(shapeFactors, (str, bytes, os.PathLike)):
            shapeFactors = None if str(shapeFactors) == "" else sad_read_shape_factors(shapeFactors, fftLen)
        sf = None if shapeFactors is None else _np(shapeFactors, np.float64)
        assert sf is None or sf.size == self.F
        self._create(_core._lib.dsr_sad_gg_create, _ptr(sf) if sf is not None else None, self.fftLen, float(sampleRate), float(lowCutoff), float(highCutoff),
                     1 if joint else 0)
        self.table = np.zeros((self.F, 6), np.float64); ft = f64(0.0)
        check(_core._lib.dsr_sad_gg_table(self.h, _ptr(self.table), C.byref(ft))); self.fixedThreshold = ft.value

    def rho_state(self, U, device="cuda:0"):
        """rho after nextSpeaker(): complex128 zeros [U][fftLen/2+1]"""
        return torch.zeros((U, self.F), dtype=torch.complex128, device=device)

    def run(self, kind, X1, env1, X2=None, env2=None, twiddle=-1.0, threshold=None, beta=0.95, rho=None, nframes=None, return_threshold=False):
        """X cuda complex128 [U][Tmax][fftLen], env cuda float32 [U][Tmax][>= fftLen/2+1] -> (decision, score) float64 [U][Tmax]; the mutual
        information also returns rho (updated in place; None: zeros) and, with return_threshold, the threshold of every frame"""
        (U, T, N), nf = _batch(X1, nframes, torch.complex128)
        assert N == self.fftLen and env1.dim() == 3 and env1.dtype == torch.float32 and env1.is_contiguous() and env1.shape[:2] == (U, T)
        if kind != SAD_NEGENTROPY:
            assert X2.shape == X1.shape and X2.dtype == torch.complex128 and X2.is_contiguous() and env2.shape == env1.shape and env2.dtype == torch.float32 and env2.is_contiguous()
        if threshold is None:
            threshold = (0.5, 1.3, 0.0)[kind]
        if kind == SAD_MUTUAL_INFORMATION and rho is None:
            rho = self.rho_state(U, X1.device)
        assert rho is None or (rho.dtype == torch.complex128 and rho.shape == (U, self.F) and rho.is_contiguous())
        dec, score = _sad_out(U, T, X1.device)
        thr = torch.zeros((U, T), dtype=torch.float64, device=X1.device) if return_threshold else None
        check(_core._lib.dsr_sad_gg_run(self.h, int(kind), _dev(X1), _dev(X2) if X2 is not None else None, _dev(env1), _dev(env2) if env2 is not None else None, env1.shape[2], nf,
                                  U, T, float(twiddle), float(threshold), float(beta), _dev(rho) if rho is not None else None, _dev(dec), _dev(score),
                                  _dev(thr) if return_threshold else None, cur_stream()))
        out = (dec, score) + ((rho,) if kind == SAD_MUTUAL_INFORMATION else ()) + ((thr,) if return_threshold else ())
        return out
