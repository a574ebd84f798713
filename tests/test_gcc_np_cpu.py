"""CPU tests of the pairwise time-delay estimators: tests/gcc_np.py against independent forms (numpy's irfft, a brute-force time-domain
correlation of whitened signals, closed-form recurrences, planted delays), the conditions the GPU comparison relies on, and the host side
of the C-ABI (exports, dsr_gcc_channel_delays, create-time refusals)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gcc_cases as K
from tests import gcc_np as G
from tests.conftest import ROOT, PKG

LIB = os.path.join(PKG, "lib", "libdsr_hip.so")


def test_correlation_is_the_scaled_inverse_real_fft():
    r = np.random.default_rng(0)
    for n in (8, 64, 256, 2048, 4096):
        s = r.standard_normal(n // 2 + 1) + 1j * r.standard_normal(n // 2 + 1)
        assert np.abs(G.correlation(s, n) - np.fft.irfft(s, n)).max() < 1e-14
        h = G.half_complex_pack(s, n)
        assert h[0] == s[0].real and h[n // 2] == s[n // 2].real and h[1] == s[1].real and h[n - 1] == s[1].imag


def _brute_circular(w1, w2):
    n = len(w1)
    return np.array([sum(w1[(m + k) % n] * w2[m] for m in range(n)) for k in range(n)])


def test_phat_is_the_correlation_of_the_whitened_signals():
    r = np.random.default_rng(1); n = 64
    x1, x2 = r.standard_normal(n), r.standard_normal(n)
    X1, X2 = np.fft.fft(x1), np.fft.fft(x2)
    w1, w2 = np.fft.ifft(X1 / np.abs(X1)).real, np.fft.ifft(X2 / np.abs(X2)).real
    g = G.GCC("phat", K.SR, n, 2, 1)
    g.calculate(X1, 0, X2, 1, 0, 0.01, sad=True, smooth=False)
    assert np.abs(g.corr[0] - _brute_circular(w1, w2)).max() < 1e-12
    zero = np.zeros(n, np.complex128)
    assert np.array_equal(G.cross_value(G.PHAT, zero, X2, None, None, None, 0.3), zero)          # a zero product gives 0, not NaN


def test_noise_trackers_follow_their_closed_forms():
    r = np.random.default_rng(2); n, T, a = 16, 7, 0.9
    S1 = r.standard_normal((T, n)) + 1j * r.standard_normal((T, n)); S2 = r.standard_normal((T, n)) + 1j * r.standard_normal((T, n))
    g = G.GCC("raw", K.SR, n, 2, 1, alpha=a)
    for t in range(T):
        g.calculate(S1[t], 0, S2[t], 1, 0, 0.01 * (t + 1), sad=False)
    w = (1 - a) * a ** (T - 1 - np.arange(T))                                                       # the first frame stores (1 - alpha) v^2 too
    ln = n // 2 + 1
    assert np.allclose(g.np_[0].p, (w[:, None] * np.abs(S1[:, :ln]) ** 2).sum(0), rtol=1e-13)
    assert np.allclose(g.nc[0].g, (w[:, None] * (S1[:, :ln] * np.conj(S2[:, :ln]))).sum(0), rtol=1e-13)
    # a first noise frame stamped 0.0 updates the cross-spectrum but not the powers; a repeated stamp is skipped too
    g = G.GCC("raw", K.SR, n, 2, 1, alpha=a)
    g.calculate(S1[0], 0, S2[0], 1, 0, 0.0, sad=False)
    assert g.np_[0].p is None and g.nc[0].g is not None
    g.calculate(S1[1], 0, S2[1], 1, 0, 0.5, sad=False); p = g.np_[0].p.copy()
    g.calculate(S1[2], 0, S2[2], 1, 0, 0.5, sad=False)
    assert np.array_equal(g.np_[0].p, p)
    # sad == True computes and learns nothing; a non-speech frame leaves cross-spectrum and correlation alone
    g.calculate(S1[3], 0, S2[3], 1, 0, 0.6, sad=True); c = g.corr[0].copy(); x = g.cross[0].copy(); gn = g.nc[0].g.copy()
    assert np.array_equal(g.nc[0].g, gn)
    g.calculate(S1[4], 0, S2[4], 1, 0, 0.7, sad=False)
    assert np.array_equal(g.corr[0], c) and np.array_equal(g.cross[0], x)


def test_fallbacks_without_a_noise_estimate():
    r = np.random.default_rng(3); n = 16
    x1 = r.standard_normal(n) + 1j * r.standard_normal(n); x2 = r.standard_normal(n) + 1j * r.standard_normal(n)
    G0 = x1 * np.conj(x2)
    assert np.allclose(G.cross_value(G.GNNSUBPHAT, x1, x2, None, None, None, 0.3), G0 / np.abs(G0))
    w = np.abs(x1) * np.abs(x2) / (0.6 * np.abs(x1) ** 2 * np.abs(x2) ** 2)
    assert np.allclose(G.cross_value(G.MLRRAW, x1, x2, None, None, None, 0.3), G0 * w)
    assert np.allclose(G.cross_value(G.MLRGNNSUB, x1, x2, None, np.ones(n), np.ones(n), 0.3), G0 * w)
    with pytest.raises(RuntimeError):
        G.cross_value(G.GNNSUB, x1, x2, None, None, None, 0.3)


def test_find_maximum_rules():
    sr = 8.0; c = np.zeros(8); c[2] = 1.0; c[6] = 1.0; c[1] = 0.5
    r = G.find_maximum(c, sr, interpolate=False)
    assert r["delay"] == 2 / sr and r["maxCorr"] == 1.0 and r["maxCorr2"] == 1.0 and r["ratio"] == 1.0      # strict >: the first of equals; the later equal is second
    r = G.find_maximum(c, sr, minDelay=-3 / sr, maxDelay=1 / sr, interpolate=False)
    assert r["delay"] == -2 / sr and r["maxCorr2"] == 0.5                                                   # index 6 is lag -2
    r = G.find_maximum(c, sr, minDelay=5.0, maxDelay=6.0, interpolate=False)
    assert r["maxCorr"] == -G.HUGE and r["ratio"] == 1.0 and r["delay"] == 0.0 and r["pos"] == 0
    # the two edge cases of the interpolation use the neighbouring triple
    e = np.zeros(8); e[4] = 3.0; e[5] = 2.0; e[6] = 0.5                                                     # lag -4 is position 0 of the delay-ordered table
    lo = G.find_maximum(e, sr); xv = (np.arange(8) - 4) / sr; yv = np.roll(e, 4)
    assert lo["pos"] == 0 and lo["delay"] == G.interpolation(xv, yv, 1)[0]
    # a parabola's vertex comes back exactly
    y = -(np.arange(8) - 4 - 1.25) ** 2
    r = G.find_maximum(np.roll(y, -4), sr)
    assert abs(r["delay"] * sr - 1.25) < 1e-12


@pytest.mark.parametrize("kind", ["raw", "phat"])
@pytest.mark.parametrize("n", [64, 256])
def test_planted_integer_delay_comes_back(kind, n):
    for seed in range(4):
        for d in (1, n // 16, n // 8):
            r = np.random.default_rng(100 + seed)
            s = r.standard_normal(2 * n); w = G.hann(n)
            x1 = w * s[n // 2:n // 2 + n]; x2 = w * s[n // 2 - d:n // 2 - d + n]                            # x2(t) = x1(t - d)
            for interp in (False, True):
                g = G.GCC(kind, K.SR, n, 2, 1, interpolate=interp)
                g.calculate(np.fft.fft(x1), 0, np.fft.fft(x2), 1, 0, 0.01, sad=True, smooth=False)
                got = g.findMaximum()["delay"]
                if interp:
                    assert abs(got * K.SR + d) <= 0.5, (seed, d, got * K.SR)
                else:
                    assert got == -(d / K.SR), (seed, d, got * K.SR)                                        # pair delay = tau_1 - tau_2 = -d samples


def test_end_to_end_signal_gives_exact_sample_delays():
    """the 8-channel signal of the GPU end-to-end test: every star pair's uninterpolated PHAT delay is the planted integer"""
    X = K.spectra(77, 1, 8, 6, 256, noise=0.02)
    pairs = K.star(8)
    out = G.run_batch("phat", X, [6], np.ones((1, 6), np.int32), 0.01 * (1 + np.arange(6))[None], pairs, K.SR, 256, interpolate=False)
    true = np.array([(3 * c) % 7 - 3 for c in range(8)], float)
    for t in range(6):
        assert np.array_equal(out["result"][0, t, :, 0] * K.SR, true[0] - true[1:]), t
    assert np.array_equal(G.channel_delays(pairs, out["result"][0, 5, :, 0], 8), (true - true[0]) / K.SR)


@pytest.mark.parametrize("i", range(len(K.CASES)))
def test_gpu_cases_leave_out_at_most_two_percent(i):
    """the cap of the GPU comparison is a condition on the inputs: checked here on the restatement, with and without a 1e-12 perturbation"""
    case = K.CASES[i]; b = K.build(case); ref = K.reference(case, b)
    r = np.random.default_rng(i)
    items = left = leftP = 0
    U, T, P = ref["valid"].shape
    for u in range(U):
        for t in range(int(b["nframes"][u])):
            for p in range(P):
                if not ref["valid"][u, t, p]:
                    continue
                items += 1
                idx, _, interp = K.comparable(ref["info"][u, t, p], ref["corr"][u, t, p])
                left += (not idx) or (case["interp"] and not interp)
                c2 = ref["corr"][u, t, p] * (1 + 1e-12 * r.standard_normal(case["N"]))
                i2 = G.find_maximum(c2, K.SR, b["minDelay"], b["maxDelay"], case["interp"])
                idx2, _, interp2 = K.comparable(i2, c2)
                leftP += (not idx2) or (case["interp"] and not interp2)
                if idx and idx2:
                    assert i2["pos"] == ref["info"][u, t, p]["pos"]
    assert items > 0 and left <= 0.02 * items and leftP <= 0.02 * items, (items, left, leftP)


def _brute_phase_cc(b1, b2, n):
    w = G.hann(n)
    x = [np.concatenate([w[:len(b)] * b, np.zeros(n - len(b))]) for b in (b1, b2)]
    A, B = np.fft.fft(x[0]), np.fft.fft(x[1])
    wa, wb = np.fft.ifft(A / np.abs(A)).real, np.fft.ifft(B / np.abs(B)).real
    return np.array([sum(wb[(m + k) % n] * wa[m] for m in range(n)) for k in range(n)])                   # conj(A) B: b against a


def test_cctde_matches_brute_force_and_orders_its_peaks():
    r = np.random.default_rng(5); n = 64
    s = r.standard_normal(3 * n).astype(np.float32)
    a = s[n:2 * n]; b = s[n - 5:2 * n - 5]                                                                  # b(t) = a(t - 5)
    cc = G.cctde_cc(a, b, n)
    assert np.abs(cc - _brute_phase_cc(a.astype(float), b.astype(float), n)).max() < 1e-12
    d, lag, v = G.cctde_peaks(cc, 3, 16000)
    assert lag[0] == 5 and d[0] == np.float32(5 / 16000) and np.all(np.diff(v) <= 0)
    order = np.argsort(-cc, kind="stable")[:3]
    assert np.array_equal(np.where(lag < 0, lag + n, lag), order)
    d, lag, v = G.cctde(b, a, n, 1, 16000)
    assert lag[0] == -5 and d[0] == np.float32(-5.0 / 16000)                                                # lags >= fftLen/2 are negative
    d, lag, v = G.cctde(a[:40], b[:40], n, 8, 16000)                                                        # a block shorter than fftLen is zero-padded
    assert lag[0] == 5
    # insertion rule: `>` against the last held value, `>=` against the others; rank 0 seeded with lag 0
    cc = np.zeros(8); cc[0] = 1.0
    assert list(G.cctde_peaks(cc, 3, 8)[1]) == [0, 2, 1]
    cc = np.array([5.0, 5.0, 7.0, 5.0, 0, 0, 0, 0])
    assert list(G.cctde_peaks(cc, 2, 8)[1]) == [2, 1] and list(G.cctde_peaks(cc, 1, 8)[1]) == [2]
    assert list(G.cctde_peaks(np.array([5.0, 5.0, 1, 0, 0, 0, 0, 0]), 1, 8)[1]) == [0]


# ---- host side of the C-ABI ---------------------------------------------------------------------------------------------------------------
NAMES = ["dsr_gcc_create", "dsr_gcc_destroy", "dsr_gcc_set_alpha", "dsr_gcc_alpha", "dsr_gcc_state_bytes", "dsr_gcc_state_init", "dsr_gcc_run",
         "dsr_gcc_find_maximum", "dsr_gcc_state_read", "dsr_gcc_channel_delays", "dsr_gcc_calculate", "dsr_gcc_peak", "dsr_gcc_get", "dsr_cctde_check",
         "dsr_cctde_run", "dsr_cctde_stream_create", "dsr_cctde_stream_next_x", "dsr_cctde_stream_allsamples", "dsr_cctde_stream_get_sample_delays",
         "dsr_cctde_stream_get_cc_values", "dsr_cctde_stream_set_target_frequency_range"]


def test_new_symbols_are_exported_and_declared(dsr):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = set(re.findall(r" T (dsr_[a-z0-9_]+)", out))
    protos = dsr.header_prototypes()
    for n in NAMES:
        assert n in exported and n in protos, n
    # nothing of the two families is exported without a declaration, or declared without being exported
    fam = lambda names: set(n for n in names if n.startswith(("dsr_gcc_", "dsr_cctde_")))
    assert fam(exported) == fam(protos)
    assert protos["dsr_gcc_run"][1][7] is C.c_double and protos["dsr_gcc_state_bytes"][0] is C.c_size_t


def _gcc(dsr, pairs, C_, **kw):
    return dsr.Gcc("phat", pairs, sampleRate=16000.0, fftLen=kw.pop("fftLen", 256), nChan=C_, **kw)


def test_channel_delays_over_pair_graphs(dsr):
    tau = np.array([0.0, 3.0, -2.0, 5.0, 1.0]) / 16000.0
    for pairs in ([(0, 1), (0, 2), (0, 3), (0, 4)], [(1, 0), (2, 1), (2, 3), (4, 3)], [(a, b) for a in range(5) for b in range(a + 1, 5)]):
        d = np.array([tau[a] - tau[b] for a, b in pairs])
        got = _gcc(dsr, pairs, 5).channelDelays(d)
        if pairs[0] == (0, 1) and len(pairs) == 4:
            assert np.array_equal(got, tau)                                                                 # a star against channel 0 is exact
        assert np.abs(got - tau).max() < 1e-18 and got[0] == 0.0
        assert np.abs(got - G.channel_delays(pairs, d, 5)).max() < 1e-18
    # a redundant, inconsistent list: the least-squares solution
    pairs = [(0, 1), (1, 2), (0, 2)]; d = np.array([1.0, 1.0, 2.5]) / 16000.0
    assert np.abs(_gcc(dsr, pairs, 3).channelDelays(d) - G.channel_delays(pairs, d, 3)).max() < 1e-18
    with pytest.raises(dsr.DsrError) as e:
        _gcc(dsr, [(0, 1), (2, 3)], 4).channelDelays([0.0, 0.0])
    assert e.value.status == dsr.E_PARAMETER


def test_create_time_refusals(dsr):
    for n in (255, 100, 4, 8192):
        with pytest.raises(dsr.DsrError) as e:
            _gcc(dsr, [(0, 1)], 2, fftLen=n)
        assert e.value.status == dsr.E_DIMENSION, n
    with pytest.raises(dsr.DsrError) as e:
        _gcc(dsr, [(0, 2)], 2)
    assert e.value.status == dsr.E_INDEX
    g = _gcc(dsr, [(0, 1)], 2, alpha=0.8)
    assert g.getAlpha() == 0.8
    g.setAlpha(0.5); assert g.getAlpha() == 0.5
    assert g.stateBytes(2) > 2 * g.stateBytes(1) - 64 and g.stateBytes(0) == 0
    L = dsr.load()
    assert L.dsr_cctde_check(512, 1) == 0
    assert L.dsr_cctde_check(512, 512) == dsr.E_DIMENSION and L.dsr_cctde_check(500, 1) == dsr.E_DIMENSION and L.dsr_cctde_check(4096, 1) == 0
    assert L.dsr_cctde_check(1 << 19, 8) == 0 and L.dsr_cctde_check(1 << 23, 1) == dsr.E_DIMENSION and L.dsr_cctde_check(4, 1) == dsr.E_DIMENSION
    from dsr.btk import localization, TDEstimator
    assert localization.GCCMLRGnnSubPtr._KIND == "mlrgnnsub" and hasattr(TDEstimator, "CCTDEPtr")


FACADE = r"""
#include "dsr_streams.hpp"
#include <cmath>
#include <cstdio>
int main() {
  try { GCCPhat bad(16000.0, 100, 2, 1); } catch (jdimension_error& e) { printf("dim %d\n", (int) e.getCode()); }
  GCCRaw r; GCCGnnSub s; GCCGnnSubPhat sp; GCCMLRRaw mr; GCCMLRGnnSub m;
  GCCPhatPtr g(new GCCPhat(16000.0, 64, 2, 1));
  g->setAlpha(0.5); printf("alpha %g\n", g->getAlpha());
  SampleFeaturePtr a(new SampleFeature("", 256, 256)), b(new SampleFeature("", 256, 256)), c8(new SampleFeature("", 256, 256));
  c8->setSamples(0, 0, 8000);
  try { CCTDEPtr bad(new CCTDE(a, b, 512, 256)); } catch (jdimension_error& e) { printf("held %d\n", (int) e.getCode()); }
  try { CCTDEPtr bad(new CCTDE(a, c8)); } catch (jdimension_error& e) { printf("rate %d\n", (int) e.getCode()); }
  VectorFeatureStreamPtr c(new CCTDE(a, b, 512, 3)); static_cast<CCTDE*>(c.get())->setTargetFrequencyRange(100, 4000);
  printf("cctde %u %s %d\n", c->size(), c->name().c_str(), c->frameX());
  try {
    CCTDE* t = static_cast<CCTDE*>(c.get());
    std::vector<std::complex<double> > x(64, std::complex<double>(1.0, 0.0));
    g->calculate(x.data(), 0, x.data(), 1, 0, 0.01, true); const double* v = g->findMaximum(-1.0, 1.0); printf("peak %d %.6f\n", (int) (std::fabs(v[0]) < 1e-9), g->getPeakCorr());
    g->getNoisePowerSpectrum(0); g->getNoiseCrossSpectrum(0); g->getCrossSpectrum(); g->getCrossCorrelation(); g->getRatio(); g->getPeakDelay();
    t->next(); t->nextX(1); t->allsamples(); const unsigned* l = t->getSampleDelays(); const double* cc = t->getCCValues(); (void) l; (void) cc; t->reset();
  } catch (j_error& e) { printf("err %d\n", (int) e.getCode()); }
  return 0;
}
"""


def test_cpp_facade_has_the_gcc_and_cctde_classes(tmp_path):
    """host/dsr_streams.hpp: GCCRaw ... GCCMLRGnnSub and CCTDE with the reference's constructor order and method names (localization.h:118-218,
    CCTDE.h:60-101), plain g++; the host-side refusals run everywhere, the device part where there is one."""
    src = tmp_path / "f.cpp"; src.write_text(FACADE); exe = tmp_path / "f"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[:5] == ["dim 4", "alpha 0.5", "held 4", "rate 4", "cctde 3 CCTDE -1"], lines
    # without a device the first calculate() raises JINITIALIZATION (6); with one the flat unit spectra give a one at lag 0, smoothed from the zero
    # cross-spectrum with beta = 0.5 to a peak of exactly 0.5, and the empty sources end (JITERATOR, 8)
    assert lines[5:] in (["err 6"], ["peak 1 0.500000", "err 8"]), lines


def test_cctde_gpu_cases_have_clear_peaks():
    """What tests/test_gpu_gcc.py relies on when it compares every lag: for its seeds, the nHeld + 1 largest values of the restatement differ
    by more than 1e-9 of the scale (block 2: the first two), and a perturbation of 1e-12 of the scale leaves the lags as they are."""
    for n, bl in [(64, 64), (512, 400), (2048, 2048), (4096, 4000), (8192, 8192)]:
        for nHeld in (1, 3, 8):
            a, b = K.cctde_blocks(K.cctde_noise(n, nHeld), n, bl)
            for k in range(6):
                cc = G.cctde_cc(a[k], b[k], n); scale = np.abs(cc).max()
                m = 1 if k == 2 else nHeld                                                                   # block 2: the same samples twice, a one at lag 0 and zeros
                assert np.abs(np.diff(np.sort(cc)[::-1][:m + 1])).min() > 1e-9 * scale, (n, nHeld, k)
                pert = cc + 1e-12 * scale * np.random.default_rng(k).uniform(-1, 1, n)
                assert np.array_equal(G.cctde_peaks(pert, nHeld, 16000)[1][:m], G.cctde_peaks(cc, nHeld, 16000)[1][:m])
    x1, x2 = K.cctde_recording(); b2 = np.zeros(20000, np.float32); b2[:19000] = x2
    cc = G.cctde_cc(x1, b2, 32768)
    assert np.abs(np.diff(np.sort(cc)[::-1][:4])).min() > 1e-9 * np.abs(cc).max() and G.cctde_peaks(cc, 3, 16000)[1][0] == 11

