"""CPU tests for the noise-suppression and binaural-mask operators (include/dsr.h 6a-2, 6a-3): the numpy restatement against independent
forms, the host-side ABI that needs no GPU, and the conditions the GPU tests rely on (comparability of every decision in the shared cases)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import postfilter2_cases as K
from tests import postfilter2_np as P
from tests.conftest import PKG

BAND = 1e-9        # a decision is comparable when its two sides differ by more than this fraction of their magnitude


def comparable(a, b):
    with np.errstate(all="ignore"):
        return ~(np.abs(a - b) <= BAND * np.maximum(np.abs(a), np.abs(b)))      # NaN and inf sides compare the same way on both machines


# ---------------------------------------------------------------------------------------------------------------- restatement vs independent forms
def test_subtraction_is_a_real_gain_on_nonzero_bins():
    """out = X sqrt(S2)/|X| on non-zero bins; a zero bin gives the positive real sqrt(floor)"""
    r = np.random.default_rng(5); M = 64; F = M // 2 + 1
    noise = (r.standard_normal((1, 9, F)) + 1j * r.standard_normal((1, 9, F))) * 0.3
    x = (r.standard_normal((1, 4, F)) + 1j * r.standard_normal((1, 4, F))); x[0, 2, 5] = 0
    s = P.SpectralSubtractor(M, 1.3, 0.01); s.setChannel(-1.0)
    s.run(noise); s.stopTraining(); s.subtract = True
    out = s.run(x)
    N2 = np.mean(np.abs(noise[0]) ** 2, axis=0)
    assert np.allclose(s.psd[0].est, N2, rtol=1e-13)
    S2 = np.maximum(np.abs(x[0]) ** 2 - np.float64(np.float32(1.3)) * N2, np.float64(np.float32(0.01)))
    S2 = np.where(np.abs(x[0]) ** 2 - np.float64(np.float32(1.3)) * N2 <= np.float64(np.float32(0.01)), np.float64(np.float32(0.01)), S2)
    nz = np.abs(x[0]) > 0
    assert np.allclose(out[nz], (x[0] * np.sqrt(S2) / np.where(nz, np.abs(x[0]), 1))[nz], rtol=1e-12)
    assert out[2, 5] == np.sqrt(np.float64(np.float32(0.01)))
    full = P.upper_mirror(out[0], M)
    assert full[M // 2 + 1:].conj()[::-1].tolist() == out[0][1:M // 2].tolist() and full[M // 2] == out[0][M // 2]


def test_recursive_estimate_contains_the_current_frame():
    M = 8; s = P.SpectralSubtractor(M, 1.0, 0.0); s.setChannel(0.5); s.subtract = True
    x = np.full((1, 3, 5), 2.0 + 0j)
    out = s.run(x)
    # estimates 4, 4, 4 -> S2 = 0 <= floor 0 -> 0
    assert np.all(out == 0) and np.all(s.psd[0].est == 4.0)
    s2 = P.SpectralSubtractor(M, 1.0, 0.001); s2.setChannel(-1.0); s2.subtract = True
    assert np.allclose(s2.run(x), 2.0)                                          # alpha < 0: the estimate stays zero until stopTraining


def test_wiener_closed_form_for_constant_inputs():
    """constant |S|^2 = s, |N|^2 = n: PSDs = s and PSDn = n from the first frame on (alpha = 0 for two frames, then a fixed point)"""
    M = 16; F = 9; w = P.WienerFilter(M, 0.8, 0.001, 2.0)
    S = np.full((6, F), 1.0 + 1.0j); N = np.full((6, F), 0.5j)
    out = w.run(S, N); H = 2.0 / (2.0 + 2.0 * 0.25)
    assert np.allclose(out[:, 1:F - 1], S[:, 1:F - 1] * H, rtol=1e-14) and np.all(out[:, 0] == S[:, 0])
    assert np.allclose(out[:, F - 1], np.conj(S[:, F - 1] * H))                 # the Nyquist bin comes out conjugated
    assert w.frames == 6
    # the forgetting factor is 0 for the object's first two frames only, whatever reset() does
    w2 = P.WienerFilter(M, 0.5, 0.001, 1.0); S2 = np.array([np.full(F, a + 0j) for a in (1.0, 2.0, 3.0)]); w2.run(S2, S2)
    assert np.allclose(w2.PSDs[1:], 0.5 * 4.0 + 0.5 * 9.0)
    # updating stopped: PSDn is the stored value
    w2.update = False; before = w2.PSDn.copy(); w2.next(S2[0], None); assert np.array_equal(before, w2.PSDn)


def test_mask_decisions_against_a_brute_force_itd():
    r = np.random.default_rng(7); M = 32; F = 17
    L = r.standard_normal((5, F)) + 1j * r.standard_normal((5, F)); R = r.standard_normal((5, F)) + 1j * r.standard_normal((5, F))
    m = P.MaskFilter(1, 0, M, 3.0, 0.0, 0.01)
    o, mu, (a, b) = m.run(L, R)
    for t in range(5):
        for f in range(1, F):
            d = np.angle(L[t, f]) - np.angle(R[t, f]); itd = min(abs(d), abs(d - 2 * np.pi), abs(d + 2 * np.pi)) / (2 * np.pi * f / M)
            assert abs(itd - a[t, f]) <= 1e-12 * max(1.0, itd)
            want = np.float32(1.0) if itd <= 3.0 else np.float32(0.01)
            assert mu[t, f] == want and o[t, f] == L[t, f] * np.float64(want)
    assert np.array_equal(o[:, 0], L[:, 0])
    m1 = P.MaskFilter(1, 1, M, 3.0, 0.0, 0.01); o1, mu1, _ = m1.run(L, R)
    assert np.all((mu1[:, 1:] == 1) != (mu[:, 1:] == 1))                        # chanX = 1 attenuates the other side


def test_mask_smoothing_is_float_arithmetic():
    m = P.MaskFilter(2, 0, 8, 0.0, 0.3, 0.1); L = np.full((4, 5), 2.0 + 0j); R = np.full((4, 5), 1.0 + 0j)
    _, mu, _ = m.run(L, R)
    a, e, p = np.float32(0.3), np.float32(0.1), np.float32(1.0)
    for t in range(4):
        p = np.float32(np.float32(a * p) + np.float32(np.float32(1) - a)); assert mu[t, 1] == p and mu.dtype == np.float32


def test_per_bin_thresholds_first_call_only_allocates():
    m = P.MaskFilter(2, 0, 8, 0.5, 0.0); th = np.arange(5) * 0.1 + 1.0 / 3
    m.setThresholds(th); assert np.all(m.thr == 0)
    m.setThresholds(th); assert m.thr[0] == 0 and np.array_equal(m.thr[1:], th[1:])
    m.next(np.ones(5, complex), np.ones(5, complex)); assert m.threshold == np.float32(th[4])


def _literal(kind, M, cand, f0, f1, eta, pc, L, R):
    """the reference's triple loop, scalar by scalar"""
    n = cand.size; F = M // 2 + 1
    acc = np.zeros((3, F, n)) if kind == 2 else np.zeros((5 if kind == 0 else 6, n))
    for t in range(L.shape[0]):
        for i in range(n):
            th = float(cand[i])
            if kind == 0:
                PT = PI = 0.0
                for f in range(f0, f1):
                    d = np.arctan2(L[t, f].imag, L[t, f].real) - np.arctan2(R[t, f].imag, R[t, f].real)
                    itd = min(abs(d), abs(d - 2 * np.pi), abs(d + 2 * np.pi)) / (2 * np.pi * f / M)
                    mT, mI = (1.0, eta) if itd <= th else (eta, 1.0)
                    PT += (L[t, f].real * mT) ** 2 + (L[t, f].imag * mT) ** 2; PI += (R[t, f].real * mI) ** 2 + (R[t, f].imag * mI) ** 2
                RT, RI = PT ** pc, PI ** pc
                for q, v in enumerate((RT * RI, RT, RI, RT * RT, RI * RI)):
                    acc[q, i] += v
            else:
                s = np.zeros(6)
                for f in range(f0, f1):
                    PT, PI = abs(L[t, f]), abs(R[t, f])
                    mT = eta if PT <= PI + th else 1.0; mI = eta if PI <= PT + th else 1.0
                    y1T = abs(L[t, f] * mT) ** (2.0 * pc); y1I = abs(R[t, f] * mI) ** (2.0 * pc)
                    v = np.array([y1T, y1I, y1T ** 2, y1I ** 2, y1T ** 4, y1I ** 4])
                    if kind == 1:
                        s += v
                    else:
                        acc[0, f, i] += v[4] + v[5]; acc[1, f, i] += v[0] + v[1]; acc[2, f, i] += v[2] + v[3]
                if kind == 1:
                    acc[:, i] += s
    return acc


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_estimator_accumulators_against_the_literal_triple_loop(kind):
    r = np.random.default_rng(40 + kind); M = 16; F = 9
    L = r.standard_normal((4, F)) + 1j * r.standard_normal((4, F)); R = r.standard_normal((4, F)) + 1j * r.standard_normal((4, F))
    e = P.ThresholdEstimator(kind, M, 0.25 if kind == 0 else -1.0, 6.0 if kind == 0 else 1.0, 0.25, dEta=0.05, dPowerCoeff=0.5).run(L, R)
    ref = _literal(kind, M, e.cand, e.f0, e.f1, e.eta, e.pc, L, R)
    got = e.acc[..., :e.cand.size]
    assert np.allclose(got, ref, rtol=1e-12, atol=0) and e.nSamples == 4


def test_candidate_tables():
    tab, n = P.candidates(0, 0.0, 0.0, 0.02)
    assert tab[0] == np.float32(-0.2 * 16000 / 340) and n == int(np.float64(np.float32(np.float32(tab[0] * -2) / np.float32(0.02))) + 1.5) and tab.size <= n
    tab, n = P.candidates(2, 0.0, 0.0, 1000.0); assert n == 201 and tab.size == 201 and tab[0] == -100000 and tab[-1] == 100000
    assert P.bin_range(64, 1000.0, 6000.0, 16000) == (4, 24) and P.bin_range(64, -1, 6000.0, 16000) == (1, 33)


def test_calc_threshold_rules():
    cand = np.arange(4, dtype=np.float32)
    # IID: first minimum wins; a NaN never wins
    flat = np.zeros(6 * 4 + 1); flat[-1] = 2.0; a = flat[:-1].reshape(6, 4); a[4] = [2.0, 6.0, 6.0, np.nan]
    th, idx, cost, rho, _ = P.calc_threshold(1, cand, 4, 3, flat); assert idx == 1 and th == 1.0
    # FDIID: last minimum wins, per bin and globally
    flat = np.zeros(3 * 3 * 4 + 1); flat[-1] = 1.0; a = flat[:-1].reshape(3, 3, 4); a[0, 1] = [5, 5, 1, 1]; a[0, 2] = [5, 5, 5, 5]
    th, idx, cost, rho, ths = P.calc_threshold(2, cand, 4, 3, flat); assert ths.tolist() == [0.0, 1.0, 3.0] and th == 3.0


# ---------------------------------------------------------------------------------------------------------------- conditions the GPU tests rely on
@pytest.mark.parametrize("c", K.MASK_CASES, ids=lambda c: c["name"])
def test_mask_cases_stay_within_the_comparability_cap(c):
    res, _ = K.mask_reference(c)
    for b, r in enumerate(res):
        bad = ~comparable(r["a"], r["b"])
        for u, n in enumerate(c["nframes"][b]):
            bad[u, n:] = False
        assert bad[:, :, 1:].mean() <= 0.02, (c["name"], b)


@pytest.mark.parametrize("c", K.EST_CASES, ids=lambda c: c["name"])
def test_estimator_cases_have_no_item_near_a_candidate_and_a_clear_minimum(c):
    X = K.est_input(c); e0 = K.est_new(c)
    for b in range(2):
        for u, n in enumerate(c["nframes"][b]):
            for t in range(n):
                for a, bb in e0.sides(X[b][0][u, t].astype(np.complex128), X[b][1][u, t].astype(np.complex128)):
                    assert comparable(a[:, None], bb).all(), (c["name"], b, u, t)        # the cap is zero
    for e in K.est_reference(c):
        if e.nSamples == 0:
            continue
        flat = e.flat(); th, idx, cost, rho, ths = P.calc_threshold(c["kind"], e.cand, e.nCand, e.F, flat)
        if c["pc"] == 0.0:
            continue            # every term is exactly 1.0 and every sum exact in any order: equal rho (or NaN) on both sides, the rule alone decides
        bound = K.acc_bound(K.est_terms(c, e)); r = np.random.default_rng(1); worst = 0.0
        for _ in range(8):                                                              # the bound propagated through the finaliser
            pert = flat.copy(); pert[:-1] *= 1.0 + bound * r.choice([-1.0, 1.0], size=flat.size - 1)
            rho2 = P.calc_threshold(c["kind"], e.cand, e.nCand, e.F, pert)[3]
            worst = max(worst, np.nanmax(np.abs(rho2 - rho)))
        rows = rho.reshape(-1, rho.shape[-1]) if c["kind"] == 2 else rho[None]
        for row in rows[1:] if c["kind"] == 2 else rows:
            # candidates between which no item falls decide every item alike: their sums, and so their rho, are equal bit for bit in the
            # restatement and (wave_scan adds nothing but zeros between them) on the device; the rule then picks among them.  The gap that
            # has to be clear is the one between the smallest rho and the next different value.
            s = np.unique(row[~np.isnan(row)])
            assert s.size < 2 or s[1] - s[0] > 4 * worst, (c["name"], s[:2], worst)


# ---------------------------------------------------------------------------------------------------------------- host-side ABI, no GPU
def test_new_classes_and_argument_errors(dsr):
    with pytest.raises(dsr.DsrError) as e:
        dsr.WienerFilter(256, noiseLen=128)
    assert e.value.status == 5                                                          # jdimension_error (spectralsubtraction.cc:278-281)
    with pytest.raises(dsr.DsrError) as e:
        dsr.SpectralSubtractor(255)
    assert e.value.status == 5
    s = dsr.SpectralSubtractor(64); s.setChannel(-1.0); s.setChannel(0.5); assert s.chanN() == 2
    s.stopTraining(); s.startTraining(); s.setNoiseOverEstimationFactor(2.0)           # flags alone need no state and no device
    with pytest.raises(dsr.DsrError):
        dsr.BinaryMask(3, 0, 64, 0.0, 0.0)
    m = dsr.BinaryMask("iid", 0, 8, 0.25, 0.0); assert m.getThreshold() == 0.25 and m.getThresholds() is None
    th = np.arange(5) * 0.5 + 1
    m.setThresholds(th); assert np.all(m.getThresholds() == 0)                          # the first call only allocates
    m.setThresholds(th); assert np.array_equal(m.getThresholds(), np.r_[0.0, th[1:]])
    m.setThreshold(1.5); assert m.getThreshold() == 1.5


def test_refused_constructor_calls(dsr):
    for kind in ("kim", "iid", "fdiid"):
        with pytest.raises(dsr.DsrError) as e:
            dsr.ThresholdEstimator(kind, 64, 0.0, 1.0, 0.0)
        assert e.value.status == 13                                                     # the loop would not end
    with pytest.raises(dsr.DsrError) as e:
        dsr.ThresholdEstimator("kim", 64, 0.0, 1.0, 0.1, 0.0, 9000.0, 16000)
    assert e.value.status == 5                                                          # the band leaves the half spectrum
    with pytest.raises(dsr.DsrError) as e:
        dsr.ThresholdEstimator("kim", 64, 1.0e8, 1.0e8 + 64.0, 1.0)                      # th += width stalls in float
    assert e.value.status == 13
    with pytest.raises(dsr.DsrError) as e:
        dsr.ThresholdEstimator("kim", 64, 0.0, 1.0, 0.1, 100.0, 4000.0, 0)              # a band with sampleRate 0 divides by it
    assert e.value.status == 13
    with pytest.raises(dsr.DsrError) as e:
        dsr.ThresholdEstimator("kim", 64, 0.0, 1.0, 0.1, 100.0, 3.0e38, 1)                # a quotient no unsigned holds
    assert e.value.status == 5
    with pytest.raises(dsr.DsrError) as e:
        dsr.ThresholdEstimator("iid", 64, -10.0, 10.0, 0.01)                            # 2001 candidates: more than the device window
    assert e.value.status == 5


# (min, max, width) whose float loop yields more values than the (int)((max-min)/width + 1.5) its arrays hold: near 2^20 and 2^16 the sum
# th + width rounds to a step shorter than width (0.28 -> 0.25, 0.011 -> 0.0078125), so the loop takes more steps than the quotient predicts
OVERRUNS = [(1000000.0, 1000010.0, 0.28), (65536.0, 65540.0, 0.011)]


@pytest.mark.parametrize("kind", ["kim", "iid", "fdiid"])
@pytest.mark.parametrize("t", OVERRUNS)
def test_candidate_loops_that_overrun_their_arrays_are_refused(dsr, kind, t):
    with pytest.raises(IndexError):
        P.candidates(0, *t)                                                             # the restatement refuses them
    n = int(np.float64(np.float32(np.float32(np.float32(t[1]) - np.float32(t[0])) / np.float32(t[2]))) + 1.5); th = np.float32(t[0]); count = 0
    while th <= np.float32(t[1]):
        count += 1; th = np.float32(th + np.float32(t[2]))
    assert count > n                                                                    # the literal loop, counted here once more
    with pytest.raises(dsr.DsrError) as e:
        dsr.ThresholdEstimator(kind, 64, *t)
    assert e.value.status == 6                                                          # JINDEX
    ok = dsr.ThresholdEstimator(kind, 64, t[0], t[1], 0.3 if t[2] > 0.1 else 0.0125)     # a neighbouring width that fits is accepted
    tab, nc = P.candidates({"kim": 0, "iid": 1, "fdiid": 2}[kind], t[0], t[1], 0.3 if t[2] > 0.1 else 0.0125); assert ok.nCand == nc and np.array_equal(ok.candidates(), tab)


@pytest.mark.parametrize("c", K.EST_CASES, ids=lambda c: c["name"])
def test_candidate_table_and_band_match_the_restatement(dsr, c):
    e = dsr.ThresholdEstimator(c["kind"], c["M"], c["rng"][0], c["rng"][1], c["rng"][2], c["band"][0], c["band"][1], c["band"][2], c["dEta"], c["pc"])
    r = K.est_new(c)
    assert e.nCand == r.nCand and np.array_equal(e.candidates(), r.cand) and e.binRange() == (r.f0, r.f1) and e.accDoubles == r.flat().size


@pytest.mark.parametrize("c", K.EST_CASES, ids=lambda c: c["name"])
def test_calc_threshold_from_injected_accumulators(dsr, c):
    e = dsr.ThresholdEstimator(c["kind"], c["M"], c["rng"][0], c["rng"][1], c["rng"][2], c["band"][0], c["band"][1], c["band"][2], c["dEta"], c["pc"])
    for r in K.est_reference(c):
        if r.nSamples == 0:
            continue
        flat = r.flat(); keep = flat.copy()
        got = e.calcThreshold(flat); th, idx, cost, rho, ths = P.calc_threshold(c["kind"], r.cand, r.nCand, r.F, flat)
        assert np.array_equal(flat, keep)                                               # the batch finaliser is pure
        assert got["index"] == idx and got["threshold"] == th
        assert np.allclose(got["cost"], cost, rtol=1e-13, atol=0, equal_nan=True)
        if c["kind"] == 2:
            assert np.array_equal(got["thresholds"], ths)
        again = e.calcThreshold(flat, inPlace=True); assert again["index"] == idx and (r.nSamples == 1 or not np.array_equal(flat, keep))   # in place, as the reference


def test_noise_file_round_trip_byte_for_byte(dsr, tmp_path):
    est = np.array([0.0, 1.5, 1.0 / 3.0, 123456.789012345, 2e-7, 1e10] + [0.25] * 27)
    fn = tmp_path / "noise.txt"; dsr.psdFileWrite(fn, est)
    assert open(fn).read() == "".join("%f\n" % v for v in est)                          # "%lf\n" per value (spectralsubtraction.cc:44-46)
    back = dsr.psdFileRead(fn, est.size); assert np.array_equal(back, np.array([float("%f" % v) for v in est]))
    fn2 = tmp_path / "again.txt"; dsr.psdFileWrite(fn2, back); assert open(fn2, "rb").read() == open(fn, "rb").read()
    with pytest.raises(dsr.DsrError) as e:
        dsr.psdFileRead(tmp_path / "missing.txt", 3)
    assert e.value.status == 8


def test_stream_classes_exist():
    from dsr.btk import postfilter as pf
    for n in ("SpectralSubtractorPtr", "WienerFilterPtr", "BinaryMaskFilterPtr", "KimBinaryMaskFilterPtr", "KimITDThresholdEstimatorPtr", "IIDBinaryMaskFilterPtr",
              "IIDThresholdEstimatorPtr", "FDIIDThresholdEstimatorPtr", "averagePSDEstimatorPtr"):
        assert hasattr(pf, n), n


def test_cpp_facade_compiles(tmp_path):
    src = tmp_path / "p.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
#include <cstdio>
int main() {
  try {
    VectorComplexFeatureStreamPtr a, b;
    SpectralSubtractorPtr ss(new SpectralSubtractor(64, false, 1.0f, 0.001f));
    ss->setNoiseOverEstimationFactor(2.0f); ss->startTraining(); ss->startNoiseSubtraction(); ss->stopNoiseSubtraction();
    printf("ss %u\n", ss->size());
    try { KimITDThresholdEstimator bad(a, b, 64, 0.0f, 1.0f, 0.0f); } catch (j_error& e) { printf("refused %d\n", (int) e.getCode()); }
  } catch (j_error& e) { printf("err %d\n", (int) e.getCode()); }
  return 0;
}
""")
    exe = tmp_path / "p"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ss 64" in out.stdout and "refused" in out.stdout


# ---------------------------------------------------------------------------------------------------------------- the device formulation, in numpy
def _canonical_scan(A, reverse):
    """wave_scan of k_binaural.hip: 64 lanes, contiguous chunks, value = (left-to-right sum of the chunk totals before) + (left-to-right sum inside)"""
    n = A.size; ch = (n + 63) // 64; v = A[::-1].copy() if reverse else A.copy(); out = np.zeros(n); tots = []
    for lane in range(64):
        b, e = lane * ch, min(lane * ch + ch, n); base = 0.0
        for tj in tots:
            base += tj
        local = 0.0
        for j in range(b, e):
            local += v[j]; out[j] = base + local
        tots.append(local)
    return out[::-1] if reverse else out


def _binned(e, L, R, rng):
    """accumStats1 of all frames as the device does it: one first-true index per item, two histograms per quantity, two running sums"""
    nL = e.cand.size; W1 = 1025; th = e.cand.astype(np.float64); eta, pc, e2 = e.eta, e.pc, 2.0 * e.pc
    acc = np.zeros_like(e.acc)

    def first_true(pred):
        return int(np.argmax(pred)) if pred.any() else nL

    def sums(items):
        """items: (slot, vTrue, vFalse) in any order (LDS atomics) -> S[i] = sum_{k<=i} vTrue + sum_{k>i} vFalse"""
        T = np.zeros(W1); Fh = np.zeros(W1)
        for k in rng.permutation(len(items)):
            s, vt, vf = items[k]; T[s] += vt; Fh[s] += vf
        T = _canonical_scan(T, False); Fh = _canonical_scan(Fh, True)
        return T[:nL] + Fh[1:nL + 1]

    for t in range(L.shape[0]):
        if e.kind == 0:
            itd = P.calc_itd(e.M, L[t], R[t]); iT, iI = [], []
            for f in range(e.f0, e.f1):
                with np.errstate(all="ignore"):
                    s = first_true(itd[f] <= th)
                l, r = L[t, f], R[t, f]
                iT.append((s, l.real * l.real + l.imag * l.imag, (l.real * eta) ** 2 + (l.imag * eta) ** 2))
                iI.append((s, (r.real * eta) ** 2 + (r.imag * eta) ** 2, r.real * r.real + r.imag * r.imag))
            RT = np.power(sums(iT), pc); RI = np.power(sums(iI), pc)
            for q, v in enumerate((RT * RI, RT, RI, RT * RT, RI * RI)):
                acc[q, :nL] += v
        else:
            sides = [[[], [], []], [[], [], []]]
            for f in range(e.f0, e.f1):
                l, r = L[t, f], R[t, f]; PT = np.hypot(l.real, l.imag); PI = np.hypot(r.real, r.imag)
                for side, (x, a, b) in enumerate(((l, PT, PI), (r, PI, PT))):
                    s = first_true(a <= (b + th)); y1 = np.power(a, e2); yE = np.power(np.hypot(x.real * eta, x.imag * eta), e2)
                    for q, (vt, vf) in enumerate(((yE, y1), (yE * yE, y1 * y1), (yE ** 2 * yE ** 2, y1 ** 2 * y1 ** 2))):
                        sides[side][q].append((s, vt, vf) if e.kind == 1 else (f, s, vt, vf))
            if e.kind == 1:
                for side in range(2):
                    for q in range(3):
                        acc[2 * q + side, :nL] += sums(sides[side][q])
            else:
                for f in range(e.f0, e.f1):
                    for q, plane in ((2, 0), (0, 1), (1, 2)):
                        it = [(s, vt, vf) for side in range(2) for (ff, s, vt, vf) in sides[side][q] if ff == f]
                        acc[plane, f, :nL] += sums(it)
    return acc


@pytest.mark.parametrize("c", [c for c in K.EST_CASES if c["M"] <= 256 and c["T"] <= 8], ids=lambda c: c["name"])
def test_binned_formulation_reproduces_every_decision(c):
    """The O(bins + candidates) formulation the kernels use, restated in numpy with the items added in a random order: accumulators within the
    bound, exact ties of the literal loop stay exact ties, and calcThreshold picks the same index."""
    X = K.est_input(c); ref = K.est_reference(c); rng = np.random.default_rng(3)
    for u, r in enumerate(ref):
        if r.nSamples == 0 or u > 0:
            continue
        e = K.est_new(c); frames = [(X[b][0][u, :c["nframes"][b][u]], X[b][1][u, :c["nframes"][b][u]]) for b in range(2)]
        L = np.concatenate([f[0] for f in frames]).astype(np.complex128); R = np.concatenate([f[1] for f in frames]).astype(np.complex128)
        acc = _binned(e, L, R, rng); want = r.acc
        with np.errstate(all="ignore"):
            rel = np.where(acc == want, 0.0, np.abs(acc - want) / np.abs(want))
        assert np.nanmax(rel) <= K.acc_bound(K.est_terms(c, r)), (c["name"], np.nanmax(rel))
        flat = np.concatenate([acc.ravel(), [float(r.nSamples)]])
        a = P.calc_threshold(c["kind"], r.cand, r.nCand, r.F, flat); b = P.calc_threshold(c["kind"], r.cand, r.nCand, r.F, r.flat())
        assert a[1] == b[1] and a[0] == b[0], (c["name"], a[1], b[1])
        if c["kind"] < 2 and c["pc"] != 0.0:
            tie = lambda rho: np.flatnonzero(np.diff(rho) == 0)
            assert np.array_equal(tie(a[3]), tie(b[3])), c["name"]            # the same runs of exactly equal rho
