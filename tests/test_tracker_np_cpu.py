"""CPU tests of the tracker restatement (tests/tracker_np.py), of the library's host side against it, and of the conditions the GPU parity
test (tests/test_gpu_tracker.py) rests on: every case of tests/tracker_cases.py must make the same decisions in float64 and in the second
precision, with the margins below, so that a last-bit difference on the device cannot flip one."""
import math

import numpy as np
import pytest

from tests import sph_np as S
from tests import tracker_cases as Cs
from tests import tracker_np as T


def test_pinned_values():
    # the tracker's harmonic is tests/sph_np.py's with phi negated (e^{-i m phi}, tracker.cc:335)
    for n in range(4):
        for m in range(-n, n + 1):
            for th, ph in ((0.3, 0.9), (1.7, -2.2)):
                assert abs(T.harmonic(n, m, th, ph) - S.Y(m, n, th, -ph)) <= 1e-15
    # ka == 0 -> 1 for every order, so _bn = 4 pi i^n at bin 0
    d = T.Decomposition(False, 3, 32, 42.0, 16000.0)
    assert np.array_equal(d.bn[0], 4.0 * math.pi * np.array([1, 1j, -1, -1j]))
    for n in range(12):
        assert T.modal_coefficient(n, 0.0) == 1.0
    # the closed forms against the Bessel form  j_n - j_n'/h_n' h_n  (a check of the restated coefficients, orders 1-8): equal up to a sign;
    # the reference's forms of orders 2, 5 and 6 are the negative of it, which is kept
    for n in range(1, 9):
        for ka in (0.4, 1.3, 3.1):
            jn, yn = S.jl(n, ka), S.yl(n, ka)
            djn = S.jl(n - 1, ka) - (n + 1) / ka * jn
            dyn = S.yl(n - 1, ka) - (n + 1) / ka * yn
            want = jn - djn / complex(djn, dyn) * complex(jn, yn)
            sign = -1 if n in (2, 5, 6) else 1
            assert abs(T.modal_coefficient(n, ka) - sign * want) <= 1e-9 * abs(want), (n, ka)
    # the EigenMike table: tracker.cc:195-297 is the table of tests/sph_np.py (modalBeamformer.cc:414-535) entry by entry
    th, ph = T.eigenmike()
    assert np.array_equal(np.round(th * 180 / math.pi).astype(int), S.EM_THETA) and np.array_equal(np.round(ph * 180 / math.pi).astype(int), S.EM_PHI)
    assert S.EM_THETA[30] == 122 and S.EM_PHI[15] == 89 and len(S.EM_THETA) == 32


def test_harmonic_derivatives():
    th, ph, h = 0.7, 0.3, 1e-6
    for n in range(4):
        for m in range(-n, n + 1):
            fd_t = (T.harmonic(n, m, th + h, ph) - T.harmonic(n, m, th - h, ph)) / (2 * h)
            fd_p = (T.harmonic(n, m, th, ph + h) - T.harmonic(n, m, th, ph - h)) / (2 * h)
            et = abs(T.harmonic_deriv_polar(n, m, th, ph) - fd_t)
            ep = abs(T.harmonic_deriv_azimuth(n, m, th, ph) - fd_p)
            print("n %d m %2d: d/dtheta error %.3e, d/dphi error %.3e" % (n, m, et, ep))
            if m >= 0:
                assert et <= 1e-6 and ep <= 1e-6, (n, m)
            else:
                # pinned: the restated value is the positive degree's derivative with the reference's own sign and scale rules
                y = T.harmonic_deriv_polar(n, m, th, ph)
                want = -T.calculate_normalization(n, m) * T.calculate_dpnm_dtheta(n, m, th) * math.sin(th) * complex(math.cos(-m * ph), math.sin(-m * ph))
                assert abs(y - want) <= 1e-15 * max(1.0, abs(want))
                assert ep <= 1e-6                                         # the azimuth derivative is exact for every degree


def _random_update(seed, K_=3, L=5):
    rng = np.random.default_rng(seed)
    N = K_ * L
    n2 = 2 * N
    Vb = []
    for _ in range(K_):
        A = rng.standard_normal((2 * L, 2 * L))
        Vb.append(np.linalg.cholesky(A @ A.T + 2 * L * np.eye(2 * L)))
    H = rng.standard_normal((n2, 2))
    Kk = np.linalg.cholesky(np.array([[2.0, 0.3], [0.3, 1.0]]))
    Uu = 0.1 * np.eye(2)
    r = rng.standard_normal(n2)
    P = np.zeros((n2 + 2, n2 + 4))
    for k in range(K_):
        s = slice(2 * k * L, 2 * (k + 1) * L)
        P[s, s] = Vb[k]
    P[:n2, n2:n2 + 2] = H @ Kk
    P[n2:, n2:n2 + 2] = Kk
    P[n2:, n2 + 2:] = Uu
    return P, n2, r, H, Kk, Vb


def test_update_is_the_square_root_kalman_step():
    for seed in range(3):
        P, n2, r, H, Kk, Vb = _random_update(seed)
        post, corr = T.dense_update(P, n2, r)
        a, b = post @ post.T, P @ P.T
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max()
        assert np.abs(np.triu(post[:, :n2 + 2], 1)).max() == 0.0 and np.abs(post[:, n2 + 2:]).max() == 0.0
        V = np.zeros((n2, n2))
        L2 = Vb[0].shape[0]
        for k, v in enumerate(Vb):
            V[k * L2:(k + 1) * L2, k * L2:(k + 1) * L2] = v
        conv = Kk @ Kk.T @ H.T @ np.linalg.solve(H @ Kk @ Kk.T @ H.T + V @ V.T, r)
        assert np.abs(corr - conv).max() <= 1e-9 * np.abs(conv).max()


def test_streaming_givens_is_bit_identical():
    for seed in range(3):
        P, n2, r, _, _, _ = _random_update(seed, K_=4, L=3)
        post, corr = T.dense_update(P, n2, r)
        scorr, A22 = T.streaming_update(lambda j: P[j:, j], P[:, n2], P[:, n2 + 1], P[n2:, n2 + 2:], r)
        assert np.array_equal(scorr, corr) and np.array_equal(A22, post[n2:, n2:n2 + 2])
    with pytest.raises(ArithmeticError):
        T.calc_givens(0.0, 0.0)


@pytest.mark.parametrize("case", Cs.CASES, ids=[c["name"] for c in Cs.CASES])
def test_case_is_well_conditioned(case):
    """a condition, not a measurement: both precisions decide alike on every frame, and no decision is close"""
    ref = Cs.reference(case)
    a, b = ref["ref"], ref["second"]
    assert np.array_equal(a["info"], b["info"])
    _, F, U, _, frames = Cs.dims(case)
    Kn = case["useSubbandsN"] or F
    for u in range(U):
        assert len(a["logs"][u]) == frames[u]
        for la, lb in zip(a["logs"][u], b["logs"][u]):
            assert la["sels"] == lb["sels"] and la["iters"] == lb["iters"] and la["clamp"] == lb["clamp"]
            for sa in la["sortedAbs"]:
                top = sa[:Kn + 1]
                if case["only"]:                                         # the source's bins apart from each other and from the rest, which is exactly zero on
                    top = top[:len(case["only"]) + 1]                    # both sides (0 / delta): there the tie rule decides, not rounding
                    assert not sa[len(case["only"]):].any()
                assert ((top[:-1] - top[1:]) / top[:-1]).min() > 1e-9
            for ratio in la["ratios"]:
                assert abs(ratio - T.TOLERANCE) >= 1e-3 * T.TOLERANCE
    if case["name"] == "modal-clamp":
        assert any(l["clamp"] for lg in a["logs"] for l in lg)
    kept = [set(s) for lg in a["logs"] for l in lg for s in l["sels"]]
    if case["name"] in ("modal-F257", "spatial-F257"):                   # a kept bin that is the second bin of a thread of k_trk_run (NT = 256)
        assert F == 257 and any(max(s) >= 256 for s in kept), kept
    if case["name"] == "modal-ties":                                     # the two live bins, then the lowest of the zeros
        assert kept and all(s == {200, 256, 0, 1} for s in kept), kept
        assert all(sorted(s[:2]) == [200, 256] and s[2:] == [0, 1] for lg in a["logs"] for l in lg for s in l["sels"])
    print("%s: s_case = %.3e (%s)" % (case["name"], ref["s_case"], "float64 vs long double" if Cs.WIDE else "float64 vs reversed sums"))
    assert ref["s_case"] < 1e-9                                           # the filter does not amplify rounding: the GPU bound stays meaningful


def test_vectorised_simulator_of_the_cases_is_the_restated_one():
    dec = Cs.sim_decomposition()
    want = T.plane_wave_coefficients(dec, 0.61, 0.23)
    assert np.abs(Cs.pws_coefficients(dec, 0.61, 0.23) - want).max() <= 1e-15 * np.abs(want).max()
    block = np.arange(1, Cs.M + 1) * (1 + 0.5j)
    out = T.PlaneWaveSimulator(dec, 3, 0.61, 0.23).next(block)
    assert np.array_equal(out[Cs.M - 5], np.conj(out[5])) and out[0].imag != 0
    prod = want[3] * block[:Cs.F]                                        # element by element or vectorised: a few ulps apart
    assert np.abs(out[:Cs.F] - prod).max() <= 4 * np.finfo(np.float64).eps * np.abs(prod).max()


def test_library_host_side_equals_the_restatement(dsr):
    for kind, order in (("modal", 3), ("spatial", 2)):
        t = dsr.SphTracker(kind, order, Cs.M, Cs.A_MM, Cs.FS, 4)
        d = T.Decomposition(kind == "spatial", order, Cs.M, Cs.A_MM, Cs.FS, 4)
        assert np.array_equal(t.bn(), d.bn) and np.array_equal(t.sensorHarmonics(), d.sc)
        assert (t.modesN, t.L, t.useSubbandsN) == (d.modesN, d.L, d.useSubbandsN)
    th, ph = dsr.SphTracker.geometry()
    eth, eph = T.eigenmike()
    assert np.array_equal(th, eth) and np.array_equal(ph, eph)
    for n in range(4):
        for m in range(-n, n + 1):
            assert abs(dsr.SphTracker.harmonic(n, m, 0.7, 0.3) - T.harmonic(n, m, 0.7, 0.3)) <= 1e-15
            assert abs(dsr.SphTracker.harmonicDerivPolarAngle(n, m, 0.7, 0.3) - T.harmonic_deriv_polar(n, m, 0.7, 0.3)) <= 1e-14
            assert abs(dsr.SphTracker.harmonicDerivAzimuth(n, m, 0.7, 0.3) - T.harmonic_deriv_azimuth(n, m, 0.7, 0.3)) <= 1e-15
    for n in range(11):                                                    # closed forms 0-8, the Bessel branch above
        for ka in (0.0, 0.3, 1.7, 4.0):
            want = T.modal_coefficient(n, ka)
            assert abs(dsr.SphTracker.modalCoefficient(n, ka) - want) <= 1e-13 * max(1.0, abs(want))
    t = dsr.SphTracker("modal", Cs.SIM_ORDER, Cs.M, Cs.A_MM, Cs.FS)
    assert np.array_equal(dsr.PlaneWaveSim(t, 0.6, 0.2).coef, T.plane_wave_coefficients(Cs.sim_decomposition(), 0.6, 0.2))
    # setV: the literal realification and the Cholesky factor
    case = Cs.BY_NAME["modal-setV"]
    Vs = Cs.inputs(case)[2]
    trk = Cs.make_tracker(case)
    t = dsr.SphTracker("modal", 2, Cs.M, Cs.A_MM, Cs.FS, 4, Cs.SIGMA2_U, Cs.SIGMA2_V, Cs.SIGMA2_INIT)
    for f in range(Cs.F):
        t.setV(Vs[f], f)
        assert np.array_equal(t.getV(f), trk.V[f])
    assert np.abs(np.triu(t.getV(3), 1)).max() == 0.0


def test_facade_and_argument_errors(dsr):
    from dsr.btk import beamformer as B
    dec = B.ModalDecompositionPtr(2, Cs.M, Cs.A_MM, Cs.FS, 4)
    sdec = B.SpatialDecompositionPtr(2, Cs.M, Cs.A_MM, Cs.FS)
    assert (dec.orderN(), dec.modesN(), dec.subbandsN2(), dec.useSubbandsN(), dec.subbandLengthN()) == (2, 9, Cs.M // 2, 4, 9)
    assert (sdec.useSubbandsN(), sdec.subbandLengthN()) == (Cs.F, 32)
    assert abs(dec.harmonic(2, -1, 0.4, 0.2) - T.harmonic(2, -1, 0.4, 0.2)) <= 1e-15 and dec.modalCoefficient(1, 0) == 4j * math.pi
    trk = B.ModalSphericalArrayTrackerPtr(dec)
    strk = B.SpatialSphericalArrayTrackerPtr(sdec, 10.0, 10.0, 10.0, 2, "t")
    assert trk.size() == 2 and trk.name() == "ModalSphericalArrayTracker" and strk.name() == "t" and trk.chanN() == 0
    trk.setInitialPosition(0.4, 0.1); trk.nextSpeaker()
    with pytest.raises(dsr.DsrError):
        B.ModalSphericalArrayTrackerPtr(sdec)
    E_ARG = dsr.E_PARAMETER                                                # DSR_E_ARG of include/dsr.h
    with pytest.raises(dsr.DsrError) as e:
        dsr.SphTracker("modal", 2, Cs.M, chanN=16)
    assert e.value.status == E_ARG
    with pytest.raises(dsr.DsrError) as e:
        B.SpatialSphericalArrayTrackerPtr(B.SpatialDecompositionPtr(3, 512, 42.0, 16000.0))   # 2N = 2 x 257 x 32
    assert e.value.status == E_ARG and dsr.SphTracker.maxRows("spatial", 3, 257) < 2 * 257 * 32
    bad = -np.eye(9, dtype=np.complex128)
    before = trk._trk.getV(2)
    with pytest.raises(dsr.DsrError) as e:
        trk.setV(bad, 2)
    assert e.value.status == E_ARG and np.array_equal(trk._trk.getV(2), before)


def test_create_refuses_one_bin_past_the_lds_row_limit(dsr):
    """dsr_trk_create at the edge of dsr_trk_max_rows, modal order 2 (L = 9): the largest useSubbandsN whose 2 K L rows fit constructs, the
    next one is an argument error.  The limit depends on K itself (the selected bins take K ints of the same LDS), so it is asked per K."""
    L, fftLen = 9, 2048                                                    # 1025 bins: more than any K the limit admits
    fits = [K_ for K_ in range(1, fftLen // 2 + 1) if 2 * K_ * L <= dsr.SphTracker.maxRows("modal", 2, K_)]
    Kmax = fits[-1]
    assert fits == list(range(1, Kmax + 1)) and Kmax + 1 <= fftLen // 2 + 1
    lim = dsr.SphTracker.maxRows("modal", 2, Kmax)
    # the figure itself: 160 KiB of doubles less the per-mode tables (8 x 9), the reduction scratch (256), 32 scalars, the K selected bins as ints
    # and one spare, in three columns of 2N + 2 rows
    assert lim == (160 * 1024 // 8 - (8 * 9 + 256 + 32 + (Kmax + 1) // 2 + 1)) // 3 - 2
    assert 2 * Kmax * L <= lim < 2 * (Kmax + 1) * L
    t = dsr.SphTracker("modal", 2, fftLen, Cs.A_MM, Cs.FS, Kmax)
    assert (t.useSubbandsN, t.L) == (Kmax, L)
    with pytest.raises(dsr.DsrError) as e:
        dsr.SphTracker("modal", 2, fftLen, Cs.A_MM, Cs.FS, Kmax + 1)
    assert e.value.status == dsr.E_PARAMETER and "rows exceed" in str(e.value)
    # the spatial case of the GPU test that passes 64 KiB is inside the limit, and far from it
    assert 2 * 41 * 32 <= dsr.SphTracker.maxRows("spatial", 2, 41)
