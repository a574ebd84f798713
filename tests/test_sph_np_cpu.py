"""The spherical-array host math (dsr_sph, csrc/sph.cpp) without a GPU: the restatement tests/sph_np.py against scipy where scipy is
importable, every host table read through the C-ABI against the restatement, the (theta, phi) grid rules, the N-best tie rule and the
error paths."""
import math

import numpy as np
import pytest

from tests import doa_srp_np as D
from tests import sph_np as S

FS, M = 16000, 256


def _scipy():
    try:
        import scipy.special as sp
    except ImportError:
        pytest.skip("scipy is not importable here")
    return sp


KA = np.concatenate([np.linspace(1e-3, 6.2, 157), [0.05, 0.5, 1.0, 3.0, 6.2]])   # the EigenMike's ka at 16 kHz reaches 6.2


@pytest.mark.parametrize("l", range(10))
def test_bessel_against_scipy(l):
    sp = _scipy()
    for x in KA:
        j, jr = S.jl(l, x), sp.spherical_jn(l, x)
        y, yr = S.yl(l, x), sp.spherical_yn(l, x)
        if abs(jr) > 1e-200:
            assert abs(j - jr) <= 1e-12 * abs(jr) + 1e-300, (l, x, j, jr)
        assert abs(y - yr) <= 1e-12 * abs(yr), (l, x, y, yr)
    assert S.jl(0, 0.0) == 1.0 and S.jl(3, 0.0) == 0.0


def test_harmonics_against_scipy():
    sp = _scipy()
    rng = np.random.default_rng(2)
    for _ in range(40):
        th, ph = rng.uniform(0, np.pi), rng.uniform(-np.pi, 2 * np.pi)
        for n in range(10):
            for m in range(-n, n + 1):
                ref = sp.sph_harm_y(n, m, th, ph) if hasattr(sp, "sph_harm_y") else sp.sph_harm(m, n, ph, th)
                got = S.Y(m, n, th, ph)
                assert abs(got - ref) <= 1e-12 * max(abs(ref), 1.0), (n, m, th, ph)


def test_mode_amplitude_closed_forms_agree_with_bessel_formula():
    """orders 0-3 by the reference's closed forms and by the j_l / y_l formula (order 0 with j_-1 = cos x / x, y_-1 = sin x / x), away from
    the small-ka cancellation; j_l and y_l are pinned against scipy above"""
    for ka in (0.8, 1.5, 3.0, 6.2):
        for n in (0, 1, 2, 3):
            a, b = S.mode_amplitude(n, ka), S.mode_amplitude(n, ka, closed=False)
            assert abs(a - b) <= 1e-10 * abs(b)


@pytest.fixture
def em(dsr):
    def make(kind="EB", maxOrder=8, nBest=2, **kw):
        s = dsr.SphDoaSRP(kind, nBest, FS, M, 32, maxOrder, **kw); s.setEigenMikeGeometry(); return s
    return make


@pytest.mark.parametrize("maxOrder", [1, 4, 8])
def test_tables_match_restatement(em, maxOrder):
    s = em(maxOrder=maxOrder)
    a, th, ph = S.eigenmike()
    assert s.getArrayGeometry(0).tolist() == th.tolist() and s.getArrayGeometry(1).tolist() == ph.tolist()
    B = S.mode_amplitudes(a, FS, M, maxOrder)
    Bc = s.modeAmplitudes()
    assert np.all(Bc[0] == 1)                                                # ka = 0: (1, 0) for every order
    # orders 0-3 use the reference's closed forms, which cancel badly at small ka (b_3 at the first bins is mostly rounding): compare each
    # b_n against the largest |b_n| of its bin, not against itself
    assert np.all(np.abs(Bc - B) <= 1e-12 * np.abs(B).max(axis=1, keepdims=True))
    Sh = S.sensor_harmonics(maxOrder, th, ph)
    assert np.abs(s.harmonics() - Sh).max() <= 1e-13
    wng = s.calcWNG()
    ref = np.array([sum((2 * n + 1) * abs(Bc[f, n]) ** 2 for n in range(maxOrder)) ** 2 * 32 / np.pi ** 2 for f in range(M // 2 + 1)])
    assert np.allclose(wng, ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize("kind,kw", [("EB", {}), ("DS", {}), ("EB", dict(normalizeWeight=True)), ("DS", dict(normalizeWeight=True))])
def test_look_weights_match_restatement(em, kind, kw):
    s = em(kind=kind, maxOrder=4, **kw)
    Bc = s.modeAmplitudes()
    opts = dict(normalize=bool(kw.get("normalizeWeight")))
    W = S.look_weights(kind, Bc, 4, 32, 0.0, 0.0, **opts)                   # default look direction (0, 0)
    assert np.abs(s.lookWeights() - W).max() <= 1e-13 * np.abs(W).max()
    s.setLookDirection(1.2, -0.4)
    if kind == "EB":
        s.setSigma2(0.01); opts["sigma2"] = 0.01
    if opts["normalize"]:
        s.setWeightGain(2.5); opts["wgain"] = 2.5
    W = S.look_weights(kind, Bc, 4, 32, 1.2, -0.4, **opts)
    Wc = s.lookWeights()
    assert np.abs(Wc - W).max() <= 1e-13 * np.abs(W).max()
    assert Wc[0, 0] == 1 and np.all(Wc[0, 1:] == 0)                          # calcDCWeights


def test_grid_rules(em):
    s = em()
    assert s.gridN() == (25, 25)                                             # the constructor's (-pi, pi, -pi, pi, 0.25, 0.25)
    th, ph = s.grid()
    rt, rp, nT, nP = S.grid(-np.pi, np.pi, -np.pi, np.pi, 0.25, 0.25)
    assert (nT, nP) == (25, 25) and np.array_equal(th, rt) and np.array_equal(ph, rp)
    t = -np.pi
    for _ in range(7):
        t += 0.25                                                            # accumulated, not min + k width
    assert th[7 * 25] == t
    s.setSearchParam()                                                       # setSearchParam() defaults: (0, pi, -pi, pi, 0.1, 0.1)
    assert s.gridN() == (31, 63) and s.units() == 1953
    s.setSearchParam(1.0, 2.0, 3.0, 3.9, 0.5, 0.5)
    th, ph = s.grid()
    assert s.gridN() == (2, 2) and th.tolist() == [1.0, 1.0, 1.5, 1.5] and ph.tolist() == [3.0, 3.5, 3.0, 3.5]


def test_grid_width_and_empty_errors(dsr, em):
    s = em()
    with pytest.raises(dsr.DsrError) as e:
        s.setSearchParam(0.0, 1.0, 0.0, 1.0, 0.0, 0.1)
    assert e.value.status == dsr.E_PARAMETER
    s.setSearchParam(1.0, 0.0, 0.0, 1.0, 0.1, 0.1)                           # not swapped: an empty grid at the first use
    with pytest.raises(dsr.DsrError) as e:
        s.steering(0)
    assert e.value.status == dsr.E_PARAMETER


def test_steering_table_and_lifetime(dsr, em):
    s = em(kind="DS", maxOrder=3)
    s.setSearchParam(0.2, 1.0, -0.5, 0.5, 0.4, 0.5)
    s.setFrequencyRange(3, 40)
    th, ph = s.grid()
    Bc = s.modeAmplitudes()
    W = S.steering_table("DS", Bc, 3, 32, th, ph, 3, 40)
    g0 = dsr._lib.dsr_sph_table_generation(s.h)
    for k in range(len(th)):
        w = s.steering(k)
        assert np.all(w[0] == 1) and np.all(w[1:3] == 0) and np.all(w[41:] == 0)
        assert np.abs(w[:41] - W[:, k]).max() <= 1e-13 * np.abs(W).max()
    assert dsr._lib.dsr_sph_table_generation(s.h) == g0 + 1
    s.setFrequencyRange(1, 60)                                               # kept: the table is not rebuilt
    assert np.all(s.steering(0)[41:] == 0) and dsr._lib.dsr_sph_table_generation(s.h) == g0 + 1
    s.setSearchParam(0.2, 1.0, -0.5, 0.5, 0.4, 0.5)                          # a new table at the next use
    assert np.any(s.steering(0)[50] != 0) and dsr._lib.dsr_sph_table_generation(s.h) == g0 + 2
    s.setFrequencyRange(0, 5); s.setSearchParam(0.2, 1.0, -0.5, 0.5, 0.4, 0.5)
    w = s.steering(1)
    Wl = S.weights("DS", Bc[0], S.harmonics_at(3, th[1], ph[1]), 3, 32)
    assert np.abs(w[0] - Wl).max() <= 1e-13 * np.abs(Wl).max()              # fbinMin = 0: bin 0 holds weights


def test_path_choice(em):
    s = em(maxOrder=4); s.setSearchParam()
    assert s.path() == "fused"                                               # 16 (32 + 1953) < 32 1953
    s = em(maxOrder=8); s.setSearchParam()
    assert s.path() == "folded"                                              # 64 (32 + 1953) >= 32 1953


def test_final_nbest_tie_rule(em):
    s = em(nBest=3); s.setSearchParam(0.0, 1.0, 0.0, 1.0, 0.5, 0.5)          # 2 x 2 units
    acc = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0]])
    s.steering(0)                                                            # the table exists
    R, I = s.finalNBest(acc)
    assert I[0].tolist() == [1, 2, 3] and R[0].tolist() == [3.0, 3.0, 2.0]   # on a tie the earlier unit stays ahead
    assert I[1].tolist() == [0, 1, 2]
    Rr, Ir = D.nbest(acc[0], 3)
    assert Ir.tolist() == I[0].tolist()


def test_error_paths(dsr):
    def status(fn, *a):
        with pytest.raises(dsr.DsrError) as e:
            fn(*a)
        return e.value.status
    assert status(dsr.SphDoaSRP, "EB", 1, FS, M, 32, 9) == dsr.E_DIMENSION
    with pytest.raises(dsr.DsrError, match="1..8 supported"):               # the message names the limit
        dsr.SphDoaSRP("EB", 1, FS, M, 32, 9)
    assert status(dsr.SphDoaSRP, "EB", 0, FS, M, 32, 4) == dsr.E_PARAMETER
    assert status(dsr.SphDoaSRP, "EB", 1, FS, M, 32, 4, False, True) == dsr.E_PARAMETER        # halfBandShift
    s = dsr.SphDoaSRP("DS", 1, FS, M, 4, 2)
    assert status(s.modeAmplitudes) == 1                                     # no geometry: DSR_E_ERROR
    assert status(s.setEigenMikeGeometry) == dsr.E_DIMENSION                 # 32 positions, 4 channels
    assert status(s.setArrayGeometry, 40.0, [0.1, 0.2, 0.3], [0, 1, 2]) == dsr.E_DIMENSION
    assert status(s.setArrayGeometry, 0.0, [0.1, 0.2, 0.3, 0.4], [0, 1, 2, 3]) == 1        # a = 0
    s.setArrayGeometry(40.0, [0.1, 0.2, 0.3, 0.4], [0, 1, 2, 3])
    assert s.modeAmplitudes().shape == (M // 2 + 1, 2)
    assert status(s.setFrequencyRange, 0, M // 2 + 1) == dsr.E_DIMENSION


def test_grid_bounded_by_table_size(dsr, em):
    s = em(maxOrder=8)
    s.setSearchParam(0.0, np.pi, -np.pi, np.pi, 1e-3, 1e-3)                  # 3142 x 6283 units: the table would need ~ 2.6e11 entries
    with pytest.raises(dsr.DsrError, match="at most") as e:
        s.steering(0)
    assert e.value.status == dsr.E_DIMENSION


def test_python_class_defaults_and_geometry_getters_before_channels(dsr):
    from dsr.btk.beamformer import DOAEstimatorSRPEBPtr, DOAEstimatorSRPSphDSBPtr, EigenBeamformerPtr, SphericalDSBeamformerPtr
    # beamformer.i's Python constructors (%extend): maxOrder 8 for EB and both DOA classes, 3 for SphericalDS
    assert EigenBeamformerPtr(FS).dim() == 64 and SphericalDSBeamformerPtr(FS).dim() == 9
    eb, ds = DOAEstimatorSRPEBPtr(1, FS), DOAEstimatorSRPSphDSBPtr(1, FS)
    assert eb.dim() == 64 and ds.dim() == 64 and eb._nm == ds._nm == "DirectionEstimatorSRPMB"
    # the geometry getters work once a geometry is set, before any setChannel
    bf = SphericalDSBeamformerPtr(FS, M)
    with pytest.raises(dsr.DsrError) as e:
        bf.getModeAmplitudes()
    assert e.value.status == 1                                               # no geometry yet: DSR_E_ERROR
    bf.setEigenMikeGeometry()
    a, th, ph = S.eigenmike()
    assert np.allclose(bf.getModeAmplitudes(), S.mode_amplitudes(a, FS, M, 3), rtol=0, atol=1e-12)
    assert bf.getArrayGeometry(0).tolist() == th.tolist() and bf.calcWNG().shape == (M // 2 + 1,)
    assert bf.chanN() == 0
