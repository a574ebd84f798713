"""Steered-response-power DOA (DOAEstimatorSRPDSBLA): the numpy restatement (tests/doa_srp_np.py) on a synthetic plane wave, and the
host-side half of the C-ABI -- theta grid, look delays, steering table -- against it, without a GPU."""
import numpy as np
import pytest

from tests import doa_srp_np as D

FS, M = 16000, 64


def _plane_wave(C, T, theta0, spacing, seed=5):
    """subband snapshots of one source seen by a uniform linear array: X_c(f) = S(f) exp(-j 2 pi f fs tau_c / M), tau_c = x_c cos(theta0)"""
    rng = np.random.default_rng(seed)
    F = M // 2 + 1
    S = (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))) / np.sqrt(2)
    x = np.arange(C) * spacing
    f = np.arange(F)
    ph = np.exp(-2j * np.pi * np.outer(x * np.cos(theta0), f) * FS / M)
    X = (S[None] * ph[:, None, :]).astype(np.complex64)
    return X, x


def test_plane_wave_peaks_at_nearest_grid_point():
    C, T, theta0 = 8, 40, 0.7
    X, x = _plane_wave(C, T, theta0, 1.0 / FS)
    thetas = D.theta_grid(0.0, np.pi, 0.05)
    out = D.run(X[None], [T], x, FS, M, 3, thetas, 1, M // 2, 0.0)
    assert out["gated"].sum() == 0
    k0 = int(np.argmin(np.abs(thetas - theta0)))
    assert int(np.argmax(out["acc"][0])) == k0
    assert (out["nbest_idx"][0, :, 0] == k0).mean() > 0.9
    # energy = sum_f g_f (sum_c |X_c|^2)^2 / (2 (M/2) C); every channel carries |S|^2
    P = (np.abs(X.astype(np.complex128)) ** 2).mean(axis=0)             # [T][F]
    g = np.where(np.arange(M // 2 + 1) < M // 2, 2.0, 1.0)
    closed = ((C * P[:, 1:]) ** 2 * g[1:]).sum(axis=1) / (2 * (M // 2) * C)
    np.testing.assert_allclose(out["energy"][0], closed, rtol=2e-6)


def test_restatement_energy_is_a_float_accumulation():
    X, _ = _plane_wave(3, 5, 0.3, 1.0 / FS, seed=9)
    X = X * np.float32(1e3)
    e = D.energy(X, 1, M // 2, M)
    assert e.dtype == np.float32
    # the float accumulation stays within float rounding of the same sum taken in double
    Xd = X.astype(np.complex128)
    s = (np.abs(Xd) ** 2).sum(axis=0)
    g = np.where(np.arange(M // 2 + 1) < M // 2, 2.0, 1.0)
    dbl = ((s[:, 1:] ** 2) * g[1:]).sum(axis=1)
    np.testing.assert_allclose(e, dbl / (2 * (M // 2) * 3), rtol=1e-5)


def test_capi_grid_delays_and_table_match_restatement(dsr):
    C = 5
    x = np.array([0.0, 3e-5, 7e-5, 1.2e-4, 1.3e-4, 9.0])                # one position more than channels is fine
    d = dsr.DoaSRP(3, FS, M, C)
    d.setArrayGeometry(x)
    assert d.thetaN() == 31                                              # the constructor's (-pi/2, pi/2, 0.1)
    np.testing.assert_array_equal(d.thetas(), D.theta_grid(-np.pi / 2, np.pi / 2, 0.1))
    d.setSearchParam(0.2, 2.9, 0.15)
    th = D.theta_grid(0.2, 2.9, 0.15)
    assert d.thetaN() == len(th) == 18
    np.testing.assert_array_equal(d.thetas(), th)                       # accumulated, not min + k width
    for t in (0.0, 0.7, th[7]):
        np.testing.assert_allclose(d.lookDelays(t), D.look_delays(x, C, t), rtol=0, atol=1e-15)
    W = D.steering_table(x, C, FS, M, th, 1, M // 2)
    for k in (0, 7, len(th) - 1):
        got = d.steering(k)
        assert got.shape == (M // 2 + 1, C)
        np.testing.assert_allclose(got, W[:, k], rtol=0, atol=1e-15)
        np.testing.assert_array_equal(got[0], np.ones(C))               # bin 0 holds (1, 0), not 1/C
    # the table stays as built until setSearchParam: a range that now starts at 0 uses bin 0's (1, 0)
    d.setFrequencyRange(0, M // 2)
    np.testing.assert_array_equal(d.steering(3)[0], np.ones(C))
    d.setSearchParam(0.2, 2.9, 0.15)                                    # rebuilt with fbinMin = 0: bin 0 is wq_0 = 1/C
    np.testing.assert_allclose(d.steering(3), D.steering_table(x, C, FS, M, th, 0, M // 2)[:, 3], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(d.steering(3)[0], np.full(C, 1.0 / C))


def test_capi_top_bin_only_and_swapped_search(dsr):
    C = 3
    x = np.array([0.0, 6.25e-5, 1.25e-4])
    d = dsr.DoaSRP(2, FS, M, C)
    d.setArrayGeometry(x)
    d.setFrequencyRange(M // 2, M // 2)
    d.setSearchParam(np.pi / 2, 0.0, 0.1)                               # min > max: swapped (beamformer.h:531-537)
    th = D.theta_grid(0.0, np.pi / 2, 0.1)
    np.testing.assert_array_equal(d.thetas(), th)
    W = D.steering_table(x, C, FS, M, th, M // 2, M // 2)
    for k in range(len(th)):
        np.testing.assert_allclose(d.steering(k)[: M // 2 + 1], W[:, k], rtol=0, atol=1e-15)


def test_capi_errors(dsr):
    d = dsr.DoaSRP(2, FS, M, 4)
    with pytest.raises(dsr.DsrError) as e:
        d.steering(0)                                                   # no geometry: the reference dereferences NULL
    assert e.value.status == 1
    d.setArrayGeometry([0.0, 1e-4, 2e-4])                               # fewer positions than channels: the reference reads out of bounds
    with pytest.raises(dsr.DsrError) as e:
        d.steering(0)
    assert e.value.code == 4                                            # JDIMENSION
    with pytest.raises(dsr.DsrError):
        d.setFrequencyRange(0, M // 2 + 1)
    with pytest.raises(dsr.DsrError):
        d.setSearchParam(0.0, 1.0, 0.0)
    d.setArrayGeometry([0.0, 1e-4, 2e-4, 3e-4])
    d.steering(0)
    with pytest.raises(dsr.DsrError) as e:
        d.steering(31)
    assert e.value.code == 5                                            # JINDEX
    R, I = d.finalNBest(np.array([[1.0, 3.0, 3.0, 2.0] + [0.0] * 27]))   # strict >: the earlier of a tie ranks first
    np.testing.assert_array_equal(I[0], [1, 2])
    np.testing.assert_array_equal(R[0], [3.0, 3.0])
