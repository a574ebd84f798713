"""CPU tests of the information-filter echo cancellers: the numpy restatement tests/aec_info_np.py against independent forms (the Givens sweeps
are unitary right-multiplications, the three inversion routes agree, the skip counter is the serial count), that the square-root kind cancels
an echo under steady near-end noise, that the inputs of the GPU comparison are admissible (no gate decision near its threshold), and the
host-side C-ABI without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import aec_info_np as I
from tests import aec_np as N


def _gram(S):
    return S @ np.conj(np.swapaxes(S, 1, 2))


def _close(a, b, tol=1e-12):
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


def _lower(K):
    return not np.triu(K, 1).any()


@pytest.mark.parametrize("L", [1, 2, 3, 8, 32])
def test_givens_sweeps_are_unitary_and_keep_k_lower_triangular(L):
    rng = np.random.default_rng(100 + L); n = 4
    K = np.tril(rng.standard_normal((n, L, L)) + 1j * rng.standard_normal((n, L, L))) + 3.0 * np.eye(L)
    Su = np.tile(np.eye(L, dtype=np.complex128) / np.sqrt(10e-4), (n, 1, 1))
    info = rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
    # temporal update: the rows of the post-array have the Gram matrix of the pre-array's
    pre = I.temporal_prearray(K, Su, info); post = I.temporal_sweep(pre.copy())
    assert _close(_gram(post), _gram(pre))
    K1, info1 = post[:, L:2 * L, L:], post[:, 2 * L, L:]
    assert _lower(K1) and not post[:, :L, L:].any()                                 # A12 is gone, A22 is lower triangular again
    # observational update
    v = 30.0 * (rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))); Ak = rng.standard_normal(n) + 1j * rng.standard_normal(n); sv = rng.uniform(0.5, 2.0, n)
    pre = I.observational_prearray(K1, info1, v, Ak, sv); post = I.observational_sweep(pre.copy())
    assert _close(_gram(post), _gram(pre))
    K2, info2 = post[:, :L, :L], post[:, L, :L]
    assert _lower(K2) and not post[:, :L, L].any()
    # diagonal loading, one pass at a time and as a whole: K K^H gains load^2 I
    load = 0.1
    Z = np.zeros((n, L, L + 1), np.complex128); Z[:, :, :L] = K2
    for d in range(L):
        Z[:, :, L] = 0.0; Z[:, d, L] = load
        pre = Z.copy(); I.loading_sweep(Z, d)
        assert _close(_gram(Z), _gram(pre)) and not Z[:, :, L].any()
    K3 = I.diagonal_loading(K2, load)
    assert np.array_equal(K3, Z[:, :, :L]) and _lower(K3)
    assert _close(_gram(K3), _gram(K2) + load * load * np.eye(L))
    # the extracted state solves K^H R = conj(info)
    R = I.extract_state(K3, info2)
    assert _close(np.einsum("nji,nj->ni", np.conj(K3), R), np.conj(info2))


def test_zero_norm_is_an_arithmetic_error():
    with pytest.raises(ArithmeticError):
        I.givens(np.array([0j, 1 + 0j]), np.array([0j, 0j]))


def _serial_resets(flags, n0=0):
    """cancelVP.cc:550-560 as written: one counter, skips visited in (frame, bin) order -> the 1-based ordinals of the skips that reset, the counter"""
    cnt, ordinal, resets = n0, 0, []
    for frame in flags:
        for skipped in frame:
            if not skipped:
                continue
            ordinal += 1
            if cnt >= 30:
                resets.append(ordinal); cnt = 0
            cnt += 1
    return resets, cnt


def test_skip_counter_is_the_serial_count():
    V, A, _ = N.echo_case(230, 9, 2, seed=21, switch=(0.5, 12.0, 40), quiet=[(30, 37), (150, 151)])
    o = I.InfoAec(I.INFO, 16, 2)
    o.run(V[:120], A[:120]); o.run(V[120:], A[120:], frame0=120)                    # two calls: the counter is carried
    resets, cnt = _serial_resets(o.skip_flags)
    total = int(sum(f.sum() for f in o.skip_flags))
    print("%d skips, %d resets, counter %d" % (total, len(resets), cnt))
    assert total > 100 and o.reset_at == resets and o.skipped == cnt and o.resets == len(resets)
    assert resets == list(range(31, total + 1, 30))                                  # the 31st, 61st, ... skip
    # a reset puts the filter back to (1, 0, ...) and the skipped frame leaves it there
    o2 = I.InfoAec(I.INFO, 16, 2); o2.skipped = 30; o2.R[:] = 0.3
    quiet = np.zeros((1, 9), np.complex64); o2.run(quiet + np.float32(1e-3), A[:1])  # every bin skips: |v0|^2 below the gate
    assert np.array_equal(o2.R[0], [1.0, 0.0]) and np.all(o2.R[1:] == 0.3) and o2.skipped == 9 and o2.resets == 1


def test_starts_from_one_zero_and_the_square_root_kind_ignores_sigmak2():
    V, A, _ = N.echo_case(3, 5, 3, seed=2)
    for kind in (I.INFO, I.SQRT_INFO):
        o = I.InfoAec(kind, 8, 3)
        assert np.array_equal(o.R, np.tile([1.0, 0.0, 0.0], (5, 1)))
        E = o.run(V[:1], A[:1])
        assert np.array_equal(E[0], A[0].astype(np.complex128) - V[0].astype(np.complex128))      # R = (1, 0, 0) at the first frame
    a = I.InfoAec(I.SQRT_INFO, 8, 3, sigmak2=5.0); b = I.InfoAec(I.SQRT_INFO, 8, 3, sigmak2=0.01)
    assert np.array_equal(a.K, np.tile(np.eye(3) / np.sqrt(10e-4), (5, 1, 1)))
    assert np.array_equal(a.run(V, A), b.run(V, A)) and np.array_equal(a.R, b.R)
    # the first update replaces R by the extracted state: nothing of (1, 0, 0) is left in it
    c = I.InfoAec(I.SQRT_INFO, 8, 3); c.run(V[:1], A[:1])
    assert _close(np.einsum("nji,nj->ni", np.conj(c.K), c.R), np.conj(c.info))


def test_amp4play_scales_the_history_and_bins_above_half_are_conjugates():
    V, A, _ = N.echo_case(40, 5, 2, seed=6)
    for kind in (I.INFO, I.SQRT_INFO):
        a = I.InfoAec(kind, 8, 2, amp4play=0.5); b = I.InfoAec(kind, 8, 2)
        Ea = a.run(V, A); Eb = b.run((V * np.float32(0.5)).astype(np.complex64), A)
        assert np.array_equal(Ea, Eb) and np.array_equal(a.hist, b.hist) and np.array_equal(a.hist[:, 0], V[-1].astype(np.complex128) * 0.5)
        X = a.full(Ea)
        assert X.shape == (40, 8) and np.array_equal(X[:, :5], Ea)
        for k in range(1, 4):
            assert np.array_equal(X[:, 8 - k], np.conj(Ea[:, k]))


def test_floor_rule_and_closed_gate():
    V, A, _ = N.echo_case(30, 5, 2, seed=8)
    for kind in (I.INFO, I.SQRT_INFO):
        o = I.InfoAec(kind, 8, 2); o.run(V, A)
        st = [x.copy() for x in (o.R, o.K, o.sv, o.scal)]
        z = np.zeros((1, 5), np.complex64)
        Rh = o.R.copy(); hist1 = o.hist[:, 0].copy()
        with np.errstate(all="ignore"):
            E = o.run(z, z)                                                         # digital silence in both streams: the gate is closed
        for a, b in zip(st, (o.R, o.K, o.sv, o.scal)):
            assert np.array_equal(a, b)
        want = -Rh[:, 1] * hist1                                                    # the residual of the frame: what the older tap still predicts
        if kind == I.INFO:                                                          # |E| < 0.01 leaves as E / |E|; exactly 0 would be NaN
            small = np.abs(want) < I.FLOOR
            assert np.allclose(E[0][~small], want[~small]) and np.allclose(np.abs(E[0][small]), 1.0)
        else:
            assert np.allclose(E[0], want, rtol=1e-14, atol=0.0)                      # no floor
        with np.errstate(all="ignore"):
            E = o.run(np.zeros((2, 5), np.complex64), np.zeros((2, 5), np.complex64))
        assert (np.isnan(E[1]).all() if kind == I.INFO else not E[1].any())         # history all zero now: the residual is exactly 0


def test_first_hundred_frames_and_frame_mode_one():
    V, A, _ = N.echo_case(130, 5, 2, seed=9, near=40.0)                             # loud near end: the post-100-frames gate would close
    for kind in (I.INFO, I.SQRT_INFO):
        a = I.InfoAec(kind, 8, 2); a.run(V, A)
        assert a.decisions["gate"][0] > 0 and sum(a.decisions["gate"]) > 100
        b = I.InfoAec(kind, 8, 2); b.run(V, A, frame_mode=1)                        # the constant -5: smoothing above 1, never a threshold decision
        assert sum(b.decisions["gate"]) == 0
        c = I.InfoAec(kind, 8, 2); c.run(V[:1], A[:1], frame_mode=1)
        E0 = A[0].astype(np.complex128) - V[0].astype(np.complex128)
        sm = 1.0 - float(-5) * (1.0 - 0.9) / 100.0
        assert sm > 1.0 and np.array_equal(c.scal[:, 0], I.abs2(E0) * sm + 0.0 * (1.0 - sm))
    # the sign of sf inside the first 100 frames: exp(-snr) = inf gives -1 (skip), a NaN snr does not skip.  smooth = -1 at frame 50 is a
    # smoothing factor of 0: the preset _snr stays as it is.
    o = I.InfoAec(I.SQRT_INFO, 8, 1, smooth=-1.0); o.scal[:, 2] = [-1e6, np.nan, 0.0, 1.0, 5.0]
    sf = o._update_band(np.arange(5), np.ones(5, complex), np.full(5, 0.5 + 0j), frameX=50)
    assert sf[0] == -1.0 and np.isnan(sf[1]) and sf[2] == 0.0 and np.all(sf[3:] > 0)
    assert list(sf < 0.0) == [True, False, False, False, False]


def test_reset_resets_nothing():
    V, A, _ = N.echo_case(30, 5, 2, seed=10)
    for kind in (I.INFO, I.SQRT_INFO):
        o = I.InfoAec(kind, 8, 2); o.run(V, A); st = [x.copy() for x in (o.R, o.K, o.sv, o.scal, o.hist)]
        o.reset()
        for a, b in zip(st, (o.R, o.K, o.sv, o.scal, o.hist)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("L,mode", [(L, m) for L in (1, 4, 8) for m in (0, 1)])
def test_square_root_kind_cancels_under_near_end_noise(L, mode):
    V, A, g = N.echo_case(400, 5, L, seed=7, near=1.0)
    o = I.InfoAec(I.SQRT_INFO, 8, L); E = o.run(V, A, 0, mode)
    erle = N.erle_db(A.astype(np.complex128), E, last=100); d = np.abs(o.R - g).max() / np.abs(g).max()
    print("L=%d mode=%d ERLE %.1f dB, max|R-g| / max|g| %.3f" % (L, mode, erle, d))
    assert erle >= 15.0 and d <= 0.15


@pytest.mark.parametrize("M,L,mode,seed", I.INFO_CASES)
def test_gpu_cases_are_admissible_and_the_inversion_routes_agree(M, L, mode, seed):
    """every decision margin of both kinds >= 1e-6, each side of the post-100-frames gate >= 10 % of the decisions; the plain kind's three
    inversion routes within 1e-10 of the largest output and filter entry (measured <= 2.2e-13)"""
    V, A, nf = I.info_inputs(M, L, seed)
    for kind in (I.INFO, I.SQRT_INFO):
        _, _, _, E, objs = I.reference(kind, M, L, mode, seed)
        assert np.isfinite(E).all()
        margin = min(min(o.margin.values()) for o in objs)
        no, yes = sum(o.decisions["gate"][0] for o in objs), sum(o.decisions["gate"][1] for o in objs)
        print("kind %d M=%d L=%d mode=%d: margin %.2e, gate %d no / %d yes, resets %d, cond %.1e" %
              (kind, M, L, mode, margin, no, yes, sum(o.resets for o in objs), max(o.cond for o in objs)))
        assert margin >= 1e-6
        if mode == 1:
            assert no + yes == 0
        else:
            assert no >= 0.1 * (no + yes) and yes >= 0.1 * (no + yes)
    _, _, _, E, objs = I.reference(I.INFO, M, L, mode, seed)
    R = I.state(objs, 3, "R")
    for route in ("inv", "chol"):
        E2, objs2 = I.run_batch(I.INFO, M, L, V, A, nf, 0, mode, route=route)
        eo = np.abs(E2 - E).max() / np.abs(E).max(); er = np.abs(I.state(objs2, 3, "R") - R).max() / np.abs(R).max()
        print("route %s: out %.2e, filter %.2e" % (route, eo, er))
        assert eo <= 1e-10 and er <= 1e-10
        assert [o.resets for o in objs2] == [o.resets for o in objs] and [o.skipped for o in objs2] == [o.skipped for o in objs]


def test_abi_host_side(dsr):
    L = dsr.load()
    for name in ("dsr_aec_create_info", "dsr_aec_set_info"):
        assert hasattr(L, name)
    h = C.c_void_p()
    for sq in (0, 1):
        for M, n in [(255, 1), (0, 1), (-4, 1), (256, 0), (256, 33), (256, -1)]:
            assert L.dsr_aec_create_info(sq, M, n, C.byref(h)) == 13, (sq, M, n)     # DSR_E_PARAMETER
        assert b"sampleN" in L.dsr_last_error()
    for kind in (4, 5, 7, 8, 9, -1):
        assert L.dsr_aec_create(kind, 256, 1, C.byref(h)) == 13, kind                # the new kinds come from dsr_aec_create_info only
    sizes = {}
    for sq, kind in ((0, 8), (1, 9)):
        dsr.check(L.dsr_aec_create_info(sq, 96, 32, C.byref(h)))
        assert (L.dsr_aec_kind(h), L.dsr_aec_fft_len(h), L.dsr_aec_sample_n(h)) == (kind, 96, 32)
        b = [L.dsr_aec_state_bytes(h, U) for U in (0, 1, 2, 3)]
        assert b[0] == 0 and 0 < b[1] < b[2] < b[3] and b[2] - b[1] == b[3] - b[2]
        F, n = 49, 32
        assert b[1] >= F * (16 * n + 16 * n * n + 8 + 16 * n + 24 + (16 * n if sq else 0))      # R, K, sigma2_v, history, the per-bin scalars, the information state
        sizes[kind] = b[1]
        assert L.dsr_aec_set_info(h, 2.0, 100.0, 0.9, 1e-2) == 0 and L.dsr_aec_set_block(h, 0.95, 1e-3, 5.0, 100.0, 1.0) == 0
        assert L.dsr_aec_set_block(h, 0.0, 1e-3, 5.0, 100.0, 1.0) == 13
        assert L.dsr_aec_set_frame_mode(h, 1) == 0 and L.dsr_aec_set_frame_mode(h, 2) == 13
        assert L.dsr_aec_set_nlms(h, 1.0, 1.0, 1.0) == 13 and L.dsr_aec_set_kalman(h, 0.9, 1.0, 1.0) == 13 and L.dsr_aec_set_dtd(h, 2.0, 100.0, 0.9) == 13
        L.dsr_aec_destroy(h)
    assert sizes[9] > sizes[8]
    dsr.check(L.dsr_aec_create(2, 64, 4, C.byref(h)))
    assert L.dsr_aec_set_info(h, 2.0, 100.0, 0.9, 1e-2) == 13                        # not an information filter
    L.dsr_aec_destroy(h)
    a = dsr.Aec("sqrtinfo", 64, 4, loading=0.02); b = dsr.Aec("info", 64, 4)
    assert (a.kind, b.kind) == (9, 8) and a.stateBytes(2) > b.stateBytes(2) > dsr.Aec("block", 64, 4).stateBytes(2)
    with pytest.raises(dsr.DsrError) as e:
        dsr.Aec("info", 64, 33)
    assert e.value.status == 13
    from dsr.btk import cancelVP
    assert issubclass(cancelVP.SquareRootInformationFilterEchoCancellationFeaturePtr, cancelVP.InformationFilterEchoCancellationFeaturePtr)
    assert issubclass(cancelVP.InformationFilterEchoCancellationFeaturePtr, cancelVP.BlockKalmanFilterEchoCancellationFeaturePtr)
