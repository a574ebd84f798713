"""CPU tests of the echo cancellers: the numpy restatement tests/aec_np.py against independent forms of the same recursions, that it cancels
an echo, that the DTD inputs of the GPU comparison are admissible (no gate decision near its threshold), and the host-side C-ABI
(dsr_aec_create / setters / state_bytes / errors) without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import aec_np as N


def test_block_with_one_tap_is_the_scalar_kalman():
    V, A, _ = N.echo_case(200, 9, 1, seed=3, quiet=[(50, 60)])
    b = N.Aec(N.BLOCK, 16, 1, sigmau2=0.7, sigmak2=0.7); k = N.Aec(N.KALMAN, 16, sigma2=0.7)
    Eb, Ek = b.run(V, A), k.run(V, A)
    assert np.abs(Eb - Ek).max() <= 1e-12 * np.abs(Ek).max()
    assert np.abs(b.R - k.R).max() <= 1e-12 * np.abs(k.R).max()
    assert np.abs(b.K - k.K).max() <= 1e-12 * np.abs(k.K).max() and np.abs(b.sv - k.sv).max() <= 1e-12 * k.sv.max()


def test_nlms_step_closed_formula():
    V = np.array([[12 + 5j]], np.complex64); A = np.array([[3 - 4j]], np.complex64)
    o = N.Aec(N.NLMS, 0, delta=50.0, epsilon=0.01, threshold=100.0); o.R[0, 0] = 0.2 - 0.1j
    E = o.run(V, A)
    R0 = 0.2 - 0.1j; v, a = complex(V[0, 0]), complex(A[0, 0])
    assert abs(E[0, 0] - (a - R0 * v)) < 1e-15
    want = R0 - (R0 - a / v) * 0.01 * abs(v) ** 2 / (50.0 + abs(a) ** 2)
    assert abs(o.R[0, 0] - want) < 1e-15


@pytest.mark.parametrize("kind", [N.NLMS, N.KALMAN, N.BLOCK])
def test_gated_frame_leaves_the_state_bit_identical(kind):
    V, A, _ = N.echo_case(40, 5, 3, seed=5)
    o = N.Aec(kind, 8, 3); o.run(V[:30], A[:30])
    st = [o.R.copy(), o.K.copy(), o.sv.copy()]
    quiet = (V[30:31] * np.float32(1e-3)).astype(np.complex64)                     # |V|^2 far below the threshold of 100
    o.run(quiet, A[30:31])
    for a, b in zip(st, [o.R, o.K, o.sv]):
        assert np.array_equal(a.view(np.float64), b.view(np.float64))
    if kind == N.BLOCK:                                                            # the history still advances
        assert np.array_equal(o.hist[:, 0], quiet[0].astype(np.complex128))


def test_amp4play_scales_the_history_not_the_recorded_stream():
    V, A, _ = N.echo_case(60, 5, 2, seed=6)
    a = N.Aec(N.BLOCK, 8, 2, amp4play=0.5); b = N.Aec(N.BLOCK, 8, 2, threshold=100.0)
    Ea = a.run(V, A); Eb = b.run((V * np.float32(0.5)).astype(np.complex64), A)     # halving is exact in fp32
    assert np.array_equal(Ea, Eb) and np.array_equal(a.hist, b.hist)
    assert np.array_equal(a.hist[:, 0], V[-1].astype(np.complex128) * 0.5)
    assert np.array_equal(Ea[0], A[0].astype(np.complex128))                       # R = 0 at the first frame: the recorded frame itself, unscaled


def test_bins_above_half_are_conjugates():
    V, A, _ = N.echo_case(10, 9, 1, seed=7)
    o = N.Aec(N.KALMAN, 16); E = o.run(V, A); X = o.full(E)
    assert X.shape == (10, 16) and np.array_equal(X[:, :9], E)
    for k in range(1, 8):
        assert np.array_equal(X[:, 16 - k], np.conj(E[:, k]))


@pytest.mark.parametrize("L", [1, 4, 16, 32])
def test_it_cancels(L):
    V, A, g = N.echo_case(600, 9, L, seed=40 + L)
    o = N.Aec(N.BLOCK, 16, L); E = o.run(V, A)
    erle = N.erle_db(A, E)
    print("L=%d ERLE %.1f dB, max|R-g| %.3f" % (L, erle, np.abs(o.R - g).max()))
    assert erle >= 15.0


@pytest.mark.parametrize("M,L,mode,seed", N.DTD_CASES)
def test_dtd_inputs_are_admissible(M, L, mode, seed):
    V, A, nf = N.dtd_inputs(M, L, seed)
    E, objs = N.run_batch(lambda: N.Aec(N.DTD, M, L), V, A, nf, 0, mode)
    assert np.isfinite(E).all()
    skip, adapt = sum(o.decisions[0] for o in objs), sum(o.decisions[1] for o in objs)
    margin = min(o.margin for o in objs)
    print("M=%d L=%d mode=%d: margin %.2e, %d skip / %d adapt" % (M, L, mode, margin, skip, adapt))
    if mode == 1:
        assert skip + adapt == 0                   # the constant -5 never leaves the first-100-frames branch: no threshold decision to get wrong
        return
    assert margin >= 1e-6
    assert skip >= 0.1 * (skip + adapt) and adapt >= 0.1 * (skip + adapt)


def test_abi_host_side(dsr):
    L = dsr.load()
    h = C.c_void_p()
    for kind, M, n in [(0, 255, 1), (0, 0, 1), (1, -4, 1), (2, 256, 0), (2, 256, 33), (3, 256, -1), (4, 256, 1), (-1, 256, 1)]:
        assert L.dsr_aec_create(kind, M, n, C.byref(h)) == 13, (kind, M, n)        # DSR_E_PARAMETER
    assert b"sampleN" in L.dsr_last_error() or b"kind" in L.dsr_last_error()
    dsr.check(L.dsr_aec_create(2, 96, 32, C.byref(h)))                              # no power of two needed
    assert (L.dsr_aec_kind(h), L.dsr_aec_fft_len(h), L.dsr_aec_sample_n(h)) == (2, 96, 32)
    F, n = 49, 32
    assert L.dsr_aec_state_bytes(h, 3) == 3 * F * (16 * n + 16 * n * n + 8 + 16 * n) + 3 * 32
    assert L.dsr_aec_state_bytes(h, 0) == 0
    assert L.dsr_aec_set_block(h, 0.95, 1e-3, 5.0, 100.0, 1.0) == 0
    for beta in (0.0, -0.1, 1.5, float("nan")):
        assert L.dsr_aec_set_block(h, beta, 1e-3, 5.0, 100.0, 1.0) == 13
    assert L.dsr_aec_set_block(h, 1.0, 1e-3, 5.0, 100.0, 1.0) == 0
    assert L.dsr_aec_set_nlms(h, 1.0, 1.0, 1.0) == 13 and L.dsr_aec_set_kalman(h, 0.9, 1.0, 1.0) == 13 and L.dsr_aec_set_dtd(h, 2.0, 100.0, 0.9) == 13
    L.dsr_aec_destroy(h)
    dsr.check(L.dsr_aec_create(1, 64, 7, C.byref(h)))                               # NLMS / Kalman have one tap whatever sampleN says
    assert L.dsr_aec_sample_n(h) == 1 and L.dsr_aec_set_kalman(h, 0.0, 5.0, 100.0) == 13 and L.dsr_aec_set_kalman(h, 0.5, 5.0, 100.0) == 0
    L.dsr_aec_destroy(h)
    dsr.check(L.dsr_aec_create(3, 64, 4, C.byref(h)))
    assert L.dsr_aec_set_dtd(h, 2.0, 100.0, 0.9) == 0 and L.dsr_aec_set_frame_mode(h, 1) == 0 and L.dsr_aec_set_frame_mode(h, 2) == 13
    buf = np.zeros(8)
    assert L.dsr_aec_state_read(h, None, 1, 0, buf.ctypes.data_as(C.c_void_p), 8) == 13
    L.dsr_aec_destroy(h)
    a = dsr.Aec("dtd", 64, 4)
    assert a.stateBytes(2) == 2 * 33 * (64 + 256 + 8 + 64) + 64
    with pytest.raises(dsr.DsrError) as e:
        dsr.Aec("block", 64, 33)
    assert e.value.status == 13
    from dsr.btk import cancelVP
    for name in ("NLMSAcousticEchoCancellationFeaturePtr", "KalmanFilterEchoCancellationFeaturePtr", "BlockKalmanFilterEchoCancellationFeaturePtr",
                 "DTDBlockKalmanFilterEchoCancellationFeaturePtr"):
        assert hasattr(cancelVP, name)
