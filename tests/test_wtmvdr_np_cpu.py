"""WarpedTwiceMVDRFeature / SpectralSmoothing without a GPU: the restatement against itself and the C oracle, and the host side of the library."""
import ctypes as C

import numpy as np
import pytest

from tests import wtmvdr_cases as Cs
from tests import wtmvdr_np as W

ALL = range(len(Cs.CASES))


@pytest.mark.parametrize("ci", ALL)
def test_loop_orders_bit_equal(ci):
    """The interchanged loop nests of the device kernels (samples outermost in the autocorrelation, stages outermost in the chain) keep every
    operation's operands and every accumulator's order of addends: R and PA are those of the reference's order to the last bit."""
    for a, b in zip(Cs.restated(ci, True), Cs.restated(ci, False)):
        assert np.array_equal(a["R"].view(np.uint32), b["R"].view(np.uint32))
        assert np.array_equal(a["PA"].view(np.uint32), b["PA"].view(np.uint32))
        assert a["PA"].shape == (Cs.CASES[ci][0] + 1,) and a["PA"][-1] == 0         # xm[dim] is never written


def test_degenerate_case_against_oracle(oracle):
    """warp 0, fixed mode, sensibility 0: rewarp is 0, the compensation the identity and the chain a pure delay, so the envelope is WarpMVDR's
    (the C oracle's lpc_feature, method 0, kind 0) up to the float (here) versus double (there) accumulation of PC.
    Measured against the C oracle on the case's 11 frames: 3.87e-05 relative at the worst element (a sharp resonance: 3.4e+08 over 5.8e+05
    within the frame; 1.6e-06 on the next worst but one); asserted: ten times that.  That the accumulation is all there is to it shows in the
    second half: with PC accumulated in double as MVDRFeature does (lpc.h:153-156) the restatement equals the oracle bit for bit."""
    dim, order = Cs.CASES[Cs.DEGENERATE][:2]
    fr = np.array(Cs.frames(Cs.DEGENERATE))
    rs = Cs.restated(Cs.DEGENERATE)
    assert all(r["rewarp"] == 0 for r in rs)
    got = np.stack([r["out"] for r in rs])
    want = oracle.lpc_feature(fr, order, 0.0, 0, 0)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    nz = fin & (want != 0)                                              # the all-zero frame: E[0] = 0 over a finite power
    assert np.array_equal(got[fin & ~nz], want[fin & ~nz])
    rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    print("degenerate case against the oracle: worst relative difference %.3e over %d elements" % (rel.max(), rel.size))
    assert rel.max() <= 10 * 3.87e-05
    for t, x in enumerate(fr):
        with np.errstate(all="ignore"):
            X = [np.float32(v) for v in x]
            LP, E0 = W.compensate_levinson(W.autocorr_streamed(X, order, 0.0), order, 0.0, np.float32(0.0))
            V = []
            for i in range(order + 1):
                acc = np.float64(0.0)
                for ii in range(order - i + 1):
                    acc = acc + np.float64(np.float32(order + 1 - i - 2 * ii) * LP[ii] * LP[ii + i])
                V.append(np.float32(-acc) if E0 > 0 else np.float32(10000000))
            PA = W.chain_staged([V[abs(w - order)] for w in range(2 * order + 1)], dim, np.float32(-0.0))
            assert np.array_equal(W.envelope(PA, E0, dim), want[t], equal_nan=True), t


@pytest.mark.parametrize("ci", ALL)
def test_cases_are_well_conditioned(ci):
    """The transform recomputed as a direct DFT in long double agrees with np.fft's within 2^-23 relative: the GPU test's tolerance hides no
    ill-conditioned input (a power whose float rounding flips is one float ulp, halved by the square root)."""
    dim = Cs.CASES[ci][0]; nd = 0
    for r in Cs.restated(ci):
        with np.errstate(all="ignore"):
            o2 = W.envelope_longdouble(list(r["PA"]), r["E0"], dim)
        fin = np.isfinite(r["out"])
        assert np.array_equal(fin, np.isfinite(o2))
        assert np.all(np.abs(r["out"][fin] - o2[fin]) <= 2.0 ** -23 * np.abs(o2[fin]))
        assert np.array_equal(r["out"][~fin], o2[~fin], equal_nan=True)
        nd += int((r["out"][fin] != o2[fin]).sum())
    print("case %d: %d elements differ" % (ci, nd))


def test_spectral_smoothing_restatement_edges():
    """size 2..4 leave R all zero (mult 0); an adjustTo below 0.01 takes the 100 * maxFFT branch"""
    for size in (2, 3, 4):
        assert np.array_equal(W.spectral_smoothing(np.ones(size), np.ones(size)), np.zeros(size))
    frm = np.arange(1.0, 8.0); to = np.full(7, 0.001)
    out = W.spectral_smoothing(to, frm)
    r4 = np.float32(3.0 / 9.0 + 2.0 * 4.0 / 9.0 + 5.0 / 3.0 + 2.0 * 6.0 / 9.0 + 7.0 / 9.0)     # i = 4 is the largest smoothed value
    assert np.array_equal(out, np.float64(np.float32(100) * r4) * to)


# ------------------------------------------------------------------------------------------------------------------ the host side
def test_symbols_and_classes(dsr):
    L = dsr.load()
    for name in ("dsr_wtmvdr_create", "dsr_wtmvdr_destroy", "dsr_wtmvdr_size", "dsr_wtmvdr_run", "dsr_wtmvdr_feature_create", "dsr_specsmooth_run",
                 "dsr_spectral_smoothing_create"):
        assert hasattr(L, name), name
    assert len(L.dsr_wtmvdr_run.argtypes) == 8 and len(L.dsr_specsmooth_run.argtypes) == 6
    from dsr.btk import feature as F
    assert issubclass(F.WarpedTwiceMVDRFeaturePtr, F.FeatureStreamPtr) and issubclass(F.SpectralSmoothingPtr, F.FeatureStreamPtr)
    assert callable(dsr.WtMvdrEnvelope) and callable(dsr.spectral_smoothing)


def _create(L, *a):
    h = C.c_void_p()
    st = L.dsr_wtmvdr_create(*a, C.byref(h))
    return st, (L.dsr_last_error() or b"").decode()


def test_create_errors(dsr):
    L = dsr.load()
    st, msg = _create(L, 64, 33, 0, 0.3, 0, 0.1)                        # lpc.cc:349-350
    assert st == dsr.E_PARAMETER and msg == "Order (33) and dimension (33) do not match."
    st, msg = _create(L, 64, 8, 65, 0.3, 0, 0.1)                        # R1R0 would read past the frame
    assert st == dsr.E_PARAMETER and "correlate" in msg
    st, _ = _create(L, 64, 33, 9, 0.3, 0, 0.1)                          # correlate < 10 means dim: the order is what is wrong
    assert st == dsr.E_PARAMETER
    assert L.dsr_specsmooth_run(None, None, 1, 1, None, None) == dsr.E_PARAMETER      # size()-2 wraps around below 2
    assert L.dsr_wtmvdr_size(None) == 0


def _source(L, typ, size):
    h = C.c_void_p()
    dsr_check = L.dsr_frame_source_create(typ, size, b"src", C.byref(h))
    assert dsr_check == 0
    return h


def test_stream_create_errors(dsr):
    L = dsr.load()
    a, b, f = _source(L, 3, 5), _source(L, 3, 6), _source(L, 2, 64)
    try:
        out = C.c_void_p()
        assert L.dsr_spectral_smoothing_create(a, b, b"", C.byref(out)) == dsr.E_DIMENSION        # lpc.cc:476-477
        assert (L.dsr_last_error() or b"").decode() == "Feature sizes (5 vs. 6) do not match."
        assert L.dsr_wtmvdr_feature_create(f, 33, 0, 0.3, 0, 0.1, b"", C.byref(out)) == dsr.E_PARAMETER
        assert not out.value
    finally:
        for h in (a, b, f):
            L.dsr_stream_release(h)
