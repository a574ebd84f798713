"""CPU tests of the numpy restatement that tests/test_gpu_conv.py checks the device against (tests/conv_np.py, tests/conv_cases.py): the two
flavours of OverlapAdd agree, the bit-count condition can see a wrong fold, OverlapSave is the matching slice of the linear convolution, and
FilterFeature delivers the reference's frame counts.  None of them runs the library: they pass with and without the feature."""
import numpy as np
import pytest

from tests import conv_cases as Cs
from tests import conv_np as R


def _xnorm(x):
    return float(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).max())


def _chain_bound(x, h, L):
    """what the fp32 roundings of a sample's chain can add up to: one rounding, 2^-24 of the partial sum, for each of its at most
    ceil((P-1)/L)+1 adds, and no partial sum of a convolution exceeds max|x| sum|h|"""
    depth = -(-(h.size - 1) // L) + 1
    return depth * 2.0 ** -24 * float(np.abs(x).max()) * float(np.abs(h).sum()) * (1 + 2.0 ** -20)


@pytest.mark.parametrize("k", sorted(Cs.ADD))
def test_overlap_add_flavours_agree(k):
    L, P, fftLen, T, C = Cs.ADD[k]
    x, h, N, y, buf = Cs.add_case(k)
    assert N == {1: 8, 2: 16, 3: 512, 4: 512, 5: 4096, 6: 8192, 7: 16384, 8: 16}[k] and y.shape == (C, T, L) and buf.shape == (C, L + P - 1)
    for c in range(C):
        yf, bf = R.overlap_add(x, h[c], fftLen, "fft")
        tol = R.tolerance(y[c], N, _xnorm(x), np.linalg.norm(h[c]))
        assert (np.abs(yf.astype(np.float64) - y[c]) <= tol).all()
        assert Cs.differing(yf, y[c]) <= 1 + y[c].size // 1000
        assert np.all(buf[c][P - 1:] == 0.0)                            # the top L entries are zeroed after every block
    if k in (1, 3, 5, 6, 7):
        yf = np.stack([R.overlap_add(x, h[c], fftLen, "fft")[0] for c in range(C)])
        assert Cs.differing(yf, y) == 0


def test_overlap_add_is_the_linear_convolution():
    L, P, fftLen, T, C = Cs.ADD[3]
    x, h, N, y, buf = Cs.add_case(3)
    full = np.convolve(x.reshape(-1).astype(np.float64), h[1])
    tol = _chain_bound(x, h[1], L)
    assert (np.abs(y[1].reshape(-1) - full[:T * L]) <= tol).all()
    assert (np.abs(buf[1][:P - 1] - full[T * L:T * L + P - 1]) <= tol).all()


def test_overlap_add_buffer_carries_over():
    L, P, fftLen, T, C = Cs.ADD[5]
    x, h, N, y, buf = Cs.add_case(5)
    y1, b1 = R.overlap_add(x[:7], h[0])
    y2, b2 = R.overlap_add(x[7:], h[0], buffer=b1)
    assert Cs.differing(np.concatenate([y1, y2]), y[0]) == 0 and Cs.differing(b2, buf[0]) == 0


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("how", ["once", "newest"])
def test_a_wrong_fold_is_seen(k, how):
    """summing a sample's contributions in fp64 and rounding once, or taking the newest block first, changes more than a tenth of the elements:
    the cap of 1 + size/1000 differing elements in the GPU test cannot miss either"""
    L, P, fftLen, T, C = Cs.ADD[k]
    x, h, N, y, buf = Cs.add_case(k)
    sec = R.sections_ld(x, h[0])
    wrong = R.ola_fold_wrong(sec, L, P, how)
    assert Cs.differing(wrong, y[0]) > y[0].size // 10
    assert (np.abs(wrong.astype(np.float64) - y[0]) <= 2 * _chain_bound(x, h[0], L)).all()   # wrong in the last bits only: a loose tolerance alone would not do


def test_unit_impulse_reproduces_the_response():
    L, P, fftLen, T, C = Cs.ADD[3]
    x, h, N, y, buf = Cs.add_case(3)
    imp = np.zeros((T, L), np.float32); imp[0, 0] = 1.0
    yi, _ = R.overlap_add(imp, h[0])
    nb = -(-P // L)
    got = yi[:nb].reshape(-1)[:P]
    assert np.array_equal(got, h[0].astype(np.float32)) and not yi[nb:].any()


@pytest.mark.parametrize("k", sorted(Cs.SAVE))
def test_overlap_save_is_a_slice_of_the_linear_convolution(k):
    L, P, T, C = Cs.SAVE[k]
    x, h, y = Cs.save_case(k)
    assert y.shape == (C, T, L - P)
    for c in range(C):
        tol = R.tolerance(y[c], L, _xnorm(x), np.linalg.norm(h[c]))
        for t in range(T):
            lin = np.convolve(x[t].astype(np.float64), h[c])
            assert (np.abs(y[c, t] - lin[P:L]) <= tol[t]).all()                        # from P: the valid sample P-1 is dropped, as in the reference
        yf = R.overlap_save(x, h[c], "fft")
        assert (np.abs(yf.astype(np.float64) - y[c]) <= tol).all() and Cs.differing(yf, y[c]) <= 1 + y[c].size // 1000


def test_overlap_save_update_flavours_agree():
    L, P, T, C = Cs.SAVE[2]
    x, h, y = Cs.save_case(2)
    rng = np.random.default_rng(7)
    delta = 0.1 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    a = R.overlap_save(x, h[0], "ld", delta); b = R.overlap_save(x, h[0], "fft", delta)
    tol = R.tolerance(a, L, _xnorm(x), np.linalg.norm(R.save_response(h[0], L, delta)))
    assert (np.abs(a.astype(np.float64) - b) <= tol).all() and Cs.differing(a, b) <= 1 + a.size // 1000
    assert Cs.differing(a, y[0]) > a.size // 2                                          # the update matters


def test_refusals_of_the_restatement():
    with pytest.raises(ValueError):
        R.fft_len(64, 3, 64)
    with pytest.raises(ValueError):
        R.overlap_save(np.zeros((1, 8), np.float32), np.ones(8))
    with pytest.raises(ValueError):
        R.filter_feature(np.zeros((4, 2), np.float32), np.ones(4))


@pytest.mark.parametrize("k", sorted(Cs.FIR))
def test_filter_feature_frame_counts(k):
    dim, lenA, T = Cs.FIR[k]
    o = (lenA - 1) // 2
    for kind in ("delta", "random"):
        x, a, y = Cs.fir_case(k, kind)
        want = {1: 1, 2: 40, 3: 4, 4: 0, 5: 7, 6: 33}[k]
        assert y.shape == (want, dim) and R.fir_count(T, lenA) == want
        if lenA == 1:
            assert not y[-1].any() and np.array_equal(y[:-1], (a[0] * x.astype(np.float64)).astype(np.float32))
        elif want:
            full = np.stack([np.convolve(x[:, c].astype(np.float64), a) for c in range(dim)], axis=1)[o:o + T]
            assert np.abs(y - full).max() <= 2.0 ** -22 * np.abs(full).max() + 1e-30


def test_regression_delta_of_a_ramp_is_its_slope():
    x = (2.5 * np.arange(20, dtype=np.float64))[:, None].astype(np.float32)
    y = R.filter_feature(x, R.regression_delta(2))
    assert np.allclose(y[2:-2, 0], 2.5)


def test_merge_feature_concatenates():
    a = np.arange(6, dtype=np.float32).reshape(3, 2); b = a + 10; c = (a + 20)[:2]
    m = R.merge_feature(a, b, c)
    assert m.shape == (2, 6) and np.array_equal(m[1], [2, 3, 12, 13, 22, 23])
