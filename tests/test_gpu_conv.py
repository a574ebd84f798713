"""GPU tests of the block convolution (OverlapAdd, OverlapSave: include/dsr.h section 2g, csrc/k_conv.hip) and of FilterFeature / MergeFeature
against the numpy restatement of tests/conv_np.py on the cases of tests/conv_cases.py.

Every element must lie within 2^-23 |ref| + 2^-44 log2(N) |x_block| |h| of the longdouble-section restatement (one fp32 rounding plus a
~500-fold margin over the fp64 radix-2 error bound), and at most 1 + size/1000 elements may differ from it in bits: tests/test_conv_np_cpu.py
shows that a fold in the wrong order differs in more than a tenth of them."""
import numpy as np
import pytest

from tests import conv_cases as Cs
from tests import conv_np as R

pytestmark = pytest.mark.gpu


class Frames:
    """a Python iterable with size()/reset(), as PyVectorFloatFeatureStreamPtr takes it"""

    def __init__(self, a): self.a = a
    def size(self): return self.a.shape[1]
    def reset(self): pass
    def __iter__(self): return iter(self.a)


def _xnorm(x):
    return float(np.sqrt((x.astype(np.float64) ** 2).sum(axis=-1)).max())


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(cuda)                 # a copy: the shared cases are read-only


def _check(tag, got, ref, N, xnorm, hnorm):
    """the tolerance and the cap on elements that differ in bits, for one channel; prints the figures before it asserts"""
    tol = R.tolerance(ref, N, xnorm, hnorm)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ratio = float((err / tol).max()) if ref.size else 0.0
    nd = Cs.differing(got, ref)
    print("%s: %d of %d elements differ in bits, largest error / tolerance %.3g" % (tag, nd, ref.size, ratio))
    assert got.shape == ref.shape
    assert (err <= tol).all(), (tag, ratio)
    assert nd <= 1 + ref.size // 1000, (tag, nd)


@pytest.mark.parametrize("k", sorted(Cs.ADD))
def test_overlap_add_matches_the_restatement(dsr, cuda, k):
    L, P, fftLen, T, C = Cs.ADD[k]
    x, h, N, y, buf = Cs.add_case(k)
    cv = dsr.BlockConvolver("add", L, h, fftLen)
    assert cv.fftLen == max(N, 4) and cv.size == L and (cv.C, cv.P) == (C, P)
    st = cv.state(1, cuda)
    got = cv.apply(_dev(x[None], cuda), st).cpu().numpy()[0]
    for c in range(C):
        _check("add %d ch %d" % (k, c), got[c], y[c], N, _xnorm(x), np.linalg.norm(h[c]))
    if P > 1:
        s = st.cpu().numpy().reshape(C, P - 1)
        for c in range(C):
            _check("add %d ch %d state" % (k, c), s[c], buf[c][:P - 1], N, _xnorm(x), np.linalg.norm(h[c]))


def test_overlap_add_ragged_batch(dsr, cuda):
    L, P, fftLen, T, C = Cs.ADD[3]
    x, h, N, y, buf = Cs.add_case(3)
    x1 = Cs.signal(901, T, L)
    nf = np.array([9, 4], np.int32)
    cv = dsr.BlockConvolver("add", L, h)
    st = cv.state(2, cuda)
    got = cv.apply(_dev(np.stack([x, x1]), cuda), st, _dev(nf, cuda)).cpu().numpy()
    s = st.cpu().numpy().reshape(2, C, P - 1)
    for c in range(C):
        _check("ragged u0 ch %d" % c, got[0, c], y[c], N, _xnorm(x), np.linalg.norm(h[c]))
        y1, b1 = R.overlap_add(x1[:4], h[c])
        _check("ragged u1 ch %d" % c, got[1, c, :4], y1, N, _xnorm(x1[:4]), np.linalg.norm(h[c]))
        _check("ragged u1 ch %d state" % c, s[1, c], b1[:P - 1], N, _xnorm(x1[:4]), np.linalg.norm(h[c]))
        assert not got[1, c, 4:].any()


def test_zero_response_and_unit_impulse(dsr, cuda):
    L, P, fftLen, T, C = Cs.ADD[3]
    x, h, N, y, buf = Cs.add_case(3)
    z = dsr.BlockConvolver("add", L, np.zeros((1, P)))
    st = z.state(1, cuda)
    got = z.apply(_dev(x[None], cuda), st).cpu().numpy()
    assert Cs.differing(got, np.zeros_like(got)) == 0 and Cs.differing(st.cpu().numpy(), np.zeros(P - 1, np.float32)) == 0
    imp = np.zeros((1, T, L), np.float32); imp[0, 0, 0] = 1.0
    cv = dsr.BlockConvolver("add", L, h)
    gi = cv.apply(_dev(imp, cuda)).cpu().numpy()[0]
    for c in range(C):
        flat = gi[c].reshape(-1)
        _check("impulse ch %d" % c, flat[:P], h[c].astype(np.float32), N, 1.0, np.linalg.norm(h[c]))
        assert np.abs(flat[P:]).max() <= 2.0 ** -44 * np.log2(N) * np.linalg.norm(h[c])      # past the response: the transforms' residue, no more


@pytest.mark.parametrize("k", sorted(Cs.SAVE))
def test_overlap_save_matches_the_restatement(dsr, cuda, k):
    L, P, T, C = Cs.SAVE[k]
    x, h, y = Cs.save_case(k)
    cv = dsr.BlockConvolver("save", L, h)
    assert cv.fftLen == L and cv.size == L - P
    got = cv.apply(_dev(x[None], cuda)).cpu().numpy()[0]
    for c in range(C):
        _check("save %d ch %d" % (k, c), got[c], y[c], L, _xnorm(x), np.linalg.norm(h[c]))


def test_overlap_save_update(dsr, cuda):
    L, P, T, C = Cs.SAVE[2]
    x, h, y = Cs.save_case(2)
    cv = dsr.BlockConvolver("save", L, h)
    rng = np.random.default_rng(7)
    delta = 0.1 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    cv.update(delta, c=1)
    got = cv.apply(_dev(x[None], cuda)).cpu().numpy()[0]
    _check("update ch 0 (untouched)", got[0], y[0], L, _xnorm(x), np.linalg.norm(h[0]))
    ref = R.overlap_save(x, h[1], "ld", delta)
    _check("update ch 1", got[1], ref, L, _xnorm(x), np.linalg.norm(R.save_response(h[1], L, delta)))
    assert Cs.differing(ref, y[1]) > ref.size // 2


@pytest.mark.parametrize("k", [3, 5])
def test_two_calls_equal_one_call_bit_for_bit(dsr, cuda, k):
    L, P, fftLen, T, C = Cs.ADD[k]
    x, h, N, y, buf = Cs.add_case(k)
    xs = np.stack([x, Cs.signal(910 + k, T, L)])
    cut = [4, 7]
    cv = dsr.BlockConvolver("add", L, h)
    s1 = cv.state(2, cuda)
    one = cv.apply(_dev(xs, cuda), s1).cpu().numpy()
    a = np.zeros((2, max(cut), L), np.float32); b = np.zeros((2, T - min(cut), L), np.float32)
    for u in range(2):
        a[u, :cut[u]] = xs[u, :cut[u]]; b[u, :T - cut[u]] = xs[u, cut[u]:]
    s2 = cv.state(2, cuda)
    ya = cv.apply(_dev(a, cuda), s2, _dev(np.array(cut, np.int32), cuda)).cpu().numpy()
    yb = cv.apply(_dev(b, cuda), s2, _dev(np.array([T - c for c in cut], np.int32), cuda)).cpu().numpy()
    for u in range(2):
        two = np.concatenate([ya[u][:, :cut[u]], yb[u][:, :T - cut[u]]], axis=1)
        assert Cs.differing(two, one[u]) == 0
        assert not ya[u][:, cut[u]:].any() and not yb[u][:, T - cut[u]:].any()
    assert Cs.differing(s1.cpu().numpy(), s2.cpu().numpy()) == 0


def test_frames_past_nframes_leave_the_state_alone(dsr, cuda):
    L, P, fftLen, T, C = Cs.ADD[3]
    x, h, N, y, buf = Cs.add_case(3)
    cv = dsr.BlockConvolver("add", L, h)
    st = cv.state(1, cuda)
    cv.apply(_dev(x[None, :5], cuda), st)
    before = st.cpu().numpy().copy()
    assert before.any()
    got = cv.apply(_dev(x[None, 5:], cuda), st, _dev(np.array([0], np.int32), cuda)).cpu().numpy()
    assert not got.any() and Cs.differing(st.cpu().numpy(), before) == 0


def test_channels_are_independent(dsr, cuda):
    L, P, fftLen, T, C = Cs.ADD[3]
    x, h, N, y, buf = Cs.add_case(3)
    xd = _dev(x[None], cuda)
    all3 = dsr.BlockConvolver("add", L, h).apply(xd).cpu().numpy()[0]
    for c in range(C):
        one = dsr.BlockConvolver("add", L, h[c]).apply(xd).cpu().numpy()[0, 0]
        assert Cs.differing(one, all3[c]) == 0


@pytest.mark.parametrize("kind", ["delta", "random"])
@pytest.mark.parametrize("k", sorted(Cs.FIR))
def test_fir_frames_bit_for_bit(dsr, cuda, k, kind):
    dim, lenA, T = Cs.FIR[k]
    x, a, y = Cs.fir_case(k, kind)
    got = dsr.fir_frames(_dev(x[None], cuda), a).cpu().numpy()[0]
    n = dsr.fir_frames_count(T, lenA)
    assert n == y.shape[0] and got.shape == (T + (lenA == 1), dim)
    assert Cs.differing(got[:n], y) == 0 and not got[n:].any()


def test_fir_frames_ragged_batch(dsr, cuda):
    dim, lenA, T = Cs.FIR[2]
    x, a, y = Cs.fir_case(2, "random")
    x1 = Cs.signal(920, T, dim)
    got = dsr.fir_frames(_dev(np.stack([x, x1]), cuda), a, _dev(np.array([T, 17], np.int32), cuda)).cpu().numpy()
    assert Cs.differing(got[0], y) == 0
    assert Cs.differing(got[1, :17], R.filter_feature(x1[:17], a)) == 0 and not got[1, 17:].any()
    one = dsr.fir_frames(_dev(x1[None, :1], cuda), a, _dev(np.array([1], np.int32), cuda)).cpu().numpy()      # T < o: an empty stream
    assert dsr.fir_frames_count(1, lenA) == 0 and not one.any()


def _passes(op):
    first = [np.array(v) for v in op]
    assert op.isEnd()
    op.reset()
    assert op.frameX() == -1
    second = [np.array(v) for v in op]
    assert len(first) == len(second) and all(Cs.differing(p, q) == 0 for p, q in zip(first, second))
    return np.stack(first) if first else np.zeros((0, op.size()), np.float32)


def test_convolution_streams(dsr, cuda):
    from dsr.btk.convolution import OverlapAddPtr, OverlapSavePtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    L, P, fftLen, T, C = Cs.ADD[3]
    x, h, N, y, buf = Cs.add_case(3)
    ola = OverlapAddPtr(PyVectorFloatFeatureStreamPtr(Frames(x)), h[0])
    assert ola.size() == L and ola.name() == "Overlap Add"
    got = _passes(ola)                                                   # the second pass starts from a zeroed buffer again
    assert Cs.differing(got, dsr.BlockConvolver("add", L, h[0]).apply(_dev(x[None], cuda)).cpu().numpy()[0, 0]) == 0
    _check("stream add", got, y[0], N, _xnorm(x), np.linalg.norm(h[0]))
    assert OverlapAddPtr(PyVectorFloatFeatureStreamPtr(Frames(x)), h[0], 1024, "ola").name() == "ola"

    L, P, T, C = Cs.SAVE[2]
    x, h, y = Cs.save_case(2)
    ols = OverlapSavePtr(PyVectorFloatFeatureStreamPtr(Frames(x)), h[0])
    assert ols.size() == L - P and ols.name() == "Overlap Save"
    _check("stream save", _passes(ols), y[0], L, _xnorm(x), np.linalg.norm(h[0]))
    rng = np.random.default_rng(7)
    delta = 0.1 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    ols.update(delta)
    _check("stream save, updated", _passes(ols), R.overlap_save(x, h[0], "ld", delta), L, _xnorm(x), np.linalg.norm(R.save_response(h[0], L, delta)))


@pytest.mark.parametrize("k", sorted(Cs.FIR))
def test_filter_and_merge_streams(dsr, cuda, k):
    from dsr.btk.feature import FilterFeaturePtr, MergeFeaturePtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    dim, lenA, T = Cs.FIR[k]
    x, a, y = Cs.fir_case(k, "random")
    f = FilterFeaturePtr(PyVectorFloatFeatureStreamPtr(Frames(x)), a)
    assert f.size() == dim and f.name() == "Filter"
    got = _passes(f)
    assert got.shape == y.shape and Cs.differing(got, y) == 0
    src = PyVectorFloatFeatureStreamPtr(Frames(x))
    d = FilterFeaturePtr(src, a, "d"); dd = FilterFeaturePtr(d, a, "dd")
    m = MergeFeaturePtr(src, d, dd)
    assert m.size() == 3 * dim and m.name() == "Merge" and dd.name() == "dd"
    ref = R.merge_feature(x, y, R.filter_feature(np.array(y), a))
    gm = _passes(m)
    assert gm.shape == ref.shape and Cs.differing(gm, ref) == 0


def test_mfcc_delta_chain_on_headset(dsr, cuda, headset):
    from dsr.btk.feature import (SampleFeaturePtr, PreemphasisFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr,
                                 MelFeaturePtr, LogFeaturePtr, CepstralFeaturePtr, FilterFeaturePtr, MergeFeaturePtr)
    s = SampleFeaturePtr(blockLen=320, shiftLen=160); s.setSamples(headset[:320 + 160 * 50], 16000)
    cep = CepstralFeaturePtr(LogFeaturePtr(MelFeaturePtr(SpectralPowerFeaturePtr(FFTFeaturePtr(HammingFeaturePtr(PreemphasisFeaturePtr(s, mu=0.95)),
                                                                                            fftLen=512), powN=257), powN=257, filterN=30)), ncep=13)
    a = R.regression_delta(2)
    d = FilterFeaturePtr(cep, a, "Delta"); dd = FilterFeaturePtr(d, a, "DeltaDelta")
    m = MergeFeaturePtr(cep, d, dd)
    got = _passes(m)
    assert got.shape == (50, 39) and np.abs(got[:, 13:]).max() > 0.0
    stat = np.ascontiguousarray(got[:, :13])
    rd = R.filter_feature(stat, a)
    assert Cs.differing(got, R.merge_feature(stat, rd, R.filter_feature(rd, a))) == 0
    assert Cs.differing(stat, np.stack([np.array(v) for v in cep])) == 0


def _refused(dsr, call, status=5):                                       # JDIMENSION + 1
    with pytest.raises(dsr.DsrError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))


def test_refusals_leave_the_device_usable(dsr, cuda):
    from dsr.btk.convolution import OverlapAddPtr, OverlapSavePtr
    from dsr.btk.feature import FilterFeaturePtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    x, h, N, y, buf = Cs.add_case(1)

    def usable():
        got = dsr.BlockConvolver("add", 4, h).apply(_dev(x[None], cuda)).cpu().numpy()[0, 0]
        _check("after a refusal", got, y[0], N, _xnorm(x), np.linalg.norm(h[0]))
    src = lambda n: PyVectorFloatFeatureStreamPtr(Frames(np.zeros((2, n), np.float32)))      # noqa: E731
    cases = [
        lambda: dsr.BlockConvolver("add", 64, np.ones(3), 100),                        # fftLen no power of two
        lambda: dsr.BlockConvolver("save", 100, np.ones(3)),                           # L no power of two
        lambda: dsr.BlockConvolver("add", 64, np.ones(3), 64),                         # fftLen < L+P-1
        lambda: dsr.BlockConvolver("save", 8, np.ones(8)),                             # P >= L
        lambda: dsr.BlockConvolver("save", 8, np.ones(9)),
        lambda: dsr.BlockConvolver("add", 4, np.ones(3), 1 << 23),                     # N above 2^22
        lambda: dsr.BlockConvolver("add", (1 << 22) + 1, np.ones(3)),
        lambda: dsr.fir_frames(_dev(np.zeros((1, 4, 2), np.float32), cuda), np.ones(4)),   # even lenA
        lambda: FilterFeaturePtr(src(2), np.ones(6)),
        lambda: dsr.BlockConvolver("save", 8, np.ones(3)).update(np.zeros(5, np.complex128)),   # update with the wrong length
        lambda: OverlapSavePtr(src(8), np.ones(3)).update(np.zeros(7, np.complex128)),
        lambda: OverlapAddPtr(src(64), np.ones(3), 100),
        lambda: OverlapSavePtr(src(8), np.ones(8)),
    ]
    for call in cases:
        _refused(dsr, call)
        usable()
    _refused(dsr, lambda: dsr.BlockConvolver("add", 4, None), 13)         # a null response: JPARAMETER + 1
    _refused(dsr, lambda: OverlapAddPtr(src(4), None), 13)
    usable()
