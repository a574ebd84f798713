"""GPU tests of the scalar feature operators (include/dsr.h section 6c, csrc/k_featops.hip) against the numpy restatement of
tests/featops_np.py on the cases of tests/featops_cases.py.

The device keeps the reference's operation order and the type of every intermediate, so every comparison is on bits: 0 elements differ (a NaN
equals a NaN).  ALog alone passes through the device's fp64 log10 and gets the bound the project asserts for LogFeature:
|got - ref| <= 1e-5 max(|ref|, |m|).  tests/test_featops_np_cpu.py shows that the value YIN returns beside the pitch sees a wrong summation
order in more than a tenth of the frames."""
import numpy as np
import pytest

from tests import featops_cases as Cs
from tests import featops_np as R

pytestmark = pytest.mark.gpu


class Frames:
    """a Python iterable with size()/reset(), as PyVectorFloatFeatureStreamPtr takes it"""

    def __init__(self, a): self.a = a
    def size(self): return self.a.shape[1]
    def reset(self): pass
    def __iter__(self): return iter(self.a)


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(cuda)                 # a copy: the shared cases are read-only


def _same(tag, got, ref):
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    nd = Cs.differing(got, ref)
    print("%s: %d of %d elements differ in bits" % (tag, nd, ref.size))
    assert nd == 0, (tag, nd)


def _ragged(x, n2=5, seed=0):
    """two utterances [2][T][dim], the second of n2 frames with noise beyond its count that must not be read"""
    T = len(x)
    b = np.random.default_rng(seed).standard_normal(x.shape).astype(x.dtype) * 1000
    b[:n2] = x[T - n2:]
    return np.stack([x, b]), np.array([T, n2], np.int32)


# ---------------------------------------------------------------- YIN
def _yin(dsr, cuda, x, thr=0.5, nf=None):
    p, v = dsr.yin_pitch(_dev(x, cuda), 16000, thr, nframes=None if nf is None else _dev(nf, cuda), return_value=True)
    return p.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("thr", [0.5, 0.1])
def test_yin_headset_pitch_and_value(dsr, cuda, thr):
    x, p, v, tau = Cs.yin_headset(thr)
    assert dsr.yin_kernel(Cs.YIN_N) == 4
    gp, gv, gc = dsr.yin_pitch(_dev(x[None], cuda), 16000, thr, return_value=True, return_chunks=True)
    _same("yin %.1f pitch" % thr, gp.cpu().numpy()[0], p)
    _same("yin %.1f value" % thr, gv.cpu().numpy()[0], v)
    chunks = np.where(tau > 0, tau // 64 + 1, 4)                             # the wave leaves after the chunk of its hit
    assert np.array_equal(gc.cpu().numpy()[0], chunks)


@pytest.mark.parametrize("N", [130, 131, 3, 2, 1024, 4002])
def test_yin_frame_lengths(dsr, cuda, N):
    """W = 65 (one lag beyond a wave), odd N, W = 1 (no lag at all), and the lengths that select the one-frame workgroup (1024) and the kernel
    that reads global memory (4002)"""
    assert dsr.yin_kernel(N) == (4 if N <= 960 else 1 if N <= 4000 else 0)
    x = Cs.frames(N, max(N, 160), 6 if N > 1000 else 23, start=3000)
    for thr in (0.5, 0.1):
        p, v = R.yin_pitch(x, 16000, thr)
        gp, gv = _yin(dsr, cuda, x[None], thr)
        _same("yin N=%d thr %.1f pitch" % (N, thr), gp[0], p)
        _same("yin N=%d thr %.1f value" % (N, thr), gv[0], v)


def test_yin_silence_sine_and_ragged(dsr, cuda):
    z = np.zeros((1, 512), np.float32)
    gp, gv = _yin(dsr, cuda, z[None])
    assert gp[0, 0, 0] == 0.0 and np.isnan(gv[0, 0])                         # 0/0 fails both comparisons
    s = Cs.sine_frame()
    p, v = R.yin_pitch(s)
    gp, gv = _yin(dsr, cuda, s[None])
    _same("sine pitch", gp[0], p); _same("sine value", gv[0], v)
    x, p, v, tau = Cs.yin_headset()
    xb, nf = _ragged(x[:40])
    gp, gv = _yin(dsr, cuda, xb, 0.5, nf)
    _same("ragged u0", gp[0], p[:40]); _same("ragged u0 value", gv[0], v[:40])
    _same("ragged u1", gp[1, :5], p[35:40]); _same("ragged u1 value", gv[1, :5], v[35:40])
    assert not gp[1, 5:].any() and not gv[1, 5:].any()
    with pytest.raises(dsr.DsrError) as e:
        dsr.yin_pitch(_dev(np.zeros((1, 2, 1), np.float32), cuda))
    assert e.value.status == dsr.E_DIMENSION


# ---------------------------------------------------------------- zero-crossing rate, signal power
@pytest.mark.parametrize("N", [2, 64, 65, 400])
def test_zcr_and_signal_power(dsr, cuda, N):
    x = np.concatenate([Cs.frames(N, 160, 30, start=2000), Cs.signed_zero_frame(N)])
    xb, nf = _ragged(x)
    for name, fn, ref in (("zcr", dsr.zero_crossing_rate, R.zero_crossing_rate), ("power", dsr.signal_power, R.signal_power)):
        r = ref(x)
        got = fn(_dev(xb, cuda), _dev(nf, cuda)).cpu().numpy()
        assert got.shape == (2, len(x), 1)
        _same("%s N=%d u0" % (name, N), got[0], r)
        _same("%s N=%d u1" % (name, N), got[1, :5], r[len(x) - 5:])
        assert not got[1, 5:].any()
        _same("%s N=%d no counts" % (name, N), fn(_dev(x[None], cuda)).cpu().numpy()[0], r)


# ---------------------------------------------------------------- SpikeFilter
@pytest.mark.parametrize("tapN", [3, 5, 9])
def test_spike_filter(dsr, cuda, tapN):
    for n in (tapN, tapN + 1, 320):
        for x in (Cs.frames(n, 160, 7, start=5000), Cs.ties_block(n, tapN)):
            r = R.spike_filter(x, tapN)
            xb, nf = _ragged(x, 2)
            got = dsr.spike_filter(_dev(xb, cuda), tapN, _dev(nf, cuda)).cpu().numpy()
            _same("spike tapN=%d n=%d" % (tapN, n), got[0], r)
            _same("spike tapN=%d n=%d u1" % (tapN, n), got[1, :2], r[len(x) - 2:])
            assert not got[1, 2:].any() and not got[0, :, n - (tapN - 1):].any()


def test_spike_filter_refusals(dsr, cuda):
    from dsr.btk.feature import SpikeFilterPtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    x = _dev(np.zeros((1, 2, 8), np.float32), cuda)
    for tapN, n in ((2, 8), (4, 8), (9, 8)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.spike_filter(x[:, :, :n].contiguous(), tapN)
        assert e.value.status == dsr.E_DIMENSION
        with pytest.raises(dsr.DsrError) as e:
            SpikeFilterPtr(PyVectorFloatFeatureStreamPtr(Frames(np.zeros((2, n), np.float32))), tapN)
        assert e.value.status == dsr.E_DIMENSION


# ---------------------------------------------------------------- SpikeFilter2
@pytest.mark.parametrize("name", sorted(Cs.SPIKES))
def test_spike_filter2_cases(dsr, cuda, name):
    x = Cs.with_spikes(Cs.spike_blocks(), Cs.SPIKES[name])
    f = R.SpikeFilter2(); r = f.run(x)
    assert f.count > 0                                                       # the case does take the spike branch
    y, (ms, cnt) = dsr.spike_filter2(_dev(x[None], cuda))
    _same("spike2 " + name, y.cpu().numpy()[0], r)
    assert int(cnt[0]) == f.count and Cs.differing(ms.cpu().numpy(), np.array([f.meanslope], np.float32)) == 0


def test_spike_filter2_batch_and_carried_state(dsr, cuda):
    import torch
    xs = [Cs.with_spikes(Cs.spike_blocks(), Cs.SPIKES[k]) for k in ("middle", "end", "consecutive")]
    nf = np.array([12, 7, 9], np.int32)
    refs = []
    for x, n in zip(xs, nf):
        f = R.SpikeFilter2(width=4, maxslope=6000.0, startslope=80.0, thresh=12.0, alpha=0.1); refs.append((f.run(x[:n]), f.count, f.meanslope))
    kw = dict(width=4, maxslope=6000.0, startslope=80.0, thresh=12.0, alpha=0.1)
    xb = _dev(np.stack(xs), cuda)
    y, (ms, cnt) = dsr.spike_filter2(xb, nframes=_dev(nf, cuda), **kw)
    y = y.cpu().numpy()
    for u, (r, c, m) in enumerate(refs):
        _same("spike2 batch u%d" % u, y[u, :nf[u]], r)
        assert not y[u, nf[u]:].any() and int(cnt[u]) == c and c > 0
        assert Cs.differing(ms[u:u + 1].cpu().numpy(), np.array([m], np.float32)) == 0
    # two calls that carry (meanslope, count) equal one call
    st = dsr.spike_filter2_state(3, 80.0, cuda)
    first = np.minimum(nf, 5).astype(np.int32)
    ya, st = dsr.spike_filter2(xb[:, :5].contiguous(), nframes=_dev(first, cuda), state=st, **kw)
    yb, st = dsr.spike_filter2(xb[:, 5:].contiguous(), nframes=_dev(nf - first, cuda), state=st, **kw)
    _same("spike2 two calls", torch.cat([ya, yb], dim=1).cpu().numpy(), y)
    assert torch.equal(st[1], cnt) and torch.equal(st[0], ms)


# ---------------------------------------------------------------- ALog, Normalize, Threshold, Amplification
def _alog_close(tag, got, ref, m):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = 1e-5 * np.maximum(np.abs(ref.astype(np.float64)), abs(m))
    print("%s: %d of %d elements differ in bits, largest error / tolerance %.3g" % (tag, Cs.differing(got, ref), ref.size, float((err / tol).max())))
    assert got.shape == ref.shape and (err <= tol).all(), tag


@pytest.mark.parametrize("runon", [False, True])
def test_alog_and_normalize(dsr, cuda, runon):
    e = Cs.energy_chain()
    wide = Cs.frames(33, 160, 20, start=7000)                                # min and max go over all 33 elements of a frame
    for x in (e, wide):
        xb, nf = _ragged(x, 5)
        for m, a in ((1.0, 4.0), (10.0, 2.0)):
            r0 = R.ALog(m, a, runon).run(x); r1 = R.ALog(m, a, runon).run(xb[1, :5])
            got = dsr.alog(_dev(xb, cuda), m, a, runon, nframes=_dev(nf, cuda)).cpu().numpy()
            assert got.shape == (2, len(x), 1) and not got[1, 5:].any()
            _alog_close("alog runon=%d m=%g u0" % (runon, m), got[0], r0, m); _alog_close("alog u1", got[1, :5], r1, m)
        r0 = R.Normalize(-1.0, 3.0, runon).run(x); r1 = R.Normalize(-1.0, 3.0, runon).run(xb[1, :5])
        got = dsr.normalize(_dev(xb, cuda), -1.0, 3.0, runon, nframes=_dev(nf, cuda)).cpu().numpy()
        _same("normalize runon=%d u0" % runon, got[0], r0); _same("normalize u1", got[1, :5], r1)
        assert not got[1, 5:].any()
    c = np.full((4, 3), 5.0, np.float32)                                     # range 0: inf or NaN as IEEE gives them
    with np.errstate(all="ignore"):
        _same("normalize constant", dsr.normalize(_dev(c[None], cuda), 0.0, 1.0, runon).cpu().numpy()[0], R.Normalize(0.0, 1.0, runon).run(c))


def test_runon_state_and_next_speaker(dsr, cuda):
    e = Cs.energy_chain()
    a, b = e[:25], e[25:]
    for keep in (True, False):                                               # two utterances through one run-on object, without and with nextSpeaker()
        ra, rn = R.ALog(1.0, 4.0, True), R.Normalize(0.0, 1.0, True)
        sa, sn = dsr.minmax_state(1, cuda), dsr.minmax_state(1, cuda)
        for k, x in enumerate((a, b)):
            if k == 1 and not keep:
                ra.nextSpeaker(); rn.nextSpeaker(); sa, sn = dsr.minmax_state(1, cuda), dsr.minmax_state(1, cuda)
            _alog_close("alog run-on keep=%d utt %d" % (keep, k), dsr.alog(_dev(x[None], cuda), 1.0, 4.0, True, sa).cpu().numpy()[0], ra.run(x), 1.0)
            _same("normalize run-on keep=%d utt %d" % (keep, k), dsr.normalize(_dev(x[None], cuda), 0.0, 1.0, True, sn).cpu().numpy()[0], rn.run(x))
            assert sa.cpu().numpy().tolist() == [[float(ra.mn), float(ra.mx)]] and sn.cpu().numpy().tolist() == [[float(rn.mn), float(rn.mx)]]


def test_threshold_and_amplify(dsr, cuda):
    x = np.array(Cs.frames(40, 160, 9, start=6000)) / np.float32(1000.0)
    x[0, :6] = [1.5, -1.5, 0.0, -0.0, np.nextafter(np.float32(1.5), np.float32(2)), np.nextafter(np.float32(-1.5), np.float32(-2))]
    xb, nf = _ragged(x, 4)
    for mode in ("upper", "lower", "both"):
        got = dsr.threshold(_dev(xb, cuda), 0.25, 1.5, mode, _dev(nf, cuda)).cpu().numpy()
        _same("threshold " + mode, got[0], R.threshold(x, 0.25, 1.5, mode)); _same("threshold u1", got[1, :4], R.threshold(xb[1, :4], 0.25, 1.5, mode))
        assert not got[1, 4:].any()
    with pytest.raises(dsr.DsrError) as e:
        dsr.threshold(_dev(xb, cuda), 0.0, 1.0, "neither")
    assert e.value.status == dsr.E_KEY
    got = dsr.amplify(_dev(xb, cuda), 1.0 / 3.0, _dev(nf, cuda)).cpu().numpy()
    _same("amplify", got[0], R.amplify(x, 1.0 / 3.0)); assert not got[1, 4:].any()


# ---------------------------------------------------------------- SpectralResampling, SphinxMel
def _spectra(T=9, n=257, seed=11):
    return np.abs(np.random.default_rng(seed).standard_normal((T, n))) * 1e3


@pytest.mark.parametrize("ratio,length", [(R.SAMPLE_RATIO, 0), (0.45, 129), (1.0, 0)])
def test_spectral_resample(dsr, cuda, ratio, length):
    x = _spectra()
    xb, nf = _ragged(x, 3)
    got = dsr.spectral_resample(_dev(xb, cuda), ratio, length, _dev(nf, cuda)).cpu().numpy()
    _same("resample %.3f -> %d" % (ratio, length), got[0], R.spectral_resample(x, ratio, length))
    _same("resample u1", got[1, :3], R.spectral_resample(xb[1, :3], ratio, length)); assert not got[1, 3:].any()


def test_spectral_resample_refusals(dsr, cuda):
    x = _dev(_spectra(2, 100)[None], cuda)
    with pytest.raises(dsr.DsrError) as e:
        dsr.spectral_resample(x, 1.0, 50)                                    # effective ratio 2
    assert e.value.status == dsr.E_CONSISTENCY
    with pytest.raises(dsr.DsrError) as e:
        dsr.spectral_resample(x, 1.0, 200)                                   # element 100 of 100 with weight 0.5
    assert e.value.status == dsr.E_DIMENSION


@pytest.mark.parametrize("filterN", [30, 40])
def test_sphinx_mel(dsr, cuda, filterN):
    A = R.sphinx_mel_filters(512, 257, 16000.0, 130.0, 6800.0, filterN)
    plan = dsr.SphinxMel(512, 257, 16000.0, 130.0, 6800.0, filterN)
    _same("sphinx filters %d" % filterN, plan.filters, A)
    x = _spectra()
    xb, nf = _ragged(x, 3)
    got = plan.apply(_dev(xb, cuda), _dev(nf, cuda)).cpu().numpy()
    _same("sphinx apply %d" % filterN, got[0], R.sphinx_mel_apply(A, x)); assert not got[1, 3:].any()


def test_sphinx_mel_defaults_and_refusal(dsr, cuda):
    plan = dsr.SphinxMel()                                                   # lowerF = upperF = 0: an all-zero bank, as in the reference
    assert plan.filters.shape == (30, 257) and not plan.filters.any()
    assert not plan.apply(_dev(_spectra()[None], cuda)).cpu().numpy().any()
    with pytest.raises(dsr.DsrError) as e:
        dsr.SphinxMel(512, 257, 16000.0, 130.0, 8001.0, 30)
    assert e.value.status == 1                                               # the generic j_error


# ---------------------------------------------------------------- the stream face
def _passes(op, dtype=np.float32):
    first = [np.array(v) for v in op]                                        # ends with StopIteration
    assert op.isEnd()
    with pytest.raises(StopIteration):
        op.next()
    op.reset()
    assert op.frameX() == -1
    second = [np.array(v) for v in op]
    assert len(first) == len(second) and all(Cs.differing(p, q) == 0 for p, q in zip(first, second))
    return np.stack(first) if first else np.zeros((0, op.size()), dtype)


def test_energy_chain_streams(dsr, cuda):
    from dsr.btk.feature import ALogFeaturePtr, NormalizeFeaturePtr, SignalPowerFeaturePtr, StorageFeaturePtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    x = Cs.frames(400, 160, 60, start=4000)
    e = Cs.energy_chain()
    power = SignalPowerFeaturePtr(PyVectorFloatFeatureStreamPtr(Frames(x)))
    store = StorageFeaturePtr(power)
    alog = ALogFeaturePtr(store, 1.0, 4.0)
    norm = NormalizeFeaturePtr(alog, 0.0, 1.0)
    assert (power.name(), power.size()) == ("Signal Power", 1) and (alog.name(), alog.size()) == ("ALog Power", 1)
    assert (norm.name(), norm.size()) == ("Normalize", 1) and NormalizeFeaturePtr(alog, nm="n2").name() == "n2"
    got = _passes(norm)
    a = _passes(alog)
    ra = R.ALog(1.0, 4.0).run(e)
    _alog_close("stream alog", a, ra, 1.0)
    _same("stream normalize of the device's alog", got, R.Normalize(0.0, 1.0).run(a))
    _same("stream power", _passes(power), e)
    # run-on keeps the bounds across reset() until nextSpeaker()
    ron = NormalizeFeaturePtr(power, 0.0, 1.0, True)
    rr = R.Normalize(0.0, 1.0, True)
    _same("run-on pass 1", np.stack([np.array(v) for v in ron]), rr.run(e))
    _same("run-on pass 2", np.stack([np.array(v) for v in ron]), rr.run(e))
    ron.nextSpeaker(); rr.nextSpeaker()
    _same("run-on after nextSpeaker", np.stack([np.array(v) for v in ron]), rr.run(e))


def test_spike_and_pitch_streams(dsr, cuda):
    from dsr.btk.feature import (AmplificationFeaturePtr, SpikeFilter2Ptr, SpikeFilterPtr, ThresholdFeaturePtr, YINPitchFeaturePtr,
                                 ZeroCrossingRateHammingFeaturePtr)
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    x = Cs.with_spikes(Cs.spike_blocks(), Cs.SPIKES["middle"])
    src = PyVectorFloatFeatureStreamPtr(Frames(x))
    sp2 = SpikeFilter2Ptr(src)
    yin = YINPitchFeaturePtr(sp2, 16000, 0.5)
    assert (sp2.name(), sp2.size()) == ("Spike Filter 2", 320) and (yin.name(), yin.size()) == ("YIN Pitch", 1)
    f = R.SpikeFilter2(); clean = f.run(x)
    _same("stream yin", _passes(yin), R.yin_pitch(clean)[0])
    assert sp2.spikesN() == f.count and f.count > 0
    _same("stream spike2", _passes(sp2), clean)
    assert sp2.spikesN() == f.count                                          # reset() starts the count again
    zcr = ZeroCrossingRateHammingFeaturePtr(src)
    assert (zcr.name(), zcr.size()) == ("Zero Crossing Rate Hamming", 1)
    _same("stream zcr", _passes(zcr), R.zero_crossing_rate(x))
    med = SpikeFilterPtr(src, 5)
    assert (med.name(), med.size()) == ("Spike Filter", 320)
    _same("stream spike", _passes(med), R.spike_filter(x, 5))
    th = ThresholdFeaturePtr(AmplificationFeaturePtr(src, 0.001), 1.0, 2.0, "both")
    assert th.name() == "Threshold" and th.size() == 320
    _same("stream threshold", _passes(th), R.threshold(R.amplify(x, 0.001), 1.0, 2.0, "both"))
    with pytest.raises(dsr.DsrError) as e:
        ThresholdFeaturePtr(src, 0.0, 1.0, "neither")
    assert e.value.status == dsr.E_KEY


def test_double_streams(dsr, cuda):
    from dsr.btk.feature import SpectralResamplingFeaturePtr, SphinxMelFeaturePtr
    from dsr.btk.stream import PyVectorFeatureStreamPtr
    x = _spectra()
    src = PyVectorFeatureStreamPtr(Frames(x))
    rs = SpectralResamplingFeaturePtr(src)
    assert (rs.name(), rs.size()) == ("Resampling", 257)
    _same("stream resample", _passes(rs, np.float64), R.spectral_resample(x))
    mel = SphinxMelFeaturePtr(src, 512, 0, 16000.0, 130.0, 6800.0, 40)
    assert (mel.name(), mel.size()) == ("Sphinx Mel Filter Bank", 40)
    _same("stream sphinx mel", _passes(mel, np.float64), R.sphinx_mel_apply(R.sphinx_mel_filters(512, 257, 16000.0, 130.0, 6800.0, 40), x))
    with pytest.raises(dsr.DsrError) as e:
        SpectralResamplingFeaturePtr(src, 1.0, 129)
    assert e.value.status == dsr.E_CONSISTENCY
