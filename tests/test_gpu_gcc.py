"""GPU tests of the pairwise time-delay estimators (include/dsr.h section 2e) against the numpy restatement tests/gcc_np.py.

Tolerances are those the project asserts for fp64 device work against a numpy restatement (test_gpu_doa.py): spectra and correlation
within 1e-12 of the frame's largest magnitude, maxCorr relative 1e-12, the peak index equal wherever best and second best differ by more
than 1e-9 of the scale, ratio relative 1e-9 where |maxCorr2| exceeds 1e-6 of the scale, the interpolated delay within 1e-6 of a sample
period where the restatement's denominator exceeds 1e-6 in relative terms.  At most 2 % of a case's items may be left out of the index
or interpolation comparison (tests/test_gcc_np_cpu.py checks that the inputs satisfy this)."""
import numpy as np
import pytest

from tests import gcc_cases as K
from tests import gcc_np as G

pytestmark = pytest.mark.gpu


def _t(a, cuda, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t.to(dt) if dt is not None else t


def _run(dsr, cuda, case, b, state=None, g=None, sl=slice(None), **kw):
    import torch
    g = g or dsr.Gcc(case["kind"], b["pairs"], sampleRate=K.SR, fftLen=case["N"], nChan=case["C"], interpolate=case["interp"])
    U = b["X"].shape[0]
    if state is None:
        state = g.newState(U, cuda)
    X = _t(b["X"][:, :, sl], cuda, torch.complex128 if case["dbl"] else torch.complex64)
    nf = np.clip(b["nframes"] - (sl.start or 0), 0, X.shape[2]).astype(np.int32)
    r = g.run(X, _t(b["sad"][:, sl], cuda), _t(b["ts"][:, sl], cuda), state, _t(nf, cuda), smooth=case["smooth"], minDelay=b["minDelay"],
              maxDelay=b["maxDelay"], **kw)
    torch.cuda.synchronize()
    return r, g, state


def _compare(case, b, ref, r):
    res = r["result"].cpu().numpy(); valid = r["valid"].cpu().numpy(); corr = r["corr"].cpu().numpy(); xs = r["xspec"].cpu().numpy()
    U, T, P = valid.shape
    items = left = 0
    for u in range(U):
        for t in range(T):
            for p in range(P):
                if t >= b["nframes"][u]:
                    assert valid[u, t, p] == 0 and not res[u, t, p].any()
                    continue
                assert valid[u, t, p] == ref["valid"][u, t, p], (u, t, p)
                if not valid[u, t, p]:
                    assert not res[u, t, p].any()
                    continue
                rc = ref["corr"][u, t, p]; scale = np.abs(rc).max(); info = ref["info"][u, t, p]
                assert np.abs(corr[u, t, p] - rc).max() <= 1e-12 * scale, (u, t, p)
                if b["sad"][u, t]:
                    rx = ref["xspec"][u, t, p]
                    assert np.abs(xs[u, t, p] - rx).max() <= 1e-12 * np.abs(rx).max(), (u, t, p)
                assert abs(res[u, t, p, 1] - info["maxCorr"]) <= 1e-12 * abs(info["maxCorr"]), (u, t, p)
                idx, ratio, interp = K.comparable(info, rc)
                items += 1
                if not idx or (case["interp"] and not interp):
                    left += 1
                if idx and not case["interp"]:
                    assert res[u, t, p, 0] == info["delay"], (u, t, p)
                if ratio:
                    assert abs(res[u, t, p, 2] - info["ratio"]) <= 1e-9 * abs(info["ratio"]), (u, t, p)
                if case["interp"] and interp:
                    assert abs(res[u, t, p, 0] - info["delay"]) * K.SR <= 1e-6, (u, t, p, res[u, t, p, 0] * K.SR, info["delay"] * K.SR)
    assert items > 0 and left <= 0.02 * items, (items, left)


@pytest.mark.parametrize("i", range(len(K.CASES)))
def test_gcc_batch_matches_restatement(dsr, cuda, i):
    case = K.CASES[i]; b = K.build(case); ref = K.reference(case, b)
    r, g, state = _run(dsr, cuda, case, b, want_corr=True, want_xspec=True)
    _compare(case, b, ref, r)
    # the carried state against the restatement's objects
    U = b["X"].shape[0]
    for u in range(U):
        o = ref["gcc"][u]
        for c in range(case["C"]):
            a, ex = g.read(state, U, g.NOISE_POWER, u, c)
            assert ex == (o.np_[c].p is not None)
            if ex:
                assert np.abs(a - o.np_[c].p).max() <= 1e-12 * np.abs(o.np_[c].p).max(), (u, c)
        for p in range(len(b["pairs"])):
            a, ex = g.read(state, U, g.NOISE_CROSS, u, p)
            assert ex == (o.nc[p].g is not None)
            if ex:
                assert np.abs(a - o.nc[p].g).max() <= 1e-12 * np.abs(o.nc[p].g).max(), (u, p)
            a, ex = g.read(state, U, g.CORRELATION, u, p)
            assert ex == bool(o.valid[p])
            if ex:
                assert np.abs(a - o.corr[p]).max() <= 1e-12 * np.abs(o.corr[p]).max(), (u, p)


@pytest.mark.parametrize("i", [1, 5, 9])
def test_two_blocks_with_carried_state_equal_one_call(dsr, cuda, i):
    import torch
    case = K.CASES[i]; b = K.build(case); T = case["T"]; cut = T // 2
    one, g, s1 = _run(dsr, cuda, case, b, want_corr=True)
    ra, g2, s2 = _run(dsr, cuda, case, b, sl=slice(0, cut), want_corr=True)
    rb, _, _ = _run(dsr, cuda, case, b, state=s2, g=g2, sl=slice(cut, T), want_corr=True)
    for k in ("result", "valid", "corr"):
        two = torch.cat([ra[k], rb[k]], dim=1)
        assert torch.equal(two.view(torch.int64) if two.dtype == torch.float64 else two, one[k].view(torch.int64) if one[k].dtype == torch.float64 else one[k]), k
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))


def test_gnnsub_without_noise_is_an_error(dsr, cuda):
    case = dict(K.CASES[1], sad="speech_first"); b = K.build(case)
    with pytest.raises(dsr.DsrError) as e:
        _run(dsr, cuda, case, b)
    assert e.value.status == 1                                               # DSR_E_ERROR


@pytest.mark.parametrize("kind,cls", [("raw", "GCCRawPtr"), ("gnnsub", "GCCGnnSubPtr"), ("phat", "GCCPhatPtr"), ("gnnsubphat", "GCCGnnSubPhatPtr"),
                                      ("mlrraw", "GCCMLRRawPtr"), ("mlrgnnsub", "GCCMLRGnnSubPtr")])
def test_per_call_classes_equal_the_batch(dsr, cuda, kind, cls):
    import torch
    from dsr.btk import localization
    case = dict(kind=kind, N=64, C=3, pairs="all", T=9, sad="lead", smooth=True, win=None, interp=True, dbl=True, seed=21)
    b = K.build(case, U=1); pairs = b["pairs"]
    r, g, state = _run(dsr, cuda, case, b, want_corr=True)
    res = r["result"].cpu().numpy(); valid = r["valid"].cpu().numpy()
    o = getattr(localization, cls)(sampleRate=K.SR, fftLen=64, nChan=3, pairs=len(pairs))
    full = np.concatenate([b["X"], np.conj(b["X"][..., 31:0:-1])], axis=-1)  # the per-call face takes all fftLen bins, as the reference does
    for t in range(case["T"]):
        for p, (c1, c2) in enumerate(pairs):
            o.calculate(full[0, c1, t], c1, full[0, c2, t], c2, p, b["ts"][0, t], bool(b["sad"][0, t]), True)
            got = o.findMaximum()
            if valid[0, t, p]:
                assert np.array_equal(got, res[0, t, p]), (t, p)
                assert o.getPeakDelay() == res[0, t, p, 0] and o.getPeakCorr() == res[0, t, p, 1] and o.getRatio() == res[0, t, p, 2]
                assert np.array_equal(o.getCrossCorrelation(), r["corr"][0, t, p].cpu().numpy())
            else:
                assert not got.any()
    for c in range(3):
        assert np.array_equal(o.getNoisePowerSpectrum(c), g.read(state, 1, g.NOISE_POWER, 0, c)[0])
    assert np.array_equal(o.getNoiseCrossSpectrum(1), g.read(state, 1, g.NOISE_CROSS, 0, 1)[0])
    o.setAlpha(0.7); assert o.getAlpha() == 0.7


@pytest.mark.parametrize("nHeld", [1, 3, 8])
@pytest.mark.parametrize("n,bl", [(64, 64), (512, 400), (2048, 2048), (4096, 4000), (8192, 8192)])
def test_cctde_batch(dsr, cuda, nHeld, n, bl):
    """fftLen up to 4096 runs in LDS, 8192 on the global-memory path.  Every lag of every block is compared, but for block 2: its two blocks
    are the same samples, the correlation is a one at lag 0 and rounding noise elsewhere, so only its first rank is.  tests/test_gcc_np_cpu.py
    shows for these seeds that everywhere else the restatement's nHeld + 1 largest values differ by more than 1e-9 of the scale."""
    s = K.cctde_noise(n, nHeld)
    a, b = K.cctde_blocks(s, n, bl)
    d, ar, v = dsr.cctde(_t(a, cuda), _t(b, cuda), n, nHeld, 16000)
    d, ar, v = d.cpu().numpy(), ar.cpu().numpy(), v.cpu().numpy()
    for k in range(6):
        cc = G.cctde_cc(a[k], b[k], n)
        rd, rl, rv = G.cctde_peaks(cc, nHeld, 16000)
        assert np.abs(v[k] - rv).max() <= 1e-12 * np.abs(cc).max(), k
        m = 1 if k == 2 else nHeld
        assert np.array_equal(np.where(ar[k] >= n // 2, ar[k] - n, ar[k])[:m], rl[:m]) and np.array_equal(d[k][:m], rd[:m]), k
        if k != 5:
            assert rl[0] == (k - 2) * 3


def test_cctde_ptr(dsr, cuda):
    from dsr.btk.feature import SampleFeaturePtr
    from dsr.btk.TDEstimator import CCTDEPtr
    r = np.random.default_rng(9); s = (1000 * r.standard_normal(4000)).astype(np.float32)
    x1, x2 = s[100:2148], s[96:2144]                                         # x2(t) = x1(t - 4)
    s1 = SampleFeaturePtr(blockLen=256, shiftLen=256, padZeros=True); s2 = SampleFeaturePtr(blockLen=256, shiftLen=256, padZeros=True)
    s1.setSamples(x1, 16000); s2.setSamples(x2, 16000)
    o = CCTDEPtr(s1, s2, nHeldMaxCC=3)
    for k in range(3):
        got = o.next().copy()
        rd, rl, rv = G.cctde(x1[k * 256:(k + 1) * 256], x2[k * 256:(k + 1) * 256], 256, 3, 16000)
        assert np.array_equal(got, rd) and rl[0] == 4 and o.getSampleDelays()[0] == 4
        assert np.abs(o.getCCValues() - rv).max() < 1e-12
    got = o.nextX(1).copy()                                                  # channel 1 moves on, channel 0 stays at block 2
    rd, rl, rv = G.cctde(x1[512:768], x2[768:1024], 256, 3, 16000)
    assert np.abs(o.getCCValues() - rv).max() < 1e-12 and o.frameX() == 2
    assert np.array_equal(got, rd) and np.array_equal(o.getSampleDelays().astype(np.int32), np.where(rl < 0, rl + 256, rl))
    got = o.next().copy()                                                    # both move on: blocks 3 and 4
    rd, rl, rv = G.cctde(x1[768:1024], x2[1024:1280], 256, 3, 16000)
    assert np.abs(o.getCCValues() - rv).max() < 1e-12 and np.array_equal(got, rd) and o.frameX() == 3
    got = o.nextX(0).copy()                                                  # channel 0 catches up: blocks 4 and 4, the delay is back
    rd, rl, rv = G.cctde(x1[1024:1280], x2[1024:1280], 256, 3, 16000)
    assert np.array_equal(got, rd) and rl[0] == 4 and o.getSampleDelays()[0] == 4 and o.frameX() == 4
    o.allsamples(2048)
    rd, rl, rv = G.cctde(x1, x2, 2048, 3, 16000)
    assert np.array_equal(o.next(o.frameX()), rd) and rl[0] == 4
    o.reset()
    got = [o.next().copy() for _ in range(8)]                                # the FFT length stays 2048, as in the reference
    assert np.array_equal(got[7], G.cctde(x1[1792:2048], x2[1792:2048], 2048, 3, 16000)[0])
    with pytest.raises(StopIteration):
        o.next()
    with pytest.raises(dsr.DsrError) as e:
        CCTDEPtr(s1, s2, nHeldMaxCC=256)
    assert e.value.status == dsr.E_DIMENSION


def test_gcc_steers_a_delay_and_sum_beamformer(dsr, cuda):
    """8-channel linear array, one broadband source with integer-sample delays, NormalFFTAnalysisBank -> star GCC-PHAT -> channel delays ->
    calcArrayManifoldVectors: the weights equal those of the true delays (the sample delays are exact, tests/test_gcc_np_cpu.py)."""
    import torch
    C, N, T = 8, 256, 6
    r = np.random.default_rng(77)
    true = np.array([(3 * c) % 7 - 3 for c in range(C)], float)
    L = (T + 2) * N
    s = r.standard_normal(L + 16)
    x = np.stack([s[8 - int(d):8 - int(d) + L] + 0.02 * r.standard_normal(L) for d in true]).astype(np.float32)[None]
    bank = dsr.NormalFFTBank(N, 1, 2)
    X = bank.analysis(_t(x, cuda))[..., :N // 2 + 1].contiguous()
    Tn = X.shape[2]; pairs = K.star(C)
    g = dsr.Gcc("phat", pairs, sampleRate=K.SR, fftLen=N, nChan=C, interpolate=False)
    res = g.run(X, torch.ones((1, Tn), dtype=torch.int32), torch.arange(1, Tn + 1, dtype=torch.float64)[None] * 0.01, g.newState(1, cuda))
    pd = res["result"][0, Tn - 1, :, 0].cpu().numpy()
    assert np.array_equal(pd * K.SR, true[0] - true[1:])
    delays = g.channelDelays(pd)
    bf = dsr.Beamformer(N, C); bf.calcArrayManifoldVectors(K.SR, delays); w = bf.get(0).copy()
    bf.calcArrayManifoldVectors(K.SR, (true - true[0]) / K.SR)
    assert np.abs(w - bf.get(0)).max() <= 1e-12


def test_cctde_allsamples_over_a_recording(dsr, cuda):
    """allsamples() with its default argument: the whole recordings in one transform, 20000 and 19000 samples -> fftLen 32768."""
    from dsr.btk.feature import SampleFeaturePtr
    from dsr.btk.TDEstimator import CCTDEPtr
    x1, x2 = K.cctde_recording()
    s1 = SampleFeaturePtr(blockLen=256, shiftLen=256, padZeros=True); s2 = SampleFeaturePtr(blockLen=256, shiftLen=256, padZeros=True)
    s1.setSamples(x1, 16000); s2.setSamples(x2, 16000)
    o = CCTDEPtr(s1, s2, nHeldMaxCC=3)
    o.allsamples()
    b2 = np.zeros(20000, np.float32); b2[:19000] = x2
    cc = G.cctde_cc(x1, b2, 32768); rd, rl, rv = G.cctde_peaks(cc, 3, 16000)
    assert rl[0] == 11
    assert np.abs(o.getCCValues() - rv).max() <= 1e-12 * np.abs(cc).max()
    assert np.array_equal(o.next(o.frameX()), rd) and np.array_equal(o.getSampleDelays().astype(np.int32), np.where(rl < 0, rl + 32768, rl))
