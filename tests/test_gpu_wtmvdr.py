"""WarpedTwiceMVDRFeature (lpc.cc:212-468) and SpectralSmoothing (lpc.cc:473-529) on the device against the restatement of tests/wtmvdr_np.py."""
import numpy as np
import pytest

from tests import wtmvdr_cases as Cs
from tests import wtmvdr_np as W

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -23        # one fp32 ulp of the power: its float rounding is the only place where a last-bit fp64 difference grows, and sqrt halves it


def _same_f32(got, want):
    """bit-equal where the restatement is a number, NaN where it is NaN (the payload of a NaN is the platform's)"""
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(nan, np.isnan(got)) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def _check_out(got, want, what):
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), what
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    assert np.all(np.abs(got[fin] - want[fin]) <= TOL * np.abs(want[fin])), (what, np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])))
    return int((got[fin] != want[fin]).sum())


def _run(dsr, cuda, ci, fr, warps=None, warp=None):
    import torch
    dim, order, corr, wp, fixed, sens, _ = Cs.CASES[ci]
    plan = dsr.WtMvdrEnvelope(dim, order, corr, wp if warp is None else warp, fixed, sens)
    out, pa, rw = plan.run(torch.from_numpy(np.ascontiguousarray(fr)).to(cuda), None if warps is None else torch.from_numpy(warps).to(cuda), want_pa=True)
    return out.cpu().numpy(), pa.cpu().numpy(), rw.cpu().numpy()


@pytest.mark.parametrize("ci", range(len(Cs.CASES)))
def test_wtmvdr_cases(dsr, cuda, ci):
    """Every case tiled to T = 70 (two waves, the second partial): rewarp and PA bit for bit, the envelope within 2^-23 relative."""
    base = Cs.frames(ci); rs = Cs.restated(ci); n = len(rs); T = 70
    idx = np.arange(T) % n
    out, pa, rw = _run(dsr, cuda, ci, base[idx])
    assert out.shape == (T, Cs.CASES[ci][0] // 2 + 1) and pa.shape == (T, Cs.CASES[ci][0] + 1)
    assert _same_f32(rw, np.array([rs[i]["rewarp"] for i in idx]))
    assert _same_f32(pa, np.stack([rs[i]["PA"] for i in idx]))
    nd = _check_out(out, np.stack([rs[i]["out"] for i in idx]), ci)
    print("case %d: %d of %d envelope values differ from the restatement" % (ci, nd, out.size))


def test_wtmvdr_chunk_boundary(dsr, cuda):
    """T = 65 536 + 6: the rows on both sides of the pass boundary, and the first and last, are their frames' restated rows."""
    base = Cs.frames(0); rs = Cs.restated(0); n = len(rs); T = 65536 + 6
    idx = np.arange(T) % n
    out, pa, rw = _run(dsr, cuda, 0, base[idx])
    rows = np.r_[0:3, 65536 - 8:65536 + 6]
    assert _same_f32(rw[rows], np.array([rs[i]["rewarp"] for i in idx[rows]]))
    assert _same_f32(pa[rows], np.stack([rs[i]["PA"] for i in idx[rows]]))
    _check_out(out[rows], np.stack([rs[i]["out"] for i in idx[rows]]), "boundary")
    # every later repetition of a frame is the first one's row
    assert np.array_equal(out[n:2 * n], out[:n], equal_nan=True)
    k = (T // n - 1) * n
    assert np.array_equal(out[k:k + n], out[:n], equal_nan=True) and np.array_equal(pa[k:k + n], pa[:n], equal_nan=True)


@pytest.mark.parametrize("ci", [0, 2])
def test_wtmvdr_per_frame_warps(dsr, cuda, ci):
    """warp_dev: two warps alternating across the frames; row t is the row of a plan built with that frame's warp (and of the restatement)."""
    base = Cs.frames(ci); n = len(base); T = 70
    idx = np.arange(T) % n
    w2 = (np.float32(Cs.CASES[ci][3]), np.float32(0.25))
    warps = np.where(np.arange(T) % 2 == 0, w2[0], w2[1]).astype(np.float32)
    out, pa, rw = _run(dsr, cuda, ci, base[idx], warps=warps)
    for j, w in enumerate(w2):
        o1, p1, r1 = _run(dsr, cuda, ci, base[idx], warp=float(w))
        sel = np.arange(T) % 2 == j
        assert np.array_equal(out[sel], o1[sel], equal_nan=True) and np.array_equal(pa[sel], p1[sel], equal_nan=True) and np.array_equal(rw[sel], r1[sel], equal_nan=True)
    rs = Cs.restated(ci, True, 0.25)                           # the odd rows against the restatement with the second warp
    odd = np.arange(1, T, 2)
    assert _same_f32(pa[odd], np.stack([rs[i]["PA"] for i in idx[odd]]))
    _check_out(out[odd], np.stack([rs[i]["out"] for i in idx[odd]]), "second warp")


@pytest.mark.parametrize("size", [2, 3, 5, 161])
def test_spectral_smoothing(dsr, cuda, size):
    """The arithmetic is fixed (double taps rounded to float, exact maxima, one float division), so the result equals the restatement's."""
    import torch
    rng = np.random.default_rng(900 + size); T = 70
    to = rng.uniform(0.0, 50.0, (T, size)); frm = rng.uniform(0.0, 1e6, (T, size))
    to[7] = 0.0                                                # maxSPEC < 0.01: mult = 100 maxFFT
    to[8] = rng.uniform(0.0, 0.009, size)
    frm[9] = -frm[9]                                           # an adjustFrom all negative: maxFFT stays 0
    got = dsr.spectral_smoothing(torch.from_numpy(to).to(cuda), torch.from_numpy(frm).to(cuda)).cpu().numpy()
    want = np.stack([W.spectral_smoothing(to[t], frm[t]) for t in range(T)])
    assert np.array_equal(got, want)
    if size >= 5:
        assert got[0].any() and not got[9].any()
    with pytest.raises(dsr.DsrError) as e:
        dsr.spectral_smoothing(torch.from_numpy(to).to(cuda), torch.zeros((T, size + 1), dtype=torch.float64, device=cuda))      # lpc.cc:476-477
    assert e.value.status == dsr.E_DIMENSION


def _hamming_frames(oracle, x, blockLen, shiftLen):
    blocks = oracle.sample_blocks(x, blockLen, shiftLen, False)
    w = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(blockLen) / (blockLen - 1.0))
    return (blocks.astype(np.float64) * w).astype(np.float32)


def test_wtmvdr_feature_streams(dsr, oracle, cuda, headset):
    """Sample -> Hamming -> WarpedTwiceMVDRFeaturePtr behind the stream protocol against the restatement on the oracle's blocks, a second pass
    after reset(), the index error, and the chain on to cepstra."""
    from dsr.btk import feature as F
    x = headset[:16000].astype(np.float32)
    samp = F.SampleFeaturePtr(blockLen=320, shiftLen=160, padZeros=False); samp.setSamples(x, 16000)
    ham = F.HammingFeaturePtr(samp)
    op = F.WarpedTwiceMVDRFeaturePtr(ham, order=30, warp=0.4595)
    assert op.size() == 161 and op.name() == "WTMVDR"
    with pytest.raises(dsr.DsrError) as e:
        op.next(5)                                              # lpc.cc:413-415
    assert e.value.status == dsr.E_INDEX
    rows = np.array([np.array(v) for v in op])
    fr = _hamming_frames(oracle, x, 320, 160)
    want = np.stack([W.wtmvdr_frame(f, 30, 0, 0.4595, False, 0.1)["out"] for f in fr])
    assert rows.shape == want.shape
    _check_out(rows, want, "stream")
    op.reset()
    again = np.array([np.array(op.next(t)) for t in range(len(rows))])
    assert np.array_equal(again, rows, equal_nan=True)
    with pytest.raises(StopIteration):
        op.next(len(rows))
    cep = F.CepstralFeaturePtr(F.LogFeaturePtr(F.MelFeaturePtr(op)))
    assert cep.size() == 13 and len([np.array(v) for v in cep]) == len(rows)
    with pytest.raises(dsr.DsrError) as e:
        F.WarpedTwiceMVDRFeaturePtr(ham, order=161)           # lpc.cc:349-350
    assert e.value.status == dsr.E_PARAMETER


def test_spectral_smoothing_stream(dsr, oracle, cuda, headset):
    """SpectralSmoothingPtr(WTMVDR, SpectralPower) on 512-sample windows (the power spectrum's 257 bins are the envelope's) equals the restatement
    on the two upstreams' rows; a second pass after reset() repeats it; unequal sizes and a wrong frameX raise."""
    from dsr.btk import feature as F
    x = headset[4000:8000].astype(np.float32)
    samp = F.SampleFeaturePtr(blockLen=512, shiftLen=160, padZeros=False); samp.setSamples(x, 16000)
    ham = F.HammingFeaturePtr(samp)
    wt = F.WarpedTwiceMVDRFeaturePtr(ham, order=30, warp=0.4595)
    pw = F.SpectralPowerFeaturePtr(F.FFTFeaturePtr(ham, fftLen=512), powN=257)
    to = np.array([np.array(v) for v in wt]); frm = np.array([np.array(v) for v in pw])
    assert to.shape == frm.shape and to.shape[1] == 257 and to.shape[0] > 10
    fr = _hamming_frames(oracle, x, 512, 160)
    _check_out(to[:3], np.stack([W.wtmvdr_frame(f, 30, 0, 0.4595, False, 0.1)["out"] for f in fr[:3]]), "512-sample windows")
    sm = F.SpectralSmoothingPtr(wt, pw)
    assert sm.size() == 257 and sm.name() == "Spectral Smoothing"
    with pytest.raises(dsr.DsrError) as e:
        sm.next(3)                                              # lpc.cc:489-491
    assert e.value.status == dsr.E_INDEX
    rows = np.array([np.array(v) for v in sm])
    want = np.stack([W.spectral_smoothing(to[t], frm[t]) for t in range(len(to))])
    assert np.array_equal(rows, want)
    sm.reset()
    assert np.array_equal(np.array([np.array(sm.next(t)) for t in range(len(rows))]), rows)
    samp2 = F.SampleFeaturePtr(blockLen=320, shiftLen=160, padZeros=False); samp2.setSamples(x, 16000)
    with pytest.raises(dsr.DsrError) as e:
        F.SpectralSmoothingPtr(F.WarpedTwiceMVDRFeaturePtr(F.HammingFeaturePtr(samp2), order=30), pw)      # 161 against 257 (lpc.cc:476-477)
    assert e.value.status == dsr.E_DIMENSION
