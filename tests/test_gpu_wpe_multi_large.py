"""Multi-channel WPE past the LDS working set of the one-workgroup kernel (dereverberation.cc:281-620 at array size): the tiled fp64-MFMA path
(csrc/k_wpe_tiled.hip) against the CPU oracle, against the numpy restatement (tests/wpe_multi_np.py) where the oracle is too slow or cannot be
seeded, and against the LDS path on the same small inputs (DSR_WPE_MULTI_TILED=1); the filters carried from one block to the next
(dsr_wpe_multi_continue) on both paths; the operators past the cap."""
import numpy as np
import pytest

from tests import wpe_multi_np as W


def _signal(U, Cn, N, F, seed, taps=10, decay=0.55):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((U, N, F)) + 1j * rng.standard_normal((U, N, F))
    Y = np.zeros((U, Cn, N, F), np.complex128)
    for c in range(Cn):
        Y[:, c] = s * np.exp(1j * c) + 0.1 * (rng.standard_normal((U, N, F)) + 1j * rng.standard_normal((U, N, F)))
        for k in range(1, taps):
            Y[:, c, k:] += (decay + 0.1 * c / Cn) ** k * np.roll(s, k, axis=1)[:, k:] * np.exp(1j * k * (c + 1))
    return Y.astype(np.complex64)


def _full(a, M):          # [C][n][F] -> [C][n][M] with the mirrored half the reference's streams carry
    F = M // 2 + 1
    f = np.zeros(a.shape[:2] + (M,), np.complex128); f[:, :, :F] = a; f[:, :, F:] = np.conj(a[:, :, 1:F - 1][:, :, ::-1]); return f


def _late(a):             # the late part of the response in the output's autocorrelation at the predicted lags (test_wpe_multi_at_benchmark_size)
    return np.mean([np.abs(np.vdot(a[0, :-k, 1], a[0, k:, 1])) for k in range(3, 10)]) / np.real(np.vdot(a[0, :, 1], a[0, :, 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("fc,bw", [(-1, 0.0), (0, 0.0), (-1, 4000.0)])
def test_wpe_multi_past_cap_vs_oracle(dsr, oracle, cuda, fc, bw):
    """32 channels x 8 taps (a 256 x 256 matrix per subband and channel; the LDS path refuses it): two ragged utterances, two iterations.
    Bars: gn rtol 2e-6, outputs 2e-6 of the largest |output|; measured on MI355X: gn 6.4e-13, outputs 4.6e-8 (printed with -s)."""
    import torch
    U, Cn, N, M, lowerN, upperN = 2, 32, 300, 4, 2, 9
    F = M // 2 + 1
    Y = _signal(U, Cn, N, F, 31 + fc)
    nfr = [N, N - 37]
    out, gn = dsr.wpe_multi(torch.from_numpy(Y).to(cuda), M, lowerN, upperN, 2, -20.0, bw, 16000.0,
                            nframes=torch.tensor(nfr, dtype=torch.int32, device=cuda), filterChan=fc)
    out, gn = out.cpu().numpy(), gn.cpu().numpy()
    for u in range(U):
        n = nfr[u]
        wo, wg = oracle.wpe_multi(_full(Y[u, :, :n], M), lowerN, upperN, 2, -20.0, bw, 16000.0, filterChan=fc)
        eg = np.abs(gn[u] - wg[:, :F]).max() / np.abs(wg[:, :F]).max()
        eo = np.abs(out[u, :, :n] - wo[:, :, :F]).max() / np.abs(wo).max()
        print("32x8 fc=%d bw=%g u=%d: gn max rel %.2e, out max rel %.2e" % (fc, bw, u, eg, eo))
        assert np.isfinite(gn[u]).all()
        np.testing.assert_allclose(gn[u], wg[:, :F], rtol=2e-6, atol=1e-9)
        assert eo <= 2e-6
        assert not out[u, :, n:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("upperN", [9, 17])
def test_wpe_multi_array_size(dsr, cuda, upperN):
    """64 channels x 8 and x 16 taps (512 and 1024 stacked lags): the full device call, then (subband, channel) pairs against the restatement
    (measured on MI355X: filters 1.6e-12, outputs 5.2e-8 relative), and the late reverberation drops."""
    import torch
    U, Cn, N, M, lowerN = 1, 64, 1250, 8, 2
    F, P = M // 2 + 1, upperN - lowerN + 1
    Y = _signal(U, Cn, N, F, 5 + upperN, taps=14, decay=0.7)
    out, gn = dsr.wpe_multi(torch.from_numpy(Y).to(cuda), M, lowerN, upperN, 2, -20.0, 0.0, 16000.0, filterChan=-1)
    out, gn = out.cpu().numpy(), gn.cpu().numpy()
    assert np.isfinite(gn).all() and np.isfinite(out).all()
    Yc = Y[0].astype(np.complex128)
    for b, c in [(0, 0), (1, 5), (2, 63), (4, 31)]:
        g = W.filters(Yc[:, :, b], c, lowerN, upperN, 2, -20.0)
        eg = np.abs(gn[0, c, b] - g).max() / np.abs(g).max()
        o = W.predict(Yc[:, :, b], c, g, lowerN, P)
        eo = np.abs(out[0, c, :, b] - o).max() / np.abs(o).max()
        print("64x%d b=%d c=%d: gn max rel %.2e, out max rel %.2e" % (P, b, c, eg, eo))
        assert eg <= 2e-6 and eo <= 2e-6
    assert _late(out[0]) < 0.9 * _late(Yc)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn,lowerN,upperN,iters,loadDb,bw,fc", [(3, 2, 5, 2, -20.0, 0.0, -1), (2, 1, 8, 2, -10.0, 0.0, 1), (4, 3, 4, 1, -30.0, 4000.0, 0)])
def test_wpe_multi_forced_tiled_small(dsr, oracle, cuda, monkeypatch, Cn, lowerN, upperN, iters, loadDb, bw, fc):
    """test_wpe_multi's shapes through the tiled path (DSR_WPE_MULTI_TILED=1): against the oracle and against the LDS path on the same input."""
    import torch
    U, N, M = 2, 120, 32
    F = M // 2 + 1
    Y = _signal(U, Cn, N, F, Cn + lowerN + upperN)
    nfr = [N, N - 21]
    args = (torch.from_numpy(Y).to(cuda), M, lowerN, upperN, iters, loadDb, bw, 16000.0)
    kw = dict(nframes=torch.tensor(nfr, dtype=torch.int32, device=cuda), filterChan=fc)
    outL, gnL = (t.cpu().numpy() for t in dsr.wpe_multi(*args, **kw))
    monkeypatch.setenv("DSR_WPE_MULTI_TILED", "1")
    out, gn = (t.cpu().numpy() for t in dsr.wpe_multi(*args, **kw))
    for u in range(U):
        n = nfr[u]
        wo, wg = oracle.wpe_multi(_full(Y[u, :, :n], M), lowerN, upperN, iters, loadDb, bw, 16000.0, filterChan=fc)
        np.testing.assert_allclose(gn[u], wg[:, :F], rtol=2e-7, atol=1e-10)
        assert np.abs(out[u, :, :n] - wo[:, :, :F]).max() <= 2e-6 * np.abs(wo).max()
        assert not out[u, :, n:].any()
    np.testing.assert_allclose(gn, gnL, rtol=1e-9, atol=1e-12)
    assert np.abs(out - outL).max() <= 1e-6 * np.abs(outL).max()


def _blocks(dsr, cuda, Y, M, lowerN, upperN, nblk):
    """Consecutive blocks of one stream through dsr_wpe_multi_continue, each checked against the restatement seeded with the filters the
    device left after the block before."""
    import torch
    U, Cn, N, F = Y.shape
    P, Lb = upperN - lowerN + 1, N // nblk
    gn = torch.zeros((U, Cn, F, Cn * P), dtype=torch.complex128, device=cuda)
    for k in range(nblk):
        Yk = np.ascontiguousarray(Y[:, :, k * Lb:(k + 1) * Lb])
        seed = gn.cpu().numpy()
        out, gn2 = dsr.wpe_multi(torch.from_numpy(Yk).to(cuda), M, lowerN, upperN, 2, -20.0, 0.0, 16000.0, gn=gn)
        assert gn2 is gn
        g, o = gn.cpu().numpy(), out.cpu().numpy()
        if k > 0:
            assert np.abs(seed).max() > 0
        Yc = Yk[0].astype(np.complex128)
        for b in range(F):
            for c in range(Cn):
                ref = W.filters(Yc[:, :, b], c, lowerN, upperN, 2, -20.0, g0=seed[0, c, b])
                assert np.abs(g[0, c, b] - ref).max() <= 2e-6 * np.abs(ref).max(), (k, b, c)
                ro = W.predict(Yc[:, :, b], c, ref, lowerN, P)
                assert np.abs(o[0, c, :, b] - ro).max() <= 2e-6 * np.abs(ro).max(), (k, b, c)
        if k == 0:     # a cold block differs from a seeded one: the carried filters are used
            continue
        cold = W.filters(Yc[:, :, 1], 0, lowerN, upperN, 2, -20.0)
        assert np.abs(g[0, 0, 1] - cold).max() > 1e-6 * np.abs(cold).max()


@pytest.mark.gpu
def test_wpe_multi_carried_past_cap(dsr, cuda):
    """Three consecutive blocks at 20 channels x 8 taps (tiled path), filters carried (reset() without nextSpeaker())."""
    Y = _signal(1, 20, 360, 3, 11)
    _blocks(dsr, cuda, Y, 4, 2, 9, 3)


@pytest.mark.gpu
def test_wpe_multi_carried_lds(dsr, cuda):
    """The same at 3 channels x 3 taps (LDS path)."""
    Y = _signal(1, 3, 240, 5, 12)
    _blocks(dsr, cuda, Y, 8, 1, 3, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn,upperN,tiled", [(3, 4, False), (3, 4, True), (20, 9, False)])
def test_wpe_multi_continue_from_zero_is_cold(dsr, cuda, monkeypatch, Cn, upperN, tiled):
    """dsr_wpe_multi_continue with all-zero filters equals dsr_wpe_multi bit for bit, on each path (20 x 8 is past the cap: tiled)."""
    import torch
    if tiled:
        monkeypatch.setenv("DSR_WPE_MULTI_TILED", "1")
    M, lowerN = 8, 2
    F = M // 2 + 1
    Y = torch.from_numpy(_signal(2, Cn, 150, F, 3 + Cn)).to(cuda)
    nf = torch.tensor([150, 111], dtype=torch.int32, device=cuda)
    o0, g0 = dsr.wpe_multi(Y, M, lowerN, upperN, 2, -20.0, 0.0, 16000.0, nframes=nf, filterChan=1)
    z = torch.zeros_like(g0)
    o1, g1 = dsr.wpe_multi(Y, M, lowerN, upperN, 2, -20.0, 0.0, 16000.0, nframes=nf, filterChan=1, gn=z)
    assert torch.equal(o0, o1) and torch.equal(g0, g1)


@pytest.mark.gpu
def test_wpe_multi_operators_past_cap(dsr, oracle, cuda):
    """MultiChannelWPEDereverberationPtr / ...FeaturePtr at 20 channels x 8 taps, channel 2's feature pulled first: every channel goes
    through channel 2's filter (dereverberation.cc:381)."""
    from dsr.btk import stream as S, dereverberation as Dv
    Cn, N, M, lowerN, upperN, iters, loadDb, bw = 20, 80, 4, 2, 9, 2, -20.0, 0.0
    F = M // 2 + 1
    fu = _full(_signal(1, Cn, N, F, 21)[0], M)

    class Frames(object):
        def __init__(self, a):
            self.a = a

        def size(self):
            return self.a.shape[1]

        def __iter__(self):
            return iter(self.a)

    src = Dv.MultiChannelWPEDereverberationPtr(M, Cn, lowerN, upperN, iters, loadDb, bw, 16000.0)
    for c in range(Cn):
        src.setInput(S.PyVectorComplexFeatureStreamPtr(Frames(fu[c])))
    feats = [Dv.MultiChannelWPEDereverberationFeaturePtr(src, c) for c in range(Cn)]
    order = [2] + [c for c in range(Cn) if c != 2]
    rows = [[] for _ in range(Cn)]
    for t in range(N):
        for c in order:
            rows[c].append(np.array(feats[c].next(t)))
    wo, _ = oracle.wpe_multi(fu, lowerN, upperN, iters, loadDb, bw, 16000.0, filterChan=2)
    got = np.array(rows)
    assert got.shape == wo.shape and np.abs(got - wo).max() <= 4e-6 * np.abs(wo).max()
