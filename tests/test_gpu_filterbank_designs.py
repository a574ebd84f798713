"""Every oversampled-DFT filter-bank kernel and design the dispatch of csrc/k_filterbank.hip can select, through the entries and the block
state of csrc/filterbank.cpp, against the CPU oracle.

The rest of the GPU suite builds its FilterBank objects from the three prototypes the reference ships, which reach 2 of the 20 analysis
instantiations, 1 of the 4 fused ones and 2 of the 8 synthesis ones.  Here a sweep of designs (tests/fb_np.py: one list per kernel family; the
prototypes of tests/synth.py fb_prototype) runs one-shot analysis and synthesis, the three analysis kernels on one input, the fused
analysis + beamformer kernel at m = 2 and with 8 waves, and the block-wise (carried-history) mode on blocks shorter than the history.

Tolerance: the project's own, max |got - ref| < 2e-5 RMS(ref) per utterance and channel (test_analysis_bank, test_synthesis_bank).  A design
that missed it would be judged by tests/fb_np.py analysis_closed_form(dtype=float32) -- the same closed form in fp32 on the CPU -- never by the
device output alone ("which design reaches which kernel").  With -s every design prints one line with its max error / RMS."""
import numpy as np
import pytest

from tests import fb_np, synth
from tests.conftest import load_proto

TOL = 2e-5
ENVS = ("DSR_FB_GENERIC", "DSR_FB_WAVE", "DSR_FB_NOFUSE", "DSR_FB_TF", "DSR_FB_FUSED_WAVES")


def _proto(design):
    M, m, r = design
    return load_proto(fb_np.SHIPPED[design]) if design in fb_np.SHIPPED else synth.fb_prototype(M, m, r, seed=M + 7 * m + r)


def _gain(dct):
    return 3 if dct == 1 else 1                      # every design sees gainFactor 1 (dct 0, 2) and 3 (dct 1), analysis and synthesis


def _setenv(monkeypatch, env):
    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                     # the library reads these at every call


def _ragged(design, headset, seed):
    """U x C = 5 x 2: a multiple of D plus three, a multiple of D, one short of it, shorter than the prototype, one sample"""
    M, m, r = design
    D = M >> r
    lens = [max(1, n) for n in (40 * D + 3, 7 * D, 7 * D - 1, m * M - 1, 1)]
    rng = np.random.default_rng(seed)
    x = np.zeros((len(lens), 2, max(lens)), np.float32)
    for u, n in enumerate(lens):
        x[u, 0, :n] = headset[1000 + 37 * u:1000 + 37 * u + n]
        x[u, 1, :n] = rng.standard_normal(n) * 1000
    return x, lens


def _analysis(dsr, cuda, fb, x, lens):
    """dsr_fb_analysis into an output filled with NaN: whatever the kernel leaves unwritten shows"""
    import torch
    U, Cn, N = x.shape
    Tmax = max(1, max(fb.frames(n) for n in lens))
    X = torch.full((U, Cn, Tmax, fb.M // 2 + 1, 2), float("nan"), dtype=torch.float32, device=cuda)
    xd = torch.from_numpy(x).to(cuda); nd = torch.tensor(lens, dtype=torch.int32, device=cuda)
    dsr.check(dsr.load().dsr_fb_analysis(fb.h, dsr._dev(xd), dsr._dev(nd), U, Cn, N, Tmax, dsr._dev(X), dsr.cur_stream()))
    return torch.view_as_complex(X).cpu().numpy()


def _check_analysis(oracle, fb, X, x, lens, h, design, dct, gain):
    """frame counts, zero rows past an utterance's frames, bins 0..M/2 within TOL of the oracle; -> largest error / RMS"""
    M, m, r = design
    F = M // 2 + 1
    worst = 0.0
    for u, n in enumerate(lens):
        for c in range(x.shape[1]):
            ref = oracle.analysis_bank(x[u, c, :n], h, M, m, r, dct, gain)[:, :F]
            T = ref.shape[0]
            assert T == fb.frames(n) == oracle.analysis_num_frames(n, M, m, r, dct)
            assert np.all(X[u, c, T:] == 0), (design, dct, u, c)
            if T == 0:                                # fewer blocks than the look-ahead: no frames at all
                continue
            rms = np.sqrt(np.mean(np.abs(ref) ** 2))
            assert rms > 0
            err = np.abs(X[u, c, :T] - ref).max() / rms
            worst = max(worst, err)
            assert err < TOL, (design, dct, u, c, err)
    return worst


# ------------------------------------------------------------------------------------------- one-shot analysis
_ANALYSIS = ([("q256", d, {}) for d in fb_np.Q256]
             + [("q256-tf32", d, {"DSR_FB_TF": "32"}) for d in ((256, 2, 1), (256, 4, 1))]
             + [("wave", d, {}) for d in fb_np.WAVE] + [("generic", d, {}) for d in fb_np.GENERIC]
             + [("forced-wave", (256, 4, 1), {"DSR_FB_WAVE": "1"}), ("forced-generic", (256, 4, 1), {"DSR_FB_GENERIC": "1"}),
                ("forced-generic", (512, 2, 2), {"DSR_FB_GENERIC": "1"})])


@pytest.mark.gpu
@pytest.mark.parametrize("family,design,env", _ANALYSIS, ids=["%s-M%d-m%d-r%d" % ((f,) + d) for f, d, e in _ANALYSIS])
def test_analysis_design_sweep(dsr, oracle, cuda, headset, monkeypatch, family, design, env):
    """one-shot analysis of a ragged 5 x 2 batch at every delayCompensationType, gainFactor 3 at type 1.  No design the bank accepted and some
    kernel can serve may fail at launch: (1024,4,0) needs 169 984 bytes of LDS in the wave-per-frame kernel at its tile of 32 frames and came
    back as a raw HIP error before the launcher learned to halve the tile.  (128,2,7) and (16,2,4) have D = 1: the wave kernel's paired window
    reads of odd frames are then 4 bytes off their natural alignment (replayed by the hardware, same data)."""
    M, m, r = design
    _setenv(monkeypatch, env)
    h, g = _proto(design)
    x, lens = _ragged(design, headset, seed=M + m + r)
    for dct in (0, 1, 2):
        if not fb_np.dct_defined(m, r, dct):          # the reference's look-ahead m*R/2 - 1 is negative there
            continue
        fb = dsr.FilterBank(h, M, m, r, False, dct, _gain(dct))
        X = _analysis(dsr, cuda, fb, x, lens)
        err = _check_analysis(oracle, fb, X, x, lens, h, design, dct, _gain(dct))
        print("\nanalysis  %-14s M=%-4d m=%d r=%d dct=%d gain=%d  max err / RMS = %.2e" % (family, M, m, r, dct, _gain(dct), err), end="")


# ------------------------------------------------------------------------------------------- one-shot synthesis
_SYNTHESIS = fb_np.DESIGNS + [(256, 4, 1), (512, 2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("design", _SYNTHESIS, ids=["M%d-m%d-r%d" % d for d in _SYNTHESIS])
def test_synthesis_design_sweep(dsr, oracle, cuda, headset, design):
    """k_synthesis<M> at every M: two utterances of different frame counts and a third with fewer frames than the processing delay (no output).
    The input is the oracle's own analysis output cut to complex64 with a spurious imaginary part on the DC and Nyquist bins, which must be
    ignored (modulated.cc:606-607).  The bank keeps TO + R*m - 1 time-domain frames in LDS; the designs whose history does not fit -- by the
    launcher's arithmetic redone in tests/fb_np.py exactly (128,2,7), (1024,4,3) and (2048,1,4) -- are refused with DSR_E_DIMENSION."""
    import torch
    M, m, r = design
    D = M >> r; F = M // 2 + 1
    h, g = _proto(design)
    fits = fb_np.synthesis_lds(M, m, r)[0] <= fb_np.LDS_MAX
    assert fits == (design not in fb_np.SYNTHESIS_REFUSED)
    lens = [max(40 * D + 3, 3 * m * M + 3), max(13 * D, 2 * m * M)]          # long enough for the output to leave the tails of the taps
    for dct in (0, 1, 2):
        if not fb_np.dct_defined(m, r, dct):
            continue
        gain = _gain(dct)
        fb = dsr.FilterBank(g, M, m, r, True, dct, gain)
        Xs = [oracle.analysis_bank(headset[3000:3000 + n], h, M, m, r, dct)[:, :F] for n in lens]
        short = max(fb.pd - 1, 0)
        Xs.append(Xs[0][:short])
        nfr = [x.shape[0] for x in Xs]
        assert nfr[0] != nfr[1] and fb.blocks(nfr[2]) == 0
        Y = np.zeros((3, max(nfr), F), np.complex64)
        for u, x in enumerate(Xs):
            Y[u, :nfr[u]] = x
        Y[:, :, 0] += 0.5j * np.abs(Y[:, :, 0]); Y[:, :, F - 1] -= 0.25j * np.abs(Y[:, :, F - 1])
        nb = max(1, max(fb.blocks(n) for n in nfr))
        y = torch.full((3, nb * D), float("nan"), dtype=torch.float32, device=cuda)
        Yd = torch.view_as_real(torch.from_numpy(Y).to(cuda)); nd = torch.tensor(nfr, dtype=torch.int32, device=cuda)
        status = dsr.load().dsr_fb_synthesis(fb.h, dsr._dev(Yd), dsr._dev(nd), 3, Y.shape[1], nb * D, dsr._dev(y), dsr.cur_stream())
        if not fits:
            assert status == dsr.E_DIMENSION, (design, status)
            print("\nsynthesis M=%-4d m=%d r=%d dct=%d refused: %d bytes of LDS" % (M, m, r, dct, fb_np.synthesis_lds(M, m, r)[0]), end="")
            continue
        dsr.check(status)
        y = y.cpu().numpy()
        worst = 0.0
        for u in range(3):
            Yfull = np.zeros((nfr[u], M), np.complex128)
            Yfull[:, :F] = Y[u, :nfr[u]].astype(np.complex128)
            Yfull[:, F:] = np.conj(Yfull[:, 1:M // 2][:, ::-1])
            ref = oracle.synthesis_bank(Yfull, g, M, m, r, dct, gain)
            assert len(ref) == fb.blocks(nfr[u]) * D
            assert np.all(y[u, len(ref):] == 0), (design, dct, u)
            if u == 2:
                assert len(ref) == 0
                continue
            rms = np.sqrt(np.mean(ref.astype(np.float64) ** 2))
            assert rms > 1e-6 * np.sqrt(np.mean(headset[3000:3000 + lens[u]].astype(np.float64) ** 2))      # not the numerical zero of the taps' tails
            err = np.abs(y[u, :len(ref)] - ref).max() / rms
            worst = max(worst, err)
            assert err < TOL, (design, dct, u, err)
        print("\nsynthesis M=%-4d m=%d r=%d dct=%d gain=%d  max err / RMS = %.2e" % (M, m, r, dct, gain, worst), end="")


@pytest.mark.gpu
def test_clean_refusals(dsr, cuda):
    """what no kernel can serve is refused on the host with DSR_E_DIMENSION before anything is launched"""
    import torch
    for M, m, r in ((8, 2, 1), (4096, 2, 1), (384, 2, 1), (256, 0, 1), (16, 2, 5)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.FilterBank(np.ones(M * m), M, m, r, False, 0)
        assert e.value.status == dsr.E_DIMENSION, (M, m, r)
    g = synth.fb_prototype(2048, 4, 3, seed=1)[1]
    with pytest.raises(dsr.DsrError) as e:
        dsr.FilterBank(g, 2048, 4, 3, True, 0).synthesis_run(torch.zeros((1, 40, 1025), dtype=torch.complex64, device=cuda))
    assert e.value.status == dsr.E_DIMENSION and "LDS" in str(e.value)
    h = synth.fb_prototype(2048, 8, 0, seed=1)[0]
    with pytest.raises(dsr.DsrError) as e:
        dsr.FilterBank(h, 2048, 8, 0, False, 0).analysis(torch.zeros((1, 1, 4096), device=cuda))
    assert e.value.status == dsr.E_DIMENSION and "LDS" in str(e.value)


# ------------------------------------------------------------------------------------------- the three analysis kernels on one input
@pytest.mark.gpu
@pytest.mark.parametrize("design", [(256, 2, 1), (256, 4, 1), (512, 2, 2)], ids=lambda d: "M%d-m%d-r%d" % d)
def test_three_analysis_kernels_on_one_input(dsr, oracle, cuda, headset, monkeypatch, design):
    """default dispatch, DSR_FB_WAVE and DSR_FB_GENERIC on one ragged batch: each within TOL of the oracle, identical shapes and zero rows.
    The pairwise difference is printed, not bounded: the FFT factorizations differ."""
    M, m, r = design
    h, g = _proto(design)
    x, lens = _ragged(design, headset, seed=9)
    out = {}
    for name, env in (("default", {}), ("wave", {"DSR_FB_WAVE": "1"}), ("generic", {"DSR_FB_GENERIC": "1"})):
        _setenv(monkeypatch, env)
        fb = dsr.FilterBank(h, M, m, r, False, 2, 3)
        out[name] = _analysis(dsr, cuda, fb, x, lens)
        _check_analysis(oracle, fb, out[name], x, lens, h, design, 2, 3)
    rms = np.sqrt(np.mean(np.abs(out["default"][0]) ** 2))
    for a, b in (("default", "wave"), ("default", "generic"), ("wave", "generic")):
        assert out[a].shape == out[b].shape
        assert np.array_equal(np.all(out[a] == 0, axis=-1), np.all(out[b] == 0, axis=-1))
        print("\nkernels   M=%-4d m=%d r=%d  %s vs %s: max diff / RMS = %.2e" % (M, m, r, a, b, np.abs(out[a] - out[b]).max() / rms), end="")


# ------------------------------------------------------------------------------------------- fused analysis + beamformer
def _beamformer(dsr, M, Cn, mode):
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(np.deg2rad(30.0)), np.float32(np.pi / 2), mp)
    bf = dsr.Beamformer(M, Cn)
    bf.calcArrayManifoldVectors(16000.0, delays)
    bf.setDiffuseNoiseModel(mp, 16000.0, 343740.0); bf.divideAllNonDiagonalElements(0.01); bf.calcMVDRWeights(16000.0, 1e-8)
    bf.select(mode)
    return bf


_FUSED = ([((256, 2, 1), Cn, mode, {}) for Cn in (1, 5, 16) for mode in ("ds", "mvdr")]
          + [((256, 4, 1), 5, "mvdr", {}), ((256, 4, 1), 8, "mvdr", {"DSR_FB_FUSED_WAVES": "8"}), ((256, 2, 1), 8, "ds", {"DSR_FB_FUSED_WAVES": "8"}),
             ((256, 2, 1), 16, "mvdr", {"DSR_FB_FUSED_WAVES": "8"})])


@pytest.mark.gpu
@pytest.mark.parametrize("design,Cn,mode,env", _FUSED, ids=["M%d-m%d-r%d-C%d-%s-%s" % (d + (c, mo, "nw8" if e else "nw4")) for d, c, mo, e in _FUSED])
def test_fused_analysis_beamform_designs(dsr, oracle, cuda, monkeypatch, design, Cn, mode, env):
    """the construction of test_analysis_beamform_in_one_pass at m = 2 (k_analysis_bf_q256<2, *>) and with 8 waves per workgroup: 5e-6 of the
    RMS against the two-step device path, 4e-5 against the oracle's analysis bank + beamformer"""
    import torch
    M, m, r = design
    _setenv(monkeypatch, env)
    h, g = _proto(design)
    bf = _beamformer(dsr, M, Cn, mode)
    dct = (Cn + len(mode)) % 3
    lens = [20000, 12345, 5000, 777, 1, 16384]
    U, N = len(lens), max(lens)
    x = np.zeros((U, Cn, N), np.float32)
    for u, n in enumerate(lens):
        x[u, :, :n] = synth.array_signal(n, Cn, seed=60 + u) * (1000.0 if u % 2 else 1.0)
    fb = dsr.FilterBank(h, M, m, r, False, dct, _gain(dct))
    assert fb.analysis_beamform_supported(bf)
    xd = torch.from_numpy(x).to(cuda); nd = torch.tensor(lens, dtype=torch.int32, device=cuda)
    Y = fb.analysis_beamform(bf, xd, nd).cpu().numpy()
    Y2 = bf.apply(fb.analysis(xd, nd)).cpu().numpy()
    W = bf.get(4)
    assert Y.shape == Y2.shape
    worst = [0.0, 0.0]
    for u, n in enumerate(lens):
        T = fb.frames(n)
        assert np.all(Y[u, T:] == 0)
        if T == 0:
            continue
        rms = np.sqrt(np.mean(np.abs(Y2[u, :T]) ** 2)) + 1e-30
        e2 = np.abs(Y[u, :T] - Y2[u, :T]).max() / rms
        assert e2 < 5e-6, (u, e2)
        Xc = np.stack([oracle.analysis_bank(x[u, c, :n], h, M, m, r, dct, _gain(dct)) for c in range(Cn)])
        ref = oracle.beamform_apply(Xc, W)[:, :M // 2 + 1]
        eo = np.abs(Y[u, :T] - ref).max() / (np.sqrt(np.mean(np.abs(ref) ** 2)) + 1e-30)
        assert eo < 4e-5, (u, eo)
        worst = [max(worst[0], e2), max(worst[1], eo)]
    print("\nfused     M=%-4d m=%d C=%-2d %-4s dct=%d %s  vs two steps %.2e  vs oracle %.2e" % (M, m, Cn, mode, dct, "8 waves" if env else "4 waves", worst[0], worst[1]), end="")


@pytest.mark.gpu
@pytest.mark.parametrize("var", ["DSR_FB_GENERIC", "DSR_FB_WAVE", "DSR_FB_NOFUSE"])
def test_fused_pipe_falls_back_to_the_two_steps(dsr, cuda, monkeypatch, var):
    """under each of the path switches the fused kernel is not offered, and a Pipe(fused=True) runs analysis and beamformer as two kernels
    (include/dsr.h, dsr_pipe_set_fused): intermediate 0 exists and every intermediate equals the unfused run bit for bit"""
    import torch
    M, m, r = 256, 4, 1
    h, g = _proto((M, m, r))
    Cn, lens = 8, [4000, 2500]
    x = np.zeros((2, Cn, max(lens)), np.float32)
    for u, n in enumerate(lens):
        x[u, :, :n] = synth.array_signal(n, Cn, seed=80 + u)
    ana = dsr.FilterBank(h, M, m, r, False, 0); syn = dsr.FilterBank(g, M, m, r, True, 0)
    bf = _beamformer(dsr, M, Cn, "mvdr")
    lda = (np.random.default_rng(1234).standard_normal((39, 195)) / np.sqrt(195)).astype(np.float32)
    gm = dsr.Gmm(**synth.gmm_model(32, 16, 39, seed=12))
    arcs, fin = synth.random_wfst(1000, 32, seed=21)
    gd = dsr.Wfst()
    for a in arcs:
        gd.add_arc(*a)
    for s, c in fin:
        gd.add_final(s, c)
    xd = torch.from_numpy(x).to(cuda); nd = torch.tensor(lens, dtype=torch.int32, device=cuda)

    def run(fused):
        mf = dsr.Mfcc(lda=lda)
        dec = dsr.Decoder(beam=60.0, lmScale=12.0, maxActive=16384, streams=4); dec.set(gd)
        pipe = dsr.Pipe(ana, syn, bf, mf, gm, dec, gmmMode=0, fused=fused)
        res, _, _ = pipe.run(xd, nd, lens, maxPath=1024)
        assert all(rr.status == 0 for rr in res)
        return [pipe.intermediate_host(k).copy() for k in range(5)], [rr.score for rr in res]

    _setenv(monkeypatch, {})
    assert ana.analysis_beamform_supported(bf)
    _setenv(monkeypatch, {var: "1"})
    assert not ana.analysis_beamform_supported(bf)
    a, sa = run(True)
    b, sb = run(False)
    assert a[0].size > 0 and np.any(a[0] != 0)
    for k in range(5):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (var, k)
    assert sa == sb


# ------------------------------------------------------------------------------------------- block-wise mode on short and uneven blocks
def _analysis_block_lists(design, dct):
    """samples per call for two streams: blocks of 1, 1, 2, 1, 1, 3, 1, ... times D -- every one shorter than the m*M - D samples of carried
    history, so every history update splices old history and new block -- until the stream is at least 3 m R blocks long; the last block is
    ragged; in one call the streams hold 3 D and 1 D samples.  delayCompensationType 2: the first block holds the look-ahead of m R / 2 - 1
    blocks, the documented minimum (include/dsr.h), still shorter than the history."""
    M, m, r = design
    D = M >> r; R = 1 << r
    la = fb_np.delays(m, r, dct, False)[1]
    units = [la] if la > 0 else []
    pat = [1, 1, 2, 1, 1, 3, 1]
    while sum(units) < 3 * m * R:
        units.append(pat[(len(units) - (1 if la > 0 else 0)) % len(pat)])
    assert max(units) * D < m * M - D
    a = [k * D for k in units] + [2 * D - 5]
    b = list(a)
    i = max(j for j, k in enumerate(units) if k == 3)
    b[i] = D
    b[-1] = D + 3
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("dct", [0, 2])
@pytest.mark.parametrize("design", [(256, 4, 1), (1024, 2, 2), (64, 3, 2)], ids=lambda d: "M%d-m%d-r%d" % d)
def test_blockwise_short_and_uneven_blocks(dsr, oracle, cuda, design, dct):
    """FilterBankState on blocks shorter than the carried history, one design per kernel family (quarter-wave, wave-per-frame, generic): the
    concatenated block outputs are the one-shot oracle over each whole stream within TOL, and the frame and block counts add up.
    Synthesis: frames per call [pd + R m, 1, 2, 1, 5] -- the first call exactly the documented minimum, later ones shorter than the R m - 1
    frames of history -- and in one call 4 and 1 frames for the two streams."""
    import torch
    M, m, r = design
    D = M >> r; R = 1 << r; F = M // 2 + 1
    h, g = _proto(design)
    L = dsr.load()
    ana = dsr.FilterBank(h, M, m, r, False, dct); syn = dsr.FilterBank(g, M, m, r, True, dct)
    la = ana.laN
    assert la == fb_np.delays(m, r, dct, False)[1]
    lists = _analysis_block_lists(design, dct)
    rng = np.random.default_rng(11 + M + dct)
    xs = [(rng.standard_normal(sum(l)) * 1000).astype(np.float32) for l in lists]
    ncall = len(lists[0])

    def stream_analysis(sa, which):
        outs = [[] for _ in which]; off = [0] * len(which)
        for i in range(ncall):
            ns = [lists[w][i] for w in which]
            blk = np.zeros((len(which), 1, max(ns)), np.float32)
            for j, w in enumerate(which):
                blk[j, 0, :ns[j]] = xs[w][off[j]:off[j] + ns[j]]; off[j] += ns[j]
            last = i == ncall - 1
            T = [L.dsr_fb_analysis_block_frames(ana.h, sa.h, n, int(last)) for n in ns]           # asked before the call
            X = sa.analysis_block(torch.from_numpy(blk).to(cuda), nsamp=ns, last=last).cpu().numpy()
            for j in range(len(which)):
                assert np.all(X[j, 0, T[j]:] == 0)
                outs[j].append(X[j, 0, :T[j]])
        return [np.concatenate(o) for o in outs]

    sa = dsr.FilterBankState(ana, 2, 1)
    Xb = stream_analysis(sa, (0, 1))
    worst = 0.0
    Xo = []
    for u in range(2):
        ref = oracle.analysis_bank(xs[u], h, M, m, r, dct)
        Xo.append(ref)
        assert Xb[u].shape[0] == ref.shape[0] == ana.frames(len(xs[u]))                           # the blocks' frames add up to the stream's
        err = np.abs(Xb[u] - ref[:, :F]).max() / np.sqrt(np.mean(np.abs(ref[:, :F]) ** 2))
        worst = max(worst, err)
        assert err < TOL, (design, dct, u, err)
    # after reset() the same state gives what a fresh state gives, bit for bit
    sa.reset()
    again = stream_analysis(sa, (1, 0))
    fresh = stream_analysis(dsr.FilterBankState(ana, 2, 1), (1, 0))
    for p, q in zip(again, fresh):
        assert np.array_equal(p.view(np.float32), q.view(np.float32))
    assert np.array_equal(again[0].view(np.float32), Xb[1].view(np.float32))
    if la > 0:                                       # a first block that cannot hold the look-ahead is refused, not processed late
        with pytest.raises(dsr.DsrError) as e:
            dsr.FilterBankState(ana, 1, 1).analysis_block(torch.zeros((1, 1, la * D - 1), device=cuda))
        assert e.value.status == dsr.E_DIMENSION

    # ---- synthesis
    first = syn.pd + R * m
    fa = [first, 1, 2, 1, 5, 4, 2]
    fbb = [first, 1, 2, 1, 5, 1, 2]
    assert max(fa[1:]) < R * m - 1
    Ys = [Xo[0][:sum(fa), :F].astype(np.complex64), Xo[1][:sum(fbb), :F].astype(np.complex64)]
    assert Ys[0].shape[0] == sum(fa) and Ys[1].shape[0] == sum(fbb)
    flists = (fa, fbb)

    def stream_synthesis(ss, which):
        outs = [[] for _ in which]; off = [0] * len(which)
        for i in range(len(fa)):
            nf = [flists[w][i] for w in which]
            blk = np.zeros((len(which), max(nf), F), np.complex64)
            for j, w in enumerate(which):
                blk[j, :nf[j]] = Ys[w][off[j]:off[j] + nf[j]]; off[j] += nf[j]
            nb = [L.dsr_fb_synthesis_block_blocks(syn.h, ss.h, n) for n in nf]
            y = ss.synthesis_block(torch.from_numpy(blk).to(cuda), nframes=nf).cpu().numpy()
            for j in range(len(which)):
                assert np.all(y[j, nb[j] * D:] == 0)
                outs[j].append(y[j, :nb[j] * D])
        return [np.concatenate(o) for o in outs]

    ss = dsr.FilterBankState(syn, 2)
    yb = stream_synthesis(ss, (0, 1))
    worst_s = 0.0
    for u in range(2):
        Yfull = np.zeros((Ys[u].shape[0], M), np.complex128)
        Yfull[:, :F] = Ys[u]; Yfull[:, F:] = np.conj(Yfull[:, 1:M // 2][:, ::-1])
        ref = oracle.synthesis_bank(Yfull, g, M, m, r, dct)
        assert len(yb[u]) == len(ref) == syn.blocks(Ys[u].shape[0]) * D
        err = np.abs(yb[u] - ref).max() / np.sqrt(np.mean(ref.astype(np.float64) ** 2))
        worst_s = max(worst_s, err)
        assert err < TOL, (design, dct, u, err)
    ss.reset()
    again = stream_synthesis(ss, (1, 0))
    fresh = stream_synthesis(dsr.FilterBankState(syn, 2), (1, 0))
    for p, q in zip(again, fresh):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
    assert np.array_equal(again[0].view(np.uint32), yb[1].view(np.uint32))
    # a first block one frame below the minimum
    with pytest.raises(dsr.DsrError) as e:
        dsr.FilterBankState(syn, 1).synthesis_block(torch.zeros((1, first - 1, F), dtype=torch.complex64, device=cuda))
    assert e.value.status == dsr.E_DIMENSION
    print("\nblockwise M=%-4d m=%d r=%d dct=%d  %d analysis calls, %d synthesis calls  max err / RMS = %.2e / %.2e"
          % (M, m, r, dct, ncall, len(fa), worst, worst_s), end="")
