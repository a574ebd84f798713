"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs.

Tolerances: filterbank/beamformer complex64 vs the reference's complex128 -- relative 1e-5 of
the frame RMS; MFCC -- abs 1e-4; GMM nearest-Gaussian scores and every WFST index/score -- bit exact.
"""
import os

import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu


def _rel_rms(a, b, axis=-1):
    num = np.sqrt(np.mean(np.abs(a - b) ** 2, axis=axis))
    den = np.sqrt(np.mean(np.abs(b) ** 2, axis=axis)) + 1e-30
    return num / den


# ------------------------------------------------------------------------------------------- filter banks
@pytest.mark.parametrize("pname,dct", [("M256-m4-r1", 0), ("M256-m4-r1", 2), ("M512-m2-r2", 0), ("M512-m2-r2", 1),
                                       ("M512-m2-r3", 2)])
def test_analysis_bank(dsr, oracle, cuda, headset, protos, pname, dct):
    import torch
    M, m, r, h, g = protos[pname]
    rng = np.random.default_rng(5)
    lens = [20000, 12345, 777, 1]                     # ragged, incl. shorter than one prototype / one sample
    U, Cn, N = len(lens), 2, max(lens)
    x = np.zeros((U, Cn, N), np.float32)
    for u, n in enumerate(lens):
        x[u, 0, :n] = headset[1000:1000 + n]
        x[u, 1, :n] = rng.standard_normal(n) * 1000
    fb = dsr.FilterBank(h, M, m, r, False, dct)
    X = fb.analysis(torch.from_numpy(x).to(cuda), torch.tensor(lens, dtype=torch.int32, device=cuda)).cpu().numpy()
    for u, n in enumerate(lens):
        for c in range(Cn):
            ref = oracle.analysis_bank(x[u, c, :n], h, M, m, r, dct)
            T = ref.shape[0]
            assert T == fb.frames(n)
            assert np.all(X[u, c, T:] == 0)
            if T == 0:                                # fewer blocks than the look-ahead: no frames at all
                continue
            got = X[u, c, :T]
            scale = np.sqrt(np.mean(np.abs(ref[:, :M // 2 + 1]) ** 2)) + 1e-30
            err = np.abs(got - ref[:, :M // 2 + 1]).max() / scale
            assert err < 2e-5, (u, c, err)
            assert np.all(X[u, c, T:] == 0)


@pytest.mark.parametrize("pname,dct", [("M256-m4-r1", 0), ("M256-m4-r1", 2), ("M512-m2-r2", 1), ("M512-m2-r3", 0)])
def test_synthesis_bank(dsr, oracle, cuda, headset, protos, pname, dct):
    import torch
    M, m, r, h, g = protos[pname]
    lens = [16000, 5000]
    Xs = [oracle.analysis_bank(headset[3000:3000 + n], h, M, m, r, dct) for n in lens]
    Tmax = max(x.shape[0] for x in Xs)
    Y = np.zeros((len(lens), Tmax, M // 2 + 1), np.complex64)
    for u, x in enumerate(Xs):
        Y[u, :x.shape[0]] = x[:, :M // 2 + 1]
        Y[u, :, 0] += 0.5j * np.abs(Y[u, :, 0])       # imaginary DC/Nyquist parts must be ignored (modulated.cc:606-607)
    fb = dsr.FilterBank(g, M, m, r, True, dct)
    nfr = torch.tensor([x.shape[0] for x in Xs], dtype=torch.int32, device=cuda)
    y = fb.synthesis_run(torch.from_numpy(Y).to(cuda), nfr).cpu().numpy()
    for u, x in enumerate(Xs):
        Yfull = np.zeros((x.shape[0], M), np.complex128)
        Yfull[:, :M // 2 + 1] = Y[u, :x.shape[0]].astype(np.complex128)
        Yfull[:, M // 2 + 1:] = np.conj(Yfull[:, 1:M // 2][:, ::-1])
        ref = oracle.synthesis_bank(Yfull, g, M, m, r, dct)
        assert len(ref) == fb.blocks(x.shape[0]) * (M >> r)
        got = y[u, :len(ref)]
        assert np.abs(got - ref).max() / (np.sqrt(np.mean(ref ** 2)) + 1e-30) < 2e-5
        assert np.all(y[u, len(ref):] == 0)


def test_analysis_many_rows(dsr, cuda, protos):
    """More (utterance, channel) rows than compute units: several workgroups share a CU and its LDS, their waves interleave.
    The result of every row must be the one it has alone (regression: a missing barrier between the window slide and the
    store of the prefetched samples only showed with co-resident workgroups)."""
    import torch
    M, m, r, h, g = protos["M256-m4-r1"]
    torch.manual_seed(3)
    x = torch.randn((80, 8, 24000), device=cuda) * 3000.0               # 640 rows
    ana = dsr.FilterBank(h, 256, 4, 1, False, 0)
    X = ana.analysis(x)
    for u in (0, 31, 32, 33, 64, 79):
        Xs = ana.analysis(x[u:u + 1].contiguous())
        assert torch.equal(X[u], Xs[0]), u


def test_filterbank_roundtrip_full_size(dsr, cuda, headset, protos):
    """Size-independent property at BASELINE scale: analysis -> synthesis with the reference's own Nyquist(M)
    prototypes and delayCompensationType=2 reconstructs the input (x D, zero delay)."""
    import torch
    M, m, r, h, g = protos["M512-m2-r3"]
    D = M >> r
    n = (len(headset) // D) * D
    x = torch.from_numpy(np.tile(headset[:n], (4, 2, 1))).to(cuda)
    a = dsr.FilterBank(h, M, m, r, False, 2); s = dsr.FilterBank(g, M, m, r, True, 2)
    X = a.analysis(x)
    y = s.synthesis_run(X[:, 0].contiguous()) * D
    e = (y[:, 2000:n - 2000] - x[:, 0, 2000:n - 2000]).pow(2).mean().sqrt() / x[:, 0].pow(2).mean().sqrt()
    assert e.item() < 1e-5


# ------------------------------------------------------------------------------------------- beamformer
def _mvdr_setup(dsr, oracle, M=256, Cn=8):
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(np.deg2rad(30.0)), np.float32(np.pi / 2), mp)
    d_ref = oracle.calc_delays_polar2(np.float32(np.deg2rad(30.0)), np.float32(np.pi / 2), mp)
    assert np.array_equal(delays, d_ref)
    bf = dsr.Beamformer(M, Cn)
    bf.calcArrayManifoldVectors(16000.0, delays)
    bf.setDiffuseNoiseModel(mp, 16000.0, 343740.0)
    bf.divideAllNonDiagonalElements(0.01)
    bf.calcMVDRWeights(16000.0, 1e-8)
    wq = oracle.calc_mainlobe(16000.0, delays, M)
    R = oracle.diffuse_noise_model(mp, M, 16000.0, 343740.0, mu=0.01)
    w = oracle.mvdr_weights(wq, R, 1e-8)
    return bf, delays, wq, R, w


def test_beamformer_weights(dsr, oracle, cuda):
    bf, delays, wq, R, w = _mvdr_setup(dsr, oracle)
    assert np.abs(bf.get(0) - wq).max() < 1e-15
    assert np.abs(bf.get(2) - R).max() < 1e-15
    got = bf.get(1)
    # both sides restate LINPACK csvdc bit for bit (pinned by tests/golden/linpack_csvdc.npz, the reference's own routine): the fp32 SVD no
    # longer separates them; what is left is fp64 summation order (round 1: two different Jacobi SVDs, 2e-3)
    assert np.abs(got - w).max() / np.abs(w).max() < 1e-12
    assert np.all(got[0] == 1.0)                       # DC bin weights are all ones (beamformer.cc:2413-2415)
    # distortionless response d^H w = 1/C ... w^H d = 1/C for f>0
    resp = np.einsum("fc,fc->f", np.conj(got[1:]), wq[1:129])
    assert np.abs(resp - 1.0 / 8).max() < 1e-4


@pytest.mark.parametrize("mode,Cn,dct", [("mvdr", 8, 0), ("ds", 8, 2), ("gsc", 8, 0), ("mvdr", 3, 1), ("ds", 16, 0)])
def test_analysis_beamform_in_one_pass(dsr, oracle, cuda, headset, protos, mode, Cn, dct):
    """dsr_fb_analysis_beamform (the pipe's fused front end: the channel snapshots never reach memory) against the two-step product path on the same
    input (same arithmetic per channel, same channel order: 5e-6 of the RMS) and against the oracle's analysis bank + beamformer (the tolerance of
    the two steps); ragged batch incl. an utterance without frames, rows past an utterance's end zero, a batch of many tiles."""
    import torch
    M, m, r, h, g = protos["M256-m4-r1"]
    bf, delays, wq, R, w = _mvdr_setup(dsr, oracle, M, Cn)
    rng = np.random.default_rng(17)
    if mode == "gsc":
        bf.calcGSCWeights(16000.0, delays)
        wa = (rng.standard_normal((M, Cn - 1)) + 1j * rng.standard_normal((M, Cn - 1))) * 0.05
        for f in range(M):
            bf.setActiveWeights_f(f, np.stack([wa[f].real, wa[f].imag], -1).reshape(-1))
    bf.select(mode)
    lens = [20000, 12345, 5000, 777, 1, 16384]
    U, N = len(lens), max(lens)
    x = np.zeros((U, Cn, N), np.float32)
    for u, n in enumerate(lens):
        x[u, :, :n] = synth.array_signal(n, Cn, seed=40 + u) * (1000.0 if u % 2 else 1.0)
    fb = dsr.FilterBank(h, M, m, r, False, dct)
    assert fb.analysis_beamform_supported(bf)
    xd = torch.from_numpy(x).to(cuda); nd = torch.tensor(lens, dtype=torch.int32, device=cuda)
    Y = fb.analysis_beamform(bf, xd, nd).cpu().numpy()
    Y2 = bf.apply(fb.analysis(xd, nd)).cpu().numpy()
    W = bf.get(4)
    assert Y.shape == Y2.shape
    for u, n in enumerate(lens):
        T = fb.frames(n)
        assert np.all(Y[u, T:] == 0)
        if T == 0:
            continue
        rms = np.sqrt(np.mean(np.abs(Y2[u, :T]) ** 2)) + 1e-30
        assert np.abs(Y[u, :T] - Y2[u, :T]).max() / rms < 5e-6, (u, np.abs(Y[u, :T] - Y2[u, :T]).max() / rms)
        Xc = np.stack([oracle.analysis_bank(x[u, c, :n], h, M, m, r, dct) for c in range(Cn)])
        ref = oracle.beamform_apply(Xc, W)[:, :M // 2 + 1]
        assert np.abs(Y[u, :T] - ref).max() / (np.sqrt(np.mean(np.abs(ref) ** 2)) + 1e-30) < 4e-5, u
    # not for an adapting beamformer, nor for another bank
    M5, m5, r5, h5, g5 = protos["M512-m2-r2"]
    assert not dsr.FilterBank(h5, M5, m5, r5, False, 0).analysis_beamform_supported(bf)


@pytest.mark.parametrize("mode", ["ds", "mvdr", "gsc", "gsc_norm"])
def test_beamformer_apply(dsr, oracle, cuda, mode):
    import torch
    M, Cn, T = 256, 8, 40
    bf, delays, wq, R, w = _mvdr_setup(dsr, oracle, M, Cn)
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((2, Cn, T, M // 2 + 1)) + 1j * rng.standard_normal((2, Cn, T, M // 2 + 1))).astype(np.complex64)
    if mode.startswith("gsc"):
        bf.calcGSCWeights(16000.0, delays)
        wa = (rng.standard_normal((M, Cn - 1)) + 1j * rng.standard_normal((M, Cn - 1))) * 0.05
        for f in range(M):
            bf.setActiveWeights_f(f, np.stack([wa[f].real, wa[f].imag], -1).reshape(-1))
    bf.select(mode)
    Y = bf.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()
    W = bf.get(4)                                       # weights in use (host double)
    for u in range(2):
        Xfull = np.zeros((Cn, T, M), np.complex128); Xfull[:, :, :M // 2 + 1] = X[u]
        if mode == "ds":
            ref = oracle.beamform_apply(Xfull, wq[:M // 2 + 1])
        elif mode == "mvdr":
            ref = oracle.beamform_apply(Xfull, W)       # same weights: isolates the apply kernel
        else:
            B = np.stack([oracle.blocking_matrix(wq[f])[0] for f in range(M // 2 + 1)])
            ref = oracle.gsc_apply(Xfull, wq[:M // 2 + 1], B, wa[:M // 2 + 1], normalize=(mode == "gsc_norm"))
        err = np.abs(Y[u] - ref[:, :M // 2 + 1]).max() / np.sqrt(np.mean(np.abs(ref) ** 2))
        assert err < 2e-5, err


def test_beamformer_apply_weights_above_64k_of_lds(dsr, oracle, cuda):
    """k_bf_apply keeps the weight image in dynamic LDS: 129 bins x 64 channels x 8 bytes = 66 048 bytes, above the 64 KiB a kernel gets
    without asking; 513 x 64 x 8 = 262 656 bytes are more than a workgroup can have and are refused"""
    import torch
    M, Cn, T = 256, 64, 8
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(np.deg2rad(30.0)), np.float32(np.pi / 2), mp)
    bf = dsr.Beamformer(M, Cn); bf.calcArrayManifoldVectors(16000.0, delays); bf.select("ds")
    wq = oracle.calc_mainlobe(16000.0, delays, M)
    rng = np.random.default_rng(5)
    X = (rng.standard_normal((2, Cn, T, M // 2 + 1)) + 1j * rng.standard_normal((2, Cn, T, M // 2 + 1))).astype(np.complex64)
    Y = bf.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()
    for u in range(2):
        Xfull = np.zeros((Cn, T, M), np.complex128); Xfull[:, :, :M // 2 + 1] = X[u]
        ref = oracle.beamform_apply(Xfull, wq[:M // 2 + 1])
        err = np.abs(Y[u] - ref[:, :M // 2 + 1]).max() / np.sqrt(np.mean(np.abs(ref) ** 2))
        assert err < 2e-5, err
    big = dsr.Beamformer(1024, Cn); big.calcArrayManifoldVectors(16000.0, delays); big.select("ds")
    with pytest.raises(dsr.DsrError) as e:
        big.apply(torch.zeros((1, Cn, 1, 513), dtype=torch.complex64, device=cuda))
    assert e.value.status == dsr.E_DIMENSION and "262656 bytes of LDS" in str(e.value)


# ------------------------------------------------------------------------------------------- MFCC
@pytest.mark.parametrize("stage,tol", [(4, 1e-5), (3, 1e-5), (1, 1e-4), (2, 1e-4), (0, 1e-4)])
def test_mfcc_chain(dsr, oracle, cuda, headset, stage, tol):
    import torch
    rng = np.random.default_rng(1234)
    lda = (rng.standard_normal((39, 195)) / np.sqrt(195)).astype(np.float32)
    lens = [len(headset), 16000, 4000, 1300]
    y = np.zeros((len(lens), max(lens)), np.float32)
    for u, n in enumerate(lens):
        y[u, :n] = headset[:n]
    mf = dsr.Mfcc(lda=lda)
    out = mf.run(torch.from_numpy(y).to(cuda), torch.tensor(lens, dtype=torch.int32, device=cuda), stage=stage).cpu().numpy()
    cfg = oracle.mfcc_cfg(lda=lda)
    for u, n in enumerate(lens):
        ref = oracle.mfcc_chain(y[u, :n], cfg, stage=stage)
        T = ref.shape[0]
        if stage == 0:
            assert T == mf.frames(n)
        got = out[u, :T]
        if stage == 4:   # power spectrum: relative
            assert (np.abs(got - ref) / (np.abs(ref) + 1e-3 * ref.max())).max() < tol
        else:
            assert np.abs(got - ref).max() < tol, (u, np.abs(got - ref).max())
        assert np.all(out[u, T:] == 0)


@pytest.mark.parametrize("kw", [dict(vtlnRatio=1.1, vtlnEdge=0.8), dict(vtlnRatio=0.9, vtlnEdge=0.8, vtlnVersion=2),
                                dict(melVersion=2), dict(dctType=0), dict(dctType=2), dict(cmnMode=2, devNormFactor=3.0),
                                dict(cmnMode=1, devNormFactor=3.0), dict(padZeros=1), dict(delta=1), dict(delta=5), dict(sphinxFlooring=1)])
def test_mfcc_variants(dsr, oracle, cuda, headset, kw):
    import torch
    n = 24000
    y = headset[5000:5000 + n].copy()
    if kw.get("sphinxFlooring"):
        y[3000:9000] = 0.0                                          # digital silence: mel energies below the 1e-5 floor (feature.cc:2411-2418)
    mf = dsr.Mfcc(**kw)
    stage = 2 if "cmnMode" in kw else 0
    out = mf.run(torch.from_numpy(y[None]).to(cuda), stage=stage).cpu().numpy()[0]
    okw = {k: v for k, v in kw.items() if k != "cmnMode"}
    cfg = oracle.mfcc_cfg(**okw)
    if kw.get("cmnMode") == 2:
        cep = oracle.mfcc_chain(y, cfg, stage=1)
        ref = oracle.cmn_runon(cep, kw["devNormFactor"])
    else:
        ref = oracle.mfcc_chain(y, cfg, stage=stage)
    T = ref.shape[0]
    assert np.abs(out[:T] - ref).max() < 1e-4


# ------------------------------------------------------------------------------------------- GMM
@pytest.mark.parametrize("K,R,D,mode", [(8, 16, 39, 0), (256, 16, 39, 0), (5, 7, 13, 0), (3, 256, 39, 0), (64, 4, 39, 0),
                                        (8, 16, 39, 1), (4, 1, 39, 1)])
def test_gmm_scores(dsr, oracle, cuda, K, R, D, mode):
    import torch
    m = synth.gmm_model(K, R, D, seed=12)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((1000, D)).astype(np.float32)
    x[:10] *= 30.0                                       # far-away frames
    gm = dsr.Gmm(**m)
    sc, am = gm.score(torch.from_numpy(x).to(cuda), mode=mode)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    if mode == 0:
        ref, arg = oracle.gmm_score_opt(cb, m["val"], x)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), ref.view(np.uint32))      # bit exact
        assert np.array_equal(am.cpu().numpy().astype(np.int32), arg)
    else:
        ref = oracle.gmm_score_all(cb, m["val"], x)
        assert np.abs(sc.cpu().numpy() - ref).max() / np.abs(ref).max() < 1e-6


def test_gmm_file_roundtrip(dsr, oracle, cuda, tmp_path):
    m = synth.gmm_model(6, 16, 39, seed=3)
    gm = dsr.Gmm(**m)
    cbf, dsf = str(tmp_path / "cb.bin"), str(tmp_path / "ds.bin")
    gm.save(cbf, dsf)
    cb, names = oracle.cbset_load(cbf)                   # the oracle's reader accepts our writer byte for byte
    assert np.array_equal(cb.mean, m["mean"]) and np.array_equal(cb.ivar, m["ivar"]) and np.array_equal(cb.det, m["det"])
    gm2 = dsr.Gmm(files=(cbf, dsf))
    assert gm2.K == 6 and gm2.D == 39


# ------------------------------------------------------------------------------------------- WFST + Viterbi
def _graphs(dsr, oracle, arcs, fin):
    go, gd = oracle.Wfst(), dsr.Wfst()
    for a in arcs:
        go.add_arc(*a); gd.add_arc(*a)
    for s, c in fin:
        go.add_final(s, c); gd.add_final(s, c)
    return go, gd


def _check_decode(ro, rd):
    assert rd["status"] == 0
    assert rd["frames"] == ro["frames"]
    assert rd["reachedFinal"] == ro["reachedFinal"]
    assert np.float32(rd["ac"]).view(np.uint32) == np.float32(ro["ac"]).view(np.uint32)
    assert np.float32(rd["lm"]).view(np.uint32) == np.float32(ro["lm"]).view(np.uint32)
    assert rd["score"] == ro["score"]
    assert np.array_equal(rd["arcs"], ro["arcs"])
    assert np.array_equal(rd["words"], ro["words"])
    assert rd["activeHypos"] == ro["activeHypos"]


@pytest.mark.parametrize("seed,S,nDist,T,beam,kw", [
    (1, 200, 16, 50, 30.0, {}),
    (2, 2000, 128, 120, 1e9, {}),
    (3, 2000, 128, 120, 20.0, dict(lmPenalty=0.7)),
    (4, 2000, 128, 120, 8.0, dict(silPenalty=1.5, silenceX=3)),
    (5, 500, 32, 60, 50.0, dict(ties=True)),
    (6, 300, 8, 40, 25.0, dict(eps_frac=0.35)),
    (7, 400, 16, 30, 40.0, dict(nFinal=0)),
])
def test_viterbi_bit_exact(dsr, oracle, cuda, seed, S, nDist, T, beam, kw):
    import torch
    gkw = {k: kw[k] for k in ("ties", "eps_frac", "nFinal") if k in kw}
    dkw = {k: kw[k] for k in ("lmPenalty", "silPenalty", "silenceX") if k in kw}
    arcs, fin = synth.random_wfst(S, nDist, seed=seed, **gkw)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    eo, ed = go.export(), gd.export()
    for k in eo:
        assert np.array_equal(eo[k], ed[k]), k            # identical node/arc numbering
    rng = np.random.default_rng(100 + seed)
    sc = rng.uniform(0, 10, (3, T, nDist)).astype(np.float32)
    if kw.get("ties"):
        sc = np.round(sc)                                  # integer scores: exact ties everywhere
    nfr = [T, T - 7, 1]
    dec = dsr.Decoder(beam=beam, lmScale=12.0, maxActive=8192, streams=2, **dkw)
    dec.set(gd)
    out = dec.decode_batch(torch.from_numpy(sc).to(cuda), torch.tensor(nfr, dtype=torch.int32, device=cuda))
    for u in range(3):
        ro = go.decode(sc[u, :nfr[u]], beam=beam, lmScale=12.0, **dkw)
        assert ro["rc"] == 0
        _check_decode(ro, out[u])


@pytest.mark.parametrize("seed,S,gkw,path", [
    (11, 4000, dict(ties=True), "register"),          # ~23k placements a frame: parked batches + two passes over the state table
    (12, 600, dict(eps_frac=0.3), "register"),        # parked batches, epsilon paths longer than one hop
    (13, 4000, dict(ties=True), "memory"),            # the same frames through the memory path
    (14, 9500, dict(), "register"),                   # > 24576 placements: the register path hands the frame over
])
def test_viterbi_large_frames(dsr, oracle, cuda, seed, S, gkw, path, monkeypatch):
    """Frames far above the 8192 placements the registers hold: every list size class of the decoder kernel against the oracle."""
    import torch
    arcs, fin = synth.random_wfst(S, 64, seed=seed, **gkw)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    rng = np.random.default_rng(seed)
    T = 14
    sc = rng.uniform(0, 4, (2, T, 64)).astype(np.float32)
    if gkw.get("ties"):
        sc = np.round(sc)
    if path == "memory":
        monkeypatch.setenv("DSR_VITERBI_NOFAST", "1")
    dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=2)
    dec.set(gd)
    out = dec.decode_batch(torch.from_numpy(sc).to(cuda))
    for u in range(2):
        ro = go.decode(sc[u], beam=1e9, lmScale=2.0)
        assert ro["rc"] == 0
        _check_decode(ro, out[u])
        assert out[u]["placements"] / T > 5000, "the case is meant to produce large frames"
        if path == "memory":
            assert out[u]["registerFrames"] == 0
        elif S < 9000:
            print("placements/frame %.0f, register frames %d of %d" % (out[u]["placements"] / T, out[u]["registerFrames"], T))
            assert out[u]["registerFrames"] >= (T if seed == 11 else 6)
        else:
            assert 0 < out[u]["registerFrames"] < T


def test_wfst_dynamic_reader(dsr, oracle, cuda, tmp_path):
    """WFSTransducer::read(fileName, noSelfLoops) (asr/fsm/fsm.cc:901-986): identical numbering with and without self loops."""
    arcs, fin = synth.random_wfst(300, 16, seed=41, eps_frac=0.2)
    rng = np.random.default_rng(41)
    f = tmp_path / "g.txt"
    with open(f, "w") as fp:
        for (s1, s2, i, o, c) in arcs:
            fp.write("%d %d %d %d %g\n" % (s1, s2, i, o, c))
            if rng.random() < 0.1:
                fp.write("%d %d %d %d %g\n" % (s1, s1, 1 + int(rng.integers(16)), 0, 0.5))     # an emitting self loop
        for s, c in fin:
            fp.write("%d %g\n" % (s, c))
    for nsl in (False, True):
        go, gd = oracle.Wfst(), dsr.Wfst()
        assert go.read_dynamic(str(f), nsl) == 0
        gd.read_dynamic(str(f), nsl)
        eo, ed = go.export(), gd.export()
        for k in eo:
            assert np.array_equal(eo[k], ed[k]), k
    g0 = dsr.Wfst(); g0.read_dynamic(str(f), False); g1 = dsr.Wfst(); g1.read_dynamic(str(f), True)
    assert g1.export()["arcDst"].size < g0.export()["arcDst"].size


def test_viterbi_token_lists(dsr, oracle, cuda):
    """Every frame's active list: same states in the same list order with the same float scores."""
    import torch
    arcs, fin = synth.random_wfst(1500, 64, seed=9, ties=True)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    rng = np.random.default_rng(77)
    sc = np.round(rng.uniform(0, 6, (1, 80, 64))).astype(np.float32)
    dec = dsr.Decoder(beam=15.0, lmScale=1.0, maxActive=8192, streams=1); dec.set(gd); dec.enable_dump(True)
    out = dec.decode_batch(torch.from_numpy(sc).to(cuda))
    ro = go.decode(sc[0], beam=15.0, lmScale=1.0, dump=True)
    _check_decode(ro, out[0])
    d = dec.get_dump()
    assert np.array_equal(d["frameOff"], ro["dumpOff"])
    assert np.array_equal(d["node"], ro["dumpNode"])
    assert np.array_equal(d["arc"], ro["dumpArc"])
    assert np.array_equal(d["ac"].view(np.uint32), ro["dumpAc"].view(np.uint32))
    assert np.array_equal(d["lm"].view(np.uint32), ro["dumpLm"].view(np.uint32))


def test_viterbi_long_epsilon_paths(dsr, oracle, cuda):
    """Epsilon chains of 1, 2, 3, 14, 15 and 20 hops (outputs on some hops) in front of emitting arcs: the expansion records carry
    one and two hops inline, up to 14 through the hop-cost table, longer ones through the path arrays -- all against the oracle."""
    import torch
    nDist = 6
    arcs = []; nxt = [1]
    def new():
        nxt[0] += 1; return nxt[0] - 1
    hub = 0
    rng = np.random.default_rng(5)
    for hops in (0, 1, 2, 3, 14, 15, 20):
        for rep in range(2):
            cur = hub
            for h in range(hops):
                n2 = new(); arcs.append((cur, n2, 0, int(rng.integers(0, 3)) if (h % 3 == rep) else 0, float(np.float32(rng.uniform(0.1, 1.5))))); cur = n2
            n2 = new(); arcs.append((cur, n2, 1 + int(rng.integers(0, nDist)), int(rng.integers(0, 4)), float(np.float32(rng.uniform(0.1, 1.5)))))
            arcs.append((n2, n2, 1 + int(rng.integers(0, nDist)), 0, float(np.float32(rng.uniform(0.1, 1.5)))))        # self loop
            arcs.append((n2, hub, 1 + int(rng.integers(0, nDist)), 0, float(np.float32(rng.uniform(0.1, 1.5)))))       # back to the hub
    fin = [(hub, 0.0)]
    go, gd = _graphs(dsr, oracle, arcs, fin)
    sc = rng.uniform(0, 3, (1, 40, nDist)).astype(np.float32)
    ro = go.decode(sc[0], beam=1e9, lmScale=3.0, lmPenalty=0.7, dump=True)
    assert ro["rc"] == 0
    for env in (None, "1"):
        if env:
            os.environ["DSR_VITERBI_NOFAST"] = env
        try:
            dec = dsr.Decoder(beam=1e9, lmScale=3.0, lmPenalty=0.7, maxActive=8192, streams=1); dec.set(gd); dec.enable_dump(True)
        finally:
            os.environ.pop("DSR_VITERBI_NOFAST", None)
        out = dec.decode_batch(torch.from_numpy(sc).to(cuda))
        _check_decode(ro, out[0])
        d = dec.get_dump()
        assert np.array_equal(d["node"], ro["dumpNode"]) and np.array_equal(d["arc"], ro["dumpArc"])
        assert np.array_equal(d["lm"].view(np.uint32), ro["dumpLm"].view(np.uint32))
        assert (out[0]["registerFrames"] > 0) == (env is None)


@pytest.mark.parametrize("seg,streams,path,U", [(7, 3, "register", 29), (5, 8, "register", 29), (16, 9, "register", 29), (7, 3, "memory", 29), (6, 256, "register", 700), (9, 64, "register", 150),
                                                 (6, 256, "drop", 700)])
def test_viterbi_time_sliced(dsr, oracle, cuda, monkeypatch, seg, streams, path, U):
    """More utterances than workgroups: the decode is time-sliced (DSR_VITERBI_SEG frames a segment; an utterance is put down after its segment -- token list and
    scalars in memory, back-pointer records in the batch's pool -- and taken up by whichever workgroup comes next: of its XCD (grids of 8 k >= 64 workgroups, the
    hand-over stays inside one L2) or, on small grids and only when DSR_VITERBI_SEG_ANY asks for it, any (device-scope fences).  Ragged lengths (utterances that end
    in different segments, one of a single frame, one without frames), utterances that fail in a late segment (their capacity runs out) while their neighbours carry
    on: every result equals the run-to-completion decode (DSR_VITERBI_SEG=0) field for field and the oracle's bits."""
    import torch
    arcs, fin = synth.random_wfst(1500, 48, seed=31, eps_frac=0.2)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    rng = np.random.default_rng(77)
    T = 45
    monkeypatch.setenv("DSR_VITERBI_SEG_ANY", "1")
    sc = rng.uniform(0, 8, (U, T, 48)).astype(np.float32)
    nfr = [int(v) for v in rng.integers(2, T + 1, U)]
    nfr[0] = T; nfr[3] = 1; nfr[5] = 0; nfr[9] = seg; nfr[10] = seg + 1; nfr[11] = 2 * seg - 1
    if path == "memory":
        monkeypatch.setenv("DSR_VITERBI_NOFAST", "1")
    if path == "drop":                                      # the workgroups of XCDs 2 and 5 do not serve their queues: the others pick those utterances up whole (the net under the XCD-bound queues)
        monkeypatch.setenv("DSR_VITERBI_SEG_DROP", "0x24")

    def run(segv, **dkw):
        monkeypatch.setenv("DSR_VITERBI_SEG", str(segv))
        dec = dsr.Decoder(beam=22.0, lmScale=12.0, streams=streams, **dkw); dec.set(gd)
        return dec.decode_batch(torch.from_numpy(sc).to(cuda), torch.tensor(nfr, dtype=torch.int32, device=cuda))
    a = run(seg, maxActive=8192); b = run(0, maxActive=8192)
    keys = ["status", "score", "ac", "lm", "frames", "reachedFinal", "activeHypos", "maxActive", "placements", "registerFrames", "finalStatesN"]
    for u in range(U):
        assert [a[u][k] for k in keys] == [b[u][k] for k in keys], (u, nfr[u])
        assert np.array_equal(a[u]["arcs"], b[u]["arcs"]) and np.array_equal(a[u]["words"], b[u]["words"]), u
        if nfr[u] == 0:
            assert a[u]["status"] == 9
        elif u < 40:
            ro = go.decode(sc[u, :nfr[u]], beam=22.0, lmScale=12.0)
            assert ro["rc"] == 0
            _check_decode(ro, a[u])
    # a capacity that some utterances outgrow after a few segments: those fail (DSR_E_ALLOCATION) exactly where the unsliced decode fails them, the others are untouched
    small = max(8, int(np.percentile([r["maxActive"] for r in a if r["status"] == 0], 60)))
    c = run(seg, maxActive=small); d = run(0, maxActive=small)
    assert sorted(set(r["status"] for r in c)) == [0, 2, 9] or sorted(set(r["status"] for r in c)) == [2, 9]
    for u in range(U):
        assert c[u]["status"] == d[u]["status"], u
        if c[u]["status"] == 0:
            assert [c[u][k] for k in keys] == [a[u][k] for k in keys] and np.array_equal(c[u]["words"], a[u]["words"])
    # the same with the back-pointer records: cfg.arenaTokens bounds an utterance's records in both forms (sliced, they come in runs from the batch's pool)
    cap = int(np.percentile([r["activeHypos"] for r in a if r["status"] == 0], 50) / 4)          # (records are the tokens WRITTEN: a fraction of the active ones)
    e = run(seg, maxActive=8192, arenaTokens=cap); f = run(0, maxActive=8192, arenaTokens=cap)
    assert [r["status"] for r in e] == [r["status"] for r in f], (cap, [r["status"] for r in e], [r["status"] for r in f])
    assert 2 in [r["status"] for r in e] and 0 in [r["status"] for r in e], (cap, [r["status"] for r in e])


def test_viterbi_errors(dsr, oracle, cuda):
    import torch
    arcs, fin = synth.random_wfst(100, 8, seed=1)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    dec = dsr.Decoder(beam=30.0, maxActive=8192, streams=1); dec.set(gd)
    sc = torch.zeros((1, 4, 8), device=cuda)
    r = dec.decode_batch(sc, torch.tensor([0], dtype=torch.int32, device=cuda))
    assert r[0]["status"] == 9                           # JITERATOR: no frames (decoder.h:691)
    tiny = dsr.Decoder(beam=1e9, maxActive=4, streams=1); tiny.set(gd)
    r = tiny.decode_batch(torch.rand((1, 20, 8), device=cuda))
    assert r[0]["status"] == 2                           # capacity exceeded is reported, never silent
    g2 = dsr.Wfst(); g2.add_arc(0, 1, 1, 0, 1.0); g2.add_arc(1, 2, 0, 0, 0.0); g2.add_arc(2, 1, 0, 0, 0.0)
    with pytest.raises(dsr.DsrError):
        dsr.Decoder().set(g2)                            # epsilon cycle


# ------------------------------------------------------------------------------------------- whole pipe
@pytest.mark.parametrize("fused", [False, True])
def test_full_pipe_small(dsr, oracle, cuda, protos, fused):
    """8-ch analysis -> MVDR -> synthesis -> MFCC -> GMM -> Viterbi for 3 ragged utterances against the chained oracle.
    GMM+WFST are fed the device features on both sides (bit-exact check); the front end is checked to tolerance."""
    import torch
    M, m, r, h, g = protos["M256-m4-r1"]
    Cn = 8
    lens = [16000, 12000, 9000]
    x = np.zeros((len(lens), Cn, max(lens)), np.float32)
    for u, n in enumerate(lens):
        x[u, :, :n] = synth.array_signal(n, Cn, seed=7 + u)
    ana = dsr.FilterBank(h, M, m, r, False, 0); syn = dsr.FilterBank(g, M, m, r, True, 0)
    bf, delays, wq, R, w = _mvdr_setup(dsr, oracle, M, Cn); bf.select("mvdr")
    rng = np.random.default_rng(1234)
    lda = (rng.standard_normal((39, 195)) / np.sqrt(195)).astype(np.float32)
    mf = dsr.Mfcc(lda=lda)
    K = 64
    gm_m = synth.gmm_model(K, 16, 39, seed=12)
    gm_m["mean"] *= 3.0
    gm = dsr.Gmm(**gm_m)
    arcs, fin = synth.random_wfst(3000, K, seed=21)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    dec = dsr.Decoder(beam=60.0, lmScale=12.0, maxActive=16384, streams=4); dec.set(gd)
    pipe = dsr.Pipe(ana, syn, bf, mf, gm, dec, gmmMode=0, fused=fused)          # fused: analysis bank + beamformer as one kernel
    xd = torch.from_numpy(x).to(cuda); nd = torch.tensor(lens, dtype=torch.int32, device=cuda)
    res, arcsO, wordsO = pipe.run(xd, nd, lens, maxPath=2048)
    if fused:
        with pytest.raises(dsr.DsrError):
            pipe.intermediate(0)                                                 # the channel snapshots were never written
    W = bf.get(4)
    cfg = oracle.mfcc_cfg(lda=lda)
    cb = oracle.Codebooks(gm_m["refN"], gm_m["mean"], gm_m["ivar"], gm_m["det"])
    Tm = max(mf.frames(((n + 127) // 128) * 128) for n in lens)
    feat_dev = pipe.intermediate_host(3)[: len(lens) * Tm * 39].reshape(len(lens), Tm, 39)
    for u, n in enumerate(lens):
        Xc = np.stack([oracle.analysis_bank(x[u, c, :n], h, M, m, r, 0) for c in range(Cn)])
        Yo = oracle.beamform_apply(Xc, W)
        yo = oracle.synthesis_bank(Yo, g, M, m, r, 0)
        fo = oracle.mfcc_chain(yo, cfg)
        T = fo.shape[0]
        assert np.abs(feat_dev[u, :T] - fo).max() < 2e-3          # fp32 filterbank vs fp64 reference, after LDA
        so, _ = oracle.gmm_score_opt(cb, gm_m["val"], feat_dev[u, :T])
        ro = go.decode(so, beam=60.0, lmScale=12.0)
        assert res[u].status == 0
        assert res[u].score == ro["score"] and res[u].nArcs == len(ro["arcs"])
        assert np.array_equal(arcsO[u, :res[u].nArcs], ro["arcs"])
        assert np.array_equal(wordsO[u, :res[u].nWords], ro["words"])


@pytest.mark.parametrize("fused", [False, True])
def test_full_pipe_batch_invariance(dsr, cuda, protos, fused):
    """Every stage with far more workgroups than compute units (co-resident workgroups, several rounds, more utterances than
    decoder slots): each utterance's intermediates and 1-best are bit-identical to those it gets in a batch of its own."""
    import torch
    M, m, r, h, g = protos["M256-m4-r1"]
    Cn, U, n = 8, 300, 8000
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((U, Cn, n)) * 2000.0).astype(np.float32)
    lens = [n - 3 * (u % 5) for u in range(U)]                        # ragged, same number of blocks (same padded strides)
    for u, L in enumerate(lens):
        x[u, :, L:] = 0.0
    ana = dsr.FilterBank(h, M, m, r, False, 0); syn = dsr.FilterBank(g, M, m, r, True, 0)
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(np.deg2rad(30.0)), np.float32(np.pi / 2), mp)
    bf = dsr.Beamformer(M, Cn); bf.calcArrayManifoldVectors(16000.0, delays); bf.setDiffuseNoiseModel(mp, 16000.0, 343740.0)
    bf.divideAllNonDiagonalElements(0.01); bf.calcMVDRWeights(16000.0, 1e-8); bf.select("mvdr")
    lda = (rng.standard_normal((39, 195)) / np.sqrt(195)).astype(np.float32)
    K = 64
    gm_m = synth.gmm_model(K, 16, 39, seed=12); gm_m["mean"] *= 3.0
    gm = dsr.Gmm(**gm_m)
    arcs, fin = synth.random_wfst(3000, K, seed=21)
    gd = dsr.Wfst()
    for a in arcs:
        gd.add_arc(*a)
    for st, c in fin:
        gd.add_final(st, c)

    def run(idx):
        mf = dsr.Mfcc(lda=lda)
        dec = dsr.Decoder(beam=60.0, lmScale=12.0, maxActive=16384); dec.set(gd)
        pipe = dsr.Pipe(ana, syn, bf, mf, gm, dec, gmmMode=0, fused=fused)
        xs = torch.from_numpy(np.ascontiguousarray(x[idx])).to(cuda); ls = [lens[i] for i in idx]
        res, arcsO, wordsO = pipe.run(xs, torch.tensor(ls, dtype=torch.int32, device=cuda), ls, maxPath=512)
        inter = [pipe.intermediate_host(k).copy() if not (fused and k == 0) else np.zeros(0, np.float32) for k in range(5)]
        return res, arcsO, wordsO, inter

    allidx = list(range(U))
    resA, arcsA, wordsA, interA = run(allidx)
    for u in (0, 7, 255, 256, 299):
        resS, arcsS, wordsS, interS = run([u])
        for k in range(5):
            per = interS[k].size                                     # one utterance's share; Tmax is the same (equal padded lengths)
            assert np.array_equal(interA[k][u * per:(u + 1) * per].view(np.uint32), interS[k].view(np.uint32)), (u, k)
        assert resA[u].status == 0 and resA[u].score == resS[0].score and resA[u].nArcs == resS[0].nArcs
        nA, nW = resA[u].nArcs, resA[u].nWords
        assert nW == resS[0].nWords and np.array_equal(arcsA[u, :nA], arcsS[0, :nA]) and np.array_equal(wordsA[u, :nW], wordsS[0, :nW])


def test_pipelined_steps_equal_serial_steps(dsr, cuda, protos):
    """bench.py's default: two pipe objects on two streams, step k+1 enqueued while step k decodes, results collected later with reused host arrays.
    Every step's results -- scores, arcs, words, the features -- are those of the same batch run alone on one pipe."""
    import torch
    M, m, r, h, g = protos["M256-m4-r1"]
    Cn, U, n = 8, 40, 6000
    rng = np.random.default_rng(91)
    ana = dsr.FilterBank(h, M, m, r, False, 0); syn = dsr.FilterBank(g, M, m, r, True, 0)
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(np.deg2rad(30.0)), np.float32(np.pi / 2), mp)
    bf = dsr.Beamformer(M, Cn); bf.calcArrayManifoldVectors(16000.0, delays); bf.setDiffuseNoiseModel(mp, 16000.0, 343740.0)
    bf.divideAllNonDiagonalElements(0.01); bf.calcMVDRWeights(16000.0, 1e-8); bf.select("mvdr")
    lda = (rng.standard_normal((39, 195)) / np.sqrt(195)).astype(np.float32)
    K = 64
    gm_m = synth.gmm_model(K, 16, 39, seed=12); gm_m["mean"] *= 3.0
    gm = dsr.Gmm(**gm_m)
    arcs, fin = synth.random_wfst(3000, K, seed=21)
    gd = dsr.Wfst()
    for a in arcs:
        gd.add_arc(*a)
    for st, c in fin:
        gd.add_final(st, c)
    batches = [(rng.standard_normal((U, Cn, n)) * 2000.0).astype(np.float32) for _ in range(4)]
    lens = [n - 5 * (u % 7) for u in range(U)]
    nd = torch.tensor(lens, dtype=torch.int32, device=cuda)

    def make():
        dec = dsr.Decoder(beam=60.0, lmScale=12.0, maxActive=16384); dec.set(gd)
        return dsr.Pipe(ana, syn, bf, dsr.Mfcc(lda=lda), gm, dec, gmmMode=2, fused=True)
    ref = []
    p0 = make()
    for xb in batches:
        res, arcsO, wordsO = p0.run(torch.from_numpy(xb).to(cuda), nd, lens, maxPath=512)
        ref.append(([(q.status, q.score, q.nArcs, q.nWords) for q in res], arcsO.copy(), wordsO.copy()))
    pipes = [make(), make()]; streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    xs = [torch.from_numpy(xb).to(cuda) for xb in batches]
    torch.cuda.synchronize()
    got = [None] * len(batches); inflight = [None, None]
    for k in range(len(batches) + 2):
        i = k % 2
        if inflight[i] is not None:
            res, arcsO, wordsO = pipes[i].collect(reuse=True)
            got[inflight[i]] = ([(q.status, q.score, q.nArcs, q.nWords) for q in res], arcsO.copy(), wordsO.copy()); inflight[i] = None
        if k < len(batches):
            with torch.cuda.stream(streams[i]):
                pipes[i].submit(xs[k], nd, lens, maxPath=512, want_paths=True)
            inflight[i] = k
    for k in range(len(batches)):
        assert got[k][0] == ref[k][0], k
        for u in range(U):
            st, sc, nA, nW = ref[k][0][u]
            assert st == 0 and np.array_equal(got[k][1][u, :nA], ref[k][1][u, :nA]) and np.array_equal(got[k][2][u, :nW], ref[k][2][u, :nW]), (k, u)


@pytest.mark.parametrize("K,R,D", [(256, 16, 39), (1024, 4, 39), (5, 7, 13), (3, 256, 39), (40, 33, 20)])
def test_gmm_mfma_mode(dsr, oracle, cuda, K, R, D):
    """mode 2 (fp32 MFMA, expanded quadratic): the nearest Gaussian is the reference's on EVERY frame (every codebook whose two best lie inside the
    rounding bound of the expanded form is re-scored in reference order, all its Gaussians); the cost carries the stated tolerance rel 1e-5."""
    import torch
    m = synth.gmm_model(K, R, D, seed=12)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3000, D)).astype(np.float32)
    gm = dsr.Gmm(**m)
    sc, am = gm.score(torch.from_numpy(x).to(cuda), mode=2)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    ref, arg = oracle.gmm_score_opt(cb, m["val"], x)
    sc = sc.cpu().numpy(); am = am.cpu().numpy().astype(np.int32)
    assert np.array_equal(am, arg)
    assert (np.abs(sc - ref) / np.maximum(np.abs(ref), 1.0)).max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,N,tiecap,R", [(7, 39, 1000, None, 4), (9, 13, 129, None, 4), (17, 39, 700, None, 4), (100, 20, 513, None, 4), (41, 39, 2000, 3, 4), (1024, 39, 640, 16, 4), (16, 5, 1, None, 4),
                                            (7, 39, 1000, None, 8), (33, 13, 515, 2, 8), (5, 39, 700, None, 16), (67, 13, 129, None, 16), (130, 39, 300, 5, 16), (3, 39, 1000, None, 32), (37, 13, 640, 4, 32)])
def test_gmm_mfma_four_gaussian_codebooks(dsr, oracle, cuda, monkeypatch, K, D, N, tiecap, R):
    """Codebooks of four (and, at the depths of 13- and 39-dimensional features, 8 / 16 / 32) Gaussians go through the one-wave-per-SIMD shape (k_gmm_sp.hip): a last chunk that the codebooks do not fill, an odd chunk
    count (a phantom chunk closes the pair), frame counts that end inside a tile / a wave / a workgroup, a strip of fewer than 32 codebooks, the
    contraction depths of 5-, 13-, 20- and 39-dimensional features (tests/test_gpu_gmm_shapes.py runs every depth the kernels are instantiated for, on
    near-tie frames) -- and a tie list that fills up (entries settled in place).  Argmin = the reference's on every
    frame, scores within the stated tolerance; the other shape (DSR_GMM_SP=0: two waves per SIMD) gives the same argmins and scores within the same
    tolerance (an entry on the edge of the trust radius may be re-scored exactly by one shape and not by the other)."""
    import torch
    m = synth.gmm_model(K, R, D, seed=12 + K)
    rng = np.random.default_rng(K)
    x = rng.standard_normal((N, D)).astype(np.float32)
    gm = dsr.Gmm(**m)
    if tiecap is not None:
        monkeypatch.setenv("DSR_GMM_TIECAP", str(tiecap))
    xd = torch.from_numpy(x).to(cuda)
    sc, am = gm.score(xd, mode=2)
    monkeypatch.setenv("DSR_GMM_SP", "0")
    sc_b, am_b = gm.score(xd, mode=2)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    ref, arg = oracle.gmm_score_opt(cb, m["val"], x)
    assert np.array_equal(am.cpu().numpy().astype(np.int32), arg)
    assert (np.abs(sc.cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0)).max() < 1e-5
    assert torch.equal(am, am_b) and float(((sc - sc_b).abs() / sc_b.abs().clamp(min=1.0)).max()) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("K,R,D,mu0,sigma", [(64, 4, 39, 50.0, 0.1), (32, 16, 39, 50.0, 0.1), (24, 8, 13, -300.0, 0.05), (7, 5, 20, 50.0, 0.1), (64, 4, 39, 5.0, 0.5)])
def test_gmm_mfma_mode_offset_means(dsr, oracle, cuda, K, R, D, mu0, sigma):
    """Means far from zero with small variances (|mu| / sigma ~ 1e3): the terms the expanded form cancels are ~1e6 times the distance, so its
    rounding error exceeds the distances themselves.  The trust test scales with the cancelled terms (2 ivMax |x|^2 + termMax), not with the
    distance: every such (frame, codebook) is re-scored in the reference's arithmetic -- argmin AND score equal mode 0's bits on every frame."""
    import torch
    rng = np.random.default_rng(5)
    m = synth.gmm_model(K, R, D, seed=3)
    G = m["mean"].shape[0]
    m["mean"] = (mu0 + sigma * rng.standard_normal((G, D)) * 2.0).astype(np.float32)
    m["ivar"] = (1.0 / (sigma * rng.uniform(0.7, 1.4, (G, D))) ** 2).astype(np.float32)
    x = (mu0 + sigma * 2.0 * rng.standard_normal((2500, D))).astype(np.float32)
    gm = dsr.Gmm(**m)
    xd = torch.from_numpy(x).to(cuda)
    sc0, am0 = gm.score(xd, mode=0)
    sc2, am2 = gm.score(xd, mode=2)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    ref, arg = oracle.gmm_score_opt(cb, m["val"], x)
    assert np.array_equal(am0.cpu().numpy().astype(np.int32), arg) and np.array_equal(sc0.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert torch.equal(am2, am0)
    if abs(mu0) / sigma >= 100:
        assert torch.equal(sc2, sc0)                     # all of them went through the exact re-score
    else:
        assert float(((sc2 - sc0).abs() / sc0.abs().clamp(min=1.0)).max()) < 1e-5


@pytest.mark.gpu
def test_gmm_mfma_two_streams_do_not_share_scratch(dsr, cuda):
    """Mode 2 hands its near-tie worklist from the contraction kernel to the re-score kernel of the same stream.  Two inputs scored with ONE model on
    two streams, stream A held back by a long kernel between the submission and the use of its results while stream B runs through: each input
    gets the bits of its own serial run (the worklist is owned by the model, one per stream -- csrc/gmm_model.h)."""
    import torch
    K, R, D, N = 1024, 4, 39, 60000
    m = synth.gmm_model(K, R, D, seed=12)
    gm = dsr.Gmm(**m)
    g = torch.Generator(device=cuda); g.manual_seed(9)
    xa = torch.randn((N, D), generator=g, device=cuda); xb = torch.randn((N, D), generator=g, device=cuda) * 1.3
    ra = gm.score(xa, mode=2); rb = gm.score(xb, mode=2)                      # serial runs, default stream
    ra = (ra[0].clone(), ra[1].clone()); rb = (rb[0].clone(), rb[1].clone())
    big = torch.randn((4096, 4096), device=cuda)
    sA, sB = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in range(3):
        with torch.cuda.stream(sA):
            for _ in range(6):
                big = torch.tanh(big @ big * 1e-3)                           # a few ms of work ahead of A's scoring
            oa = gm.score(xa, mode=2)
        with torch.cuda.stream(sB):
            ob = gm.score(xb, mode=2)
            ob2 = gm.score(xb, mode=2)
        sA.synchronize(); sB.synchronize()
        assert torch.equal(oa[0], ra[0]) and torch.equal(oa[1], ra[1]), rep
        assert torch.equal(ob[0], rb[0]) and torch.equal(ob[1], rb[1]) and torch.equal(ob2[0], rb[0]), rep


# ------------------------------------------------------------------------------------------- LPC / MVDR envelopes
def _ar_frames(T, dim, seed):
    rng = np.random.default_rng(seed)
    fr = np.zeros((T, dim), np.float32)
    for t in range(T):
        rad, th = rng.uniform(0.5, 0.95), rng.uniform(0.2, 2.8); a1, a2 = 2 * rad * np.cos(th), -rad * rad      # a stable resonance
        e = rng.standard_normal(dim + 64) * 300.0; y = np.zeros(dim + 64)
        for n in range(2, dim + 64):
            y[n] = a1 * y[n - 1] + a2 * y[n - 2] + e[n]
        fr[t] = (y[64:] * np.hamming(dim)).astype(np.float32)
    return fr


@pytest.mark.gpu
@pytest.mark.parametrize("method,kind,order,warp,dim", [
    (0, 0, 20, 0.0, 320), (0, 0, 60, 0.4595, 320), (1, 0, 20, 0.0, 320), (0, 1, 13, 0.0, 320), (0, 1, 13, 0.3, 400),
    (1, 1, 13, 0.0, 320), (1, 0, 40, 0.0, 512), (0, 0, 8, -0.2, 64),
])
def test_lpc_envelopes(dsr, oracle, cuda, method, kind, order, warp, dim):
    """lpc.cc:44-207, lpc.h:134-195,291-331: the fp32 recursions are replayed in the reference's order (thread per frame), so the
    envelopes agree with the oracle to the rounding of the fp64 DFT (1e-9 relative asserted; the oracle's DFT sums the same terms)."""
    import torch
    fr = _ar_frames(70, dim, seed=31 + order)
    fr[3] = 0.0                                             # an all-zero frame: E[0] = 0 branches (lpc.cc:117-121, lpc.h:162-166)
    want = oracle.lpc_feature(fr, order, warp, method, kind)
    got = dsr.LpcEnvelope(dim, order, warp, method, kind).run(torch.from_numpy(fr).to(cuda)).cpu().numpy()
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-9, atol=0)


@pytest.mark.gpu
def test_lpc_feature_streams(dsr, oracle, cuda, headset):
    """WarpMVDRFeaturePtr / BurgLPCFeaturePtr behind the stream protocol: Sample -> Hamming -> envelope."""
    from dsr.btk import feature as F
    x = headset[:16000].astype(np.float32)
    samp = F.SampleFeaturePtr(blockLen=320, shiftLen=160, padZeros=False); samp.setSamples(x, 16000)
    ham = F.HammingFeaturePtr(samp)
    blocks = oracle.sample_blocks(x, 320, 160, False)
    w = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(320) / 319.0)
    fr = (blocks.astype(np.float64) * w).astype(np.float32)
    for cls, method, kind in ((F.WarpMVDRFeaturePtr, 0, 0), (F.BurgLPCFeaturePtr, 1, 1)):
        op = cls(ham, order=30, warp=0.0)
        assert op.size() == 161
        rows = [np.array(v) for v in op]
        want = oracle.lpc_feature(fr, 30, 0.0, method, kind)
        assert len(rows) == want.shape[0]
        np.testing.assert_allclose(np.array(rows), want, rtol=1e-9)
    with pytest.raises(Exception):
        F.WarpLPCFeaturePtr(ham, order=161)                 # lpc.h:126-127: order >= dim/2+1


# ------------------------------------------------------------------------------------------- NormalFFTAnalysisBank
@pytest.mark.gpu
@pytest.mark.parametrize("M,r,win", [(256, 1, 1), (512, 2, 2), (64, 0, 0), (128, 3, 1)])
def test_normal_fft_bank(dsr, oracle, cuda, headset, M, r, win):
    """modulated.cc:72-97,121-257: windowed STFT (all M bins), fp32 on the device vs the fp64 oracle: 2e-5 of the frame RMS."""
    import torch
    x = headset[3000:3000 + 4000 + 37].astype(np.float32)              # ragged: not a multiple of D
    want = oracle.normal_fft_bank(x, M, r, winType=win)
    bank = dsr.NormalFFTBank(M, r, win)
    xs = np.stack([x, x[::-1].copy()])[None]                          # [U=1][C=2][N]
    got = bank.analysis(torch.from_numpy(xs).to(cuda)).cpu().numpy()
    assert got.shape[2:] == want.shape
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    assert np.abs(got[0, 0] - want).max() < 2e-5 * rms * np.sqrt(M)
    want2 = oracle.normal_fft_bank(x[::-1].copy(), M, r, winType=win)
    assert np.abs(got[0, 1] - want2).max() < 2e-5 * rms * np.sqrt(M)
    # the operator behind the stream protocol
    from dsr.btk import feature as F, modulated as Mo
    D = M >> r
    samp = F.SampleFeaturePtr(blockLen=D, shiftLen=D, padZeros=True); samp.setSamples(x, 16000)
    rows = np.array([np.array(v) for v in Mo.NormalFFTAnalysisBankPtr(samp, M, r, win)])
    assert rows.shape == want.shape and rows.dtype == np.complex128
    assert np.abs(rows - want).max() < 2e-5 * rms * np.sqrt(M)


# ------------------------------------------------------------------------------------------- PerfectReconstructionFFT banks
@pytest.mark.gpu
@pytest.mark.parametrize("M,m,r", [(128, 2, 0), (64, 3, 1), (256, 2, 2), (16, 4, 0)])
def test_pr_fft_banks(dsr, oracle, cuda, headset, M, m, r):
    """modulated.cc:686-970: the 2M-band pair, fp32 on the device vs the literal fp64 restatement of the ring buffers: 2e-5 of the RMS
    (analysis), 1e-4 of the RMS (synthesis: the reference accumulates the output in fp32 as well)."""
    import torch
    rng = np.random.default_rng(M + m)
    N = 2 * M * m
    h = np.sin(np.pi * (np.arange(N) + 0.5) / N) * rng.uniform(0.9, 1.1, N)
    x = headset[5000:5000 + 3000 + 11].astype(np.float32)
    want = oracle.pr_analysis_bank(x, h, M, m, r)
    bank = dsr.PrFilterBank(h, M, m, r)
    got = bank.analysis(torch.from_numpy(x[None, None]).to(cuda)).cpu().numpy()[0, 0]
    assert got.shape == want.shape
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    assert np.abs(got - want).max() < 2e-5 * rms * np.sqrt(2 * M)
    # synthesis of a random subband sequence
    T = 40
    Y = (rng.standard_normal((T, 2 * M)) + 1j * rng.standard_normal((T, 2 * M))) * 100.0
    g = rng.standard_normal(N)
    wy = oracle.pr_synthesis_bank(Y, g, M, m, r)
    gy = dsr.PrFilterBank(g, M, m, r).synthesis(torch.from_numpy(Y.astype(np.complex64)[None]).to(cuda)).cpu().numpy()[0]
    assert gy.size == wy.size
    yr = np.sqrt(np.mean(wy.astype(np.float64) ** 2))
    assert np.abs(gy.reshape(wy.shape) - wy).max() < 1e-4 * yr * np.sqrt(2 * M)
    # both operators behind the stream protocol: samples -> analysis -> synthesis
    from dsr.btk import feature as F, modulated as Mo
    D = M >> r
    samp = F.SampleFeaturePtr(blockLen=D, shiftLen=D, padZeros=True); samp.setSamples(x, 16000)
    ana = Mo.PerfectReconstructionFFTAnalysisBankPtr(samp, h, M, m, r)
    assert ana.size() == 2 * M and ana.fftLen() == 2 * M
    syn = Mo.PerfectReconstructionFFTSynthesisBankPtr(ana, g, M, m, r)
    rows = np.array([np.array(v) for v in syn])
    wy2 = oracle.pr_synthesis_bank(want, g, M, m, r)
    assert rows.shape == wy2.shape
    assert np.abs(rows - wy2).max() < 2e-4 * np.sqrt(np.mean(wy2.astype(np.float64) ** 2)) * np.sqrt(2 * M)
    with pytest.raises(Exception):
        Mo.PerfectReconstructionFFTAnalysisBankPtr(samp, h[:-1], M, m, r)


# ------------------------------------------------------------------------------------------- Zelinski post-filter
@pytest.mark.gpu
@pytest.mark.parametrize("Cn,ptype,alpha,minFrames", [(8, 2, 0.6, 0), (8, 1, 0.6, 3), (4, 10, 0.9, 0), (2, 2, 0.0, 0), (13, 1, 0.5, 1)])
def test_zelinski_postfilter(dsr, oracle, cuda, Cn, ptype, alpha, minFrames):
    """postfilter.cc:8-221,428-493: fp64 recursions of the auto/cross spectral densities in the reference's order, one thread per
    (utterance, bin).  Weights agree to 1e-6 relative (they leave as fp32), the filtered output to 1e-6 of its magnitude.
    The input s conj(wq_c) C + noise is NOT a source from the look direction: the filter time-aligns with conj(d_c) x_c (postfilter.cc:30-43), so s arrives as
    s conj(wq_c)^2 C, incoherent across the channels, and the weight sits on or near its floor.  This and the other post-filter tests of this file keep that input;
    tests/test_gpu_postfilter_kernels.py feeds aligned input (X_c = s d_c C + noise), which moves the weight through its whole range."""
    import torch
    rng = np.random.default_rng(5 + Cn)
    U, T, M = 3, 40, 64
    F = M // 2 + 1
    wq = (np.exp(-1j * rng.uniform(0, 6, (F, Cn))) / Cn).astype(np.complex128)
    s = rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))
    X = np.stack([s * np.conj(wq[:, c]) * Cn + 0.4 * (rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))) for c in range(Cn)], axis=1)
    X = X.astype(np.complex64); X[1, :, 7] = 0                           # an all-zero snapshot (0/0 in the weight: NaN, as in the reference)
    Y = np.einsum("fc,uctf->utf", np.conj(wq), X.astype(np.complex128)).astype(np.complex64)
    nfr = [T, T - 9, 1]
    pf = dsr.ZelinskiPostFilter(M, Cn, wq, alpha=alpha, type=ptype, minFrames=minFrames)
    got, w = pf.apply(torch.from_numpy(X).to(cuda), torch.from_numpy(Y).to(cuda), torch.tensor(nfr, dtype=torch.int32, device=cuda), want_weights=True)
    got, w = got.cpu().numpy(), w.cpu().numpy()
    for u in range(U):
        n = nfr[u]
        wo, ww = oracle.zelinski_postfilter(X[u, :, :n].astype(np.complex128), Y[u, :n].astype(np.complex128), wq, alpha, ptype, minFrames)
        fin = np.isfinite(ww)
        assert np.array_equal(fin, np.isfinite(w[u, :n]))
        np.testing.assert_allclose(w[u, :n][fin], ww[fin], rtol=1e-6)
        fo = np.isfinite(wo)
        assert np.array_equal(fo, np.isfinite(got[u, :n]))
        assert np.abs(got[u, :n][fo] - wo[fo]).max() <= 1e-6 * np.abs(wo[fo]).max()
        assert not got[u, n:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", [13, 64, 8])
def test_zelinski_postfilter_behind_its_beamformer(dsr, oracle, cuda, Cn):
    """dsr_zelinski_apply_bf = postfilter(X, bf(X)) (ZelinskiPostFilter::setBeamformer, postfilter.cc:376-384).  Arrays the filter streams (13 and 64 channels) get the
    beamformer's sum from the filter's own pass over the snapshots; 8 channels go through the two separate calls inside.  Ragged lengths, two blocks of a carried stream:
    the beamformer's output is dsr_bf_apply's (2e-6 of its largest value: the same sum, with and without fused multiply-adds), the filtered output the two-call result
    and the oracle's."""
    import torch
    rng = np.random.default_rng(40 + Cn)
    U, T, M = 3, 50, 64
    F = M // 2 + 1
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(0.5), np.float32(np.pi / 2), mp)
    bf = dsr.Beamformer(M, Cn); bf.calcArrayManifoldVectors(16000.0, delays); bf.select("ds")
    wq = bf.get(0)[:F]
    X = (rng.standard_normal((U, Cn, 2 * T, F)) + 1j * rng.standard_normal((U, Cn, 2 * T, F))).astype(np.complex64)
    nfr = [T, T - 9, 1]
    for u in range(U):
        X[u, :, nfr[u]:T] = 0; X[u, :, T + nfr[u]:] = 0
    Xd = torch.from_numpy(X).to(cuda); nd = torch.tensor(nfr, dtype=torch.int32, device=cuda)
    pfa = dsr.ZelinskiPostFilter(M, Cn, wq, alpha=0.7, type=2, minFrames=1); pfa.carry(True)
    pfb = dsr.ZelinskiPostFilter(M, Cn, wq, alpha=0.7, type=2, minFrames=1); pfb.carry(True)
    for blk in range(2):
        Xb = Xd[:, :, blk * T:(blk + 1) * T].contiguous()
        got, w, Yf = pfa.apply_bf(bf, Xb, nd, want_weights=True, want_bf_output=True)
        Y = bf.apply(Xb)
        ref, wr = pfb.apply(Xb, Y, nd, want_weights=True)
        assert float((Yf - Y).abs().max()) <= 2e-6 * float(Y.abs().max())
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) and float((w - wr).abs().max()) <= 1e-5
    u = 0                                                                    # the first block of the longest stream against the oracle
    pfc = dsr.ZelinskiPostFilter(M, Cn, wq, alpha=0.7, type=2, minFrames=1)
    got = pfc.apply_bf(bf, Xd[:, :, :T].contiguous(), nd).cpu().numpy()
    Yo = np.einsum("fc,ctf->tf", np.conj(wq), X[u, :, :T].astype(np.complex128))
    wo, _ = oracle.zelinski_postfilter(X[u, :, :T].astype(np.complex128), Yo, wq, 0.7, 2, 1)
    assert np.abs(got[u] - wo).max() <= 2e-5 * np.abs(wo).max()


@pytest.mark.gpu
def test_zelinski_postfilter_stream(dsr, oracle, cuda, protos, headset):
    """ZelinskiPostFilterPtr behind the stream protocol: analysis banks -> SubbandDS -> post-filter (setBeamformer)."""
    from dsr.btk import feature as F, modulated as Mo, beamformer as B, postfilter as P
    M, m, r, h, g = protos["M256-m4-r1"]
    Cn, n = 4, 6000
    x = synth.array_signal(n, Cn, seed=3)
    mp = synth.linear_array(Cn)
    delays = B.calcDelaysPolar2(np.deg2rad(30.0), np.pi / 2, mp)
    D = M >> r
    bf = B.SubbandDSPtr(fftLen=M)
    chans = []
    for c in range(Cn):
        sm = F.SampleFeaturePtr(blockLen=D, shiftLen=D, padZeros=True); sm.setSamples(x[c], 16000)
        a = Mo.OverSampledDFTAnalysisBankPtr(sm, h, M, m, r); chans.append(a); bf.setChannel(a)
    bf.calcArrayManifoldVectors(16000.0, delays)
    pf = P.ZelinskiPostFilterPtr(bf, M, alpha=0.7, type=2, minFrames=0)
    pf.setBeamformer(bf)
    rows = np.array([np.array(v) for v in pf])
    Xc = np.stack([oracle.analysis_bank(x[c], h, M, m, r, 0) for c in range(Cn)])          # [C][T][M]
    Fh = M // 2 + 1
    wq = bf._weights().get(0)[:Fh]
    Yo = np.einsum("fc,ctf->tf", np.conj(wq), Xc[:, :, :Fh])
    wo, _ = oracle.zelinski_postfilter(Xc[:, :, :Fh], Yo, wq, 0.7, 2, 0)
    assert rows.shape == (Xc.shape[1], M)
    sc = np.abs(wo).max()
    assert np.abs(rows[:, :Fh] - wo).max() < 5e-5 * sc                  # fp32 snapshots and beamformer output on the device
    assert np.abs(rows[:, Fh:] - np.conj(rows[:, 1:Fh - 1][:, ::-1])).max() < 1e-12      # conjugate mirror (postfilter.cc:194-196,213-215)
    # McCowanPostFilterPtr on the same chain
    mc = P.McCowanPostFilterPtr(bf, M, alpha=0.7, type=2, minFrames=1)
    mc.setDiffuseNoiseModel(mp, 16000.0); mc.divideAllNonDiagonalElements(0.01)
    mc.setBeamformer(bf)
    rows2 = np.array([np.array(v) for v in mc])
    R = oracle.pf_diffuse_noise_model(mp, M, 16000.0); off = ~np.eye(Cn, dtype=bool); R[:, off] = R[:, off] / (1.0 + np.float32(0.01))
    wo2, _ = oracle.mccowan_postfilter(Xc[:, :, :Fh], Yo, wq, R, 0.7, 2, 1, 0.99)
    assert np.abs(rows2[:, :Fh] - wo2).max() < 5e-5 * np.abs(wo2).max()


@pytest.mark.gpu
@pytest.mark.parametrize("Cn,ptype,alpha,minFrames,myu", [(8, 2, 0.6, 0, 0.01), (4, 1, 0.8, 2, 0.0), (6, 2, 0.0, 0, 0.1)])
def test_mccowan_postfilter(dsr, oracle, cuda, Cn, ptype, alpha, minFrames, myu):
    """postfilter.cc:568-945: McCowan's noise-coherence corrected estimate on top of the same density recursions."""
    import torch
    rng = np.random.default_rng(50 + Cn)
    U, T, M = 2, 30, 64
    F = M // 2 + 1
    mp = synth.linear_array(Cn)
    wq = (np.exp(-1j * rng.uniform(0, 6, (F, Cn))) / Cn).astype(np.complex128)
    s = rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))
    X = np.stack([s * np.conj(wq[:, c]) * Cn + 0.8 * (rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))) for c in range(Cn)], axis=1).astype(np.complex64)
    Y = np.einsum("fc,uctf->utf", np.conj(wq), X.astype(np.complex128)).astype(np.complex64)
    pf = dsr.McCowanPostFilter(M, Cn, wq, alpha=alpha, type=ptype, minFrames=minFrames, threshold=0.99)
    with pytest.raises(dsr.DsrError):
        pf.apply(torch.from_numpy(X).to(cuda), torch.from_numpy(Y).to(cuda))         # no noise coherence matrix yet (postfilter.cc:835-838)
    pf.setDiffuseNoiseModel(mp, 16000.0)
    R = oracle.pf_diffuse_noise_model(mp, M, 16000.0)
    if myu > 0:
        pf.divideAllNonDiagonalElements(myu)
        off = ~np.eye(Cn, dtype=bool); R[:, off] = R[:, off] / (1.0 + np.float32(myu))
    pf.setLevelOfDiagonalLoading(3, 0.05); R[3][np.eye(Cn, dtype=bool)] += np.float32(0.05)
    got, w = pf.apply(torch.from_numpy(X).to(cuda), torch.from_numpy(Y).to(cuda), want_weights=True)
    got, w = got.cpu().numpy(), w.cpu().numpy()
    for u in range(U):
        wo, ww = oracle.mccowan_postfilter(X[u].astype(np.complex128), Y[u].astype(np.complex128), wq, R, alpha, ptype, minFrames, 0.99)
        np.testing.assert_allclose(w[u], ww, rtol=1e-6)
        assert np.abs(got[u] - wo).max() <= 1e-6 * np.abs(wo).max()
    assert w.min() < 0.9                                               # the case is not saturated everywhere


@pytest.mark.gpu
@pytest.mark.parametrize("Cn,ptype,alpha,minFrames,fbinX1,load", [(8, 2, 0.6, 0, 0, 0.05), (4, 1, 0.8, 2, 5, 0.2), (6, 2, 0.0, 0, 40, 0.01)])
def test_lefkimmiatis_postfilter(dsr, oracle, cuda, Cn, ptype, alpha, minFrames, fbinX1, load):
    """postfilter.cc:948-1210 on McCowan's recursions: noise estimate sum (0.5(phi_ii+phi_jj) - phi_ij)/(1 - R_ij), divided by d^H pinv(R) d
    from bin fbinX1 on.  The pseudo-inverse is the reference's single-precision LINPACK csvdc on both sides (product: csrc/svd_linpack.cpp,
    oracle: orc_svd.c; both pinned bit for bit against the reference's own routine), so the weights agree as McCowan's do: 1e-6 (round 1 ran a
    double-precision Jacobi SVD on the product side and could only hold 2e-4)."""
    import torch
    rng = np.random.default_rng(70 + Cn)
    U, T, M = 2, 25, 64
    F = M // 2 + 1
    mp = synth.linear_array(Cn)
    wq = (np.exp(-1j * rng.uniform(0, 6, (F, Cn))) / Cn).astype(np.complex128)
    s = rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))
    X = np.stack([s * np.conj(wq[:, c]) * Cn + 0.8 * (rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))) for c in range(Cn)], axis=1).astype(np.complex64)
    Y = np.einsum("fc,uctf->utf", np.conj(wq), X.astype(np.complex128)).astype(np.complex64)
    pf = dsr.LefkimmiatisPostFilter(M, Cn, wq, minSV=1e-8, fbinX1=fbinX1, alpha=alpha, type=ptype, minFrames=minFrames, threshold=0.99)
    pf.setDiffuseNoiseModel(mp, 16000.0)
    pf.setAllLevelsOfDiagonalLoading(load)
    R = oracle.pf_diffuse_noise_model(mp, M, 16000.0)
    R[:, np.eye(Cn, dtype=bool)] += np.float32(load)
    lam = oracle.lefkimmiatis_lambda(R, wq, 1e-8)
    got, w = pf.apply(torch.from_numpy(X).to(cuda), torch.from_numpy(Y).to(cuda), want_weights=True)
    got, w = got.cpu().numpy(), w.cpu().numpy()
    for u in range(U):
        wo, ww = oracle.lefkimmiatis_postfilter(X[u].astype(np.complex128), Y[u].astype(np.complex128), wq, R, lam, alpha, ptype, minFrames, 0.99, fbinX1)
        np.testing.assert_allclose(w[u], ww, rtol=1e-6)
        assert np.abs(got[u] - wo).max() <= 1e-6 * np.abs(wo).max()
    assert 0.0001 < w.min() < 0.9 or w.max() > 0.0001
    # a rank-deficient matrix (bin 0 of the unloaded diffuse model is all ones): a singular value under the floor makes the reference fall
    # back to the identity for that bin (postfilter.cc:989-991), Lambda = d^H d; the floor is chosen above single-precision round-off
    pf2 = dsr.LefkimmiatisPostFilter(M, Cn, wq, minSV=1e-4, fbinX1=0, alpha=alpha, type=ptype)
    pf2.setDiffuseNoiseModel(mp, 16000.0)
    R2 = oracle.pf_diffuse_noise_model(mp, M, 16000.0)
    lam2 = oracle.lefkimmiatis_lambda(R2, wq, 1e-4)
    assert abs(lam2[0] - np.vdot(wq[0], wq[0])) < 1e-12
    _, w2 = pf2.apply(torch.from_numpy(X).to(cuda), torch.from_numpy(Y).to(cuda), want_weights=True)
    _, ww2 = oracle.lefkimmiatis_postfilter(X[0].astype(np.complex128), Y[0].astype(np.complex128), wq, R2, lam2, alpha, ptype, 0, 0.99, 0)
    np.testing.assert_allclose(w2.cpu().numpy()[0][:, 0], ww2[:, 0], rtol=1e-5)


@pytest.mark.gpu
def test_highpass_filter_stream(dsr, cuda):
    """postfilter.cc:1222-1261: bins below fftLen * cutOffFreq / sampleRate are zero (and bin 0, which the reference never writes), the rest
    passes with its mirror; a cut-off bin of 0 would make the reference write outside its vector and is refused."""
    from dsr.btk import stream as S, postfilter as P
    rng = np.random.default_rng(3)
    T, M = 7, 32
    F = M // 2 + 1

    class Frames(object):
        def __init__(self, a):
            self.a = a

        def size(self):
            return self.a.shape[1]

        def __iter__(self):
            return iter(self.a)

    half = rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))
    full = np.zeros((T, M), np.complex128); full[:, :F] = half; full[:, F:] = np.conj(half[:, 1:F - 1][:, ::-1])
    src = S.PyVectorComplexFeatureStreamPtr(Frames(full))
    hp = P.highPassFilterPtr(src, 1600.0, 16000)                       # cut bin = 32 * 1600 / 16000 = 3
    rows = np.array([np.array(v) for v in hp])
    exp = full.copy(); exp[:, :3] = 0.0; exp[:, M - 2:] = 0.0
    assert rows.shape == exp.shape and np.array_equal(rows, exp)
    with pytest.raises(dsr.DsrError):
        P.highPassFilterPtr(src, 100.0, 16000)                         # cut bin 0


# ------------------------------------------------------------------------------------------- single-channel WPE
@pytest.mark.gpu
@pytest.mark.parametrize("lowerN,upperN,iters,loadDb,bw", [(2, 9, 2, -20.0, 0.0), (1, 16, 3, -10.0, 0.0), (3, 6, 1, -30.0, 4000.0), (0, 3, 2, -20.0, 0.0)])
def test_wpe_single(dsr, oracle, cuda, lowerN, upperN, iters, loadDb, bw):
    """dereverberation.cc:28-300: per (utterance, subband) weighted correlation matrix, Cholesky, prediction filter, fp64 on the device;
    terms are weighted with 1/theta_n (one division per frame): 1e-8 relative on the filters, 1e-6 of the magnitude on the fp32 output."""
    import torch
    rng = np.random.default_rng(lowerN + upperN)
    U, N, M = 2, 160, 32
    F = M // 2 + 1
    s = rng.standard_normal((U, N, F)) + 1j * rng.standard_normal((U, N, F))
    for k in range(1, 12):
        s[:, k:] += 0.6 ** k * np.roll(s, k, axis=1)[:, k:] * np.exp(1j * k)          # a decaying tail
    Y = s.astype(np.complex64)
    nfr = [N, N - 33]
    out, gn = dsr.wpe_single(torch.from_numpy(Y).to(cuda), M, lowerN, upperN, iters, loadDb, bw, 16000.0,
                             nframes=torch.tensor(nfr, dtype=torch.int32, device=cuda), want_filters=True)
    out, gn = out.cpu().numpy(), gn.cpu().numpy()
    for u in range(U):
        n = nfr[u]
        full = np.zeros((n, M), np.complex128); full[:, :F] = Y[u, :n]; full[:, F:] = np.conj(Y[u, :n, 1:F - 1][:, ::-1])
        wo, wg = oracle.wpe_single(full, lowerN, upperN, iters, loadDb, bw, 16000.0)
        np.testing.assert_allclose(gn[u], wg[:F], rtol=1e-8, atol=1e-12)
        assert np.abs(out[u, :n] - wo[:, :F]).max() <= 1e-6 * np.abs(wo).max()
        assert not out[u, n:].any()
        assert np.abs(wo[:, F:] - np.conj(wo[:, 1:F - 1][:, ::-1])).max() < 1e-9       # the mirrored half of the reference's output is redundant
    # the operator behind the stream protocol: a Python iterable of frames as the source (pyStream.h:44-152)
    from dsr.btk import stream as S, dereverberation as Dv

    class Frames(object):
        def __init__(self, a):
            self.a = a

        def size(self):
            return self.a.shape[1]

        def __iter__(self):
            return iter(self.a)

    full = np.zeros((N, M), np.complex128); full[:, :F] = Y[0]; full[:, F:] = np.conj(Y[0, :, 1:F - 1][:, ::-1])
    src = S.PyVectorComplexFeatureStreamPtr(Frames(full))
    rows = np.array([np.array(v) for v in Dv.SingleChannelWPEDereverberationFeaturePtr(src, lowerN, upperN, iters, loadDb, bw, 16000.0)])
    wo, _ = oracle.wpe_single(full, lowerN, upperN, iters, loadDb, bw, 16000.0)
    assert rows.shape == wo.shape and np.abs(rows - wo).max() <= 2e-6 * np.abs(wo).max()


@pytest.mark.gpu
@pytest.mark.parametrize("Cn,lowerN,upperN,iters,loadDb,bw,fc", [(3, 2, 5, 2, -20.0, 0.0, -1), (2, 1, 8, 2, -10.0, 0.0, 1), (4, 3, 4, 1, -30.0, 4000.0, 0)])
def test_wpe_multi(dsr, oracle, cuda, Cn, lowerN, upperN, iters, loadDb, bw, fc):
    """dereverberation.cc:281-586: stacked lags [channel][lag], per-channel theta_n / weighted correlation matrix / Cholesky / filter, fp64 on the
    device (1/theta_n weighting as in the single-channel kernel); getOutput's filter choice (own channel, or the first asker's for all)."""
    import torch
    rng = np.random.default_rng(Cn + lowerN + upperN)
    U, N, M = 2, 120, 32
    F = M // 2 + 1
    s = rng.standard_normal((U, 1, N, F)) + 1j * rng.standard_normal((U, 1, N, F))
    Y = np.zeros((U, Cn, N, F), np.complex128)
    for c in range(Cn):
        Y[:, c] = s[:, 0] * np.exp(1j * c) + 0.1 * (rng.standard_normal((U, N, F)) + 1j * rng.standard_normal((U, N, F)))
        for k in range(1, 10):
            Y[:, c, k:] += (0.55 + 0.05 * c) ** k * np.roll(s[:, 0], k, axis=1)[:, k:] * np.exp(1j * k * (c + 1))
    Y = Y.astype(np.complex64)
    nfr = [N, N - 21]
    out, gn = dsr.wpe_multi(torch.from_numpy(Y).to(cuda), M, lowerN, upperN, iters, loadDb, bw, 16000.0,
                            nframes=torch.tensor(nfr, dtype=torch.int32, device=cuda), filterChan=fc)
    out, gn = out.cpu().numpy(), gn.cpu().numpy()

    def full_of(a):            # [C][n][F] -> [C][n][M] with the mirrored half the reference's streams carry
        f = np.zeros(a.shape[:2] + (M,), np.complex128); f[:, :, :F] = a; f[:, :, F:] = np.conj(a[:, :, 1:F - 1][:, :, ::-1]); return f
    for u in range(U):
        n = nfr[u]
        wo, wg = oracle.wpe_multi(full_of(Y[u, :, :n]), lowerN, upperN, iters, loadDb, bw, 16000.0, filterChan=fc)
        np.testing.assert_allclose(gn[u], wg[:, :F], rtol=2e-7, atol=1e-10)
        assert np.abs(out[u, :, :n] - wo[:, :, :F]).max() <= 2e-6 * np.abs(wo).max()
        assert not out[u, :, n:].any()
    # the operators: a shared source, one feature per channel, pulled channel 0 first -> every channel through channel 0's filter
    from dsr.btk import stream as S, dereverberation as Dv

    class Frames(object):
        def __init__(self, a):
            self.a = a

        def size(self):
            return self.a.shape[1]

        def __iter__(self):
            return iter(self.a)

    fu = full_of(Y[0])
    src = Dv.MultiChannelWPEDereverberationPtr(M, Cn, lowerN, upperN, iters, loadDb, bw, 16000.0)
    for c in range(Cn):
        src.setInput(S.PyVectorComplexFeatureStreamPtr(Frames(fu[c])))
    with pytest.raises(dsr.DsrError):
        src.setInput(S.PyVectorComplexFeatureStreamPtr(Frames(fu[0])))                 # Channel capacity exceeded (dereverberation.cc:359-360)
    feats = [Dv.MultiChannelWPEDereverberationFeaturePtr(src, c) for c in range(Cn)]
    rows = [[] for _ in range(Cn)]
    for t in range(N):
        for c in range(Cn):
            rows[c].append(np.array(feats[c].next(t)))
    with pytest.raises(StopIteration):
        feats[0].next(N)
    wo, _ = oracle.wpe_multi(fu, lowerN, upperN, iters, loadDb, bw, 16000.0, filterChan=0)
    got = np.array(rows)
    assert got.shape == wo.shape and np.abs(got - wo).max() <= 4e-6 * np.abs(wo).max()


# ------------------------------------------------------------------------------------------- adaptive beamformers
@pytest.mark.gpu
@pytest.mark.parametrize("Cn,myu,sigma2,qc,alpha,mode", [(4, 0.9, 0.0, 0, -1.0, "gsc"), (8, 0.95, 0.01, 2, 0.05, "gsc"), (5, 0.8, 0.001, 1, 0.3, "gsc_norm")])
def test_gsc_rls(dsr, oracle, cuda, Cn, myu, sigma2, qc, alpha, mode):
    """beamformer.cc:1497-1698: GSC output with the weights as they stand, then the recursive-least-squares update of the precision matrix and
    the active weights per (utterance, bin), fp64 on the device; summation order of the small matrix-vector products differs from CBLAS:
    1e-9 relative on the final active weights, 1e-6 of the magnitude on the fp32 output."""
    import torch
    rng = np.random.default_rng(90 + Cn)
    U, T, M = 2, 60, 32
    F = M // 2 + 1
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(0.4), np.float32(np.pi / 2), mp)
    bf = dsr.Beamformer(M, Cn); bf.calcGSCWeights(16000.0, delays); bf.select(mode); bf.rlsConfig(myu, sigma2)
    s = rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))
    wq = bf.get(0); B = bf.get(3)[:F]
    X = np.stack([s * np.conj(wq[:F, c]) * Cn + 0.7 * (rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))) for c in range(Cn)], axis=1).astype(np.complex64)
    with pytest.raises(dsr.DsrError):
        bf.gsc_rls(torch.from_numpy(X).to(cuda))                           # no precision matrix yet (beamformer.cc:1566-1569)
    bf.initPrecisionMatrix(0.01)
    if qc:
        bf.setQuadraticConstraint(alpha, qc)
    Y, wa = bf.gsc_rls(torch.from_numpy(X).to(cuda))
    Y, wa = Y.cpu().numpy(), wa.cpu().numpy()

    def full_of(a):            # [C][T][F] -> [C][T][M]
        f = np.zeros(a.shape[:2] + (M,), np.complex128); f[:, :, :F] = a; f[:, :, F:] = np.conj(a[:, :, 1:F - 1][:, :, ::-1]); return f
    for u in range(U):
        Yo, wao = oracle.gsc_rls(full_of(X[u]), wq, B, myu, sigma2, 0.01, alpha, qc, True, mode == "gsc_norm")
        np.testing.assert_allclose(wa[u][1:], wao[1:], rtol=1e-8, atol=1e-12)
        assert np.abs(Y[u] - Yo[:, :F]).max() <= 2e-6 * np.abs(Yo).max()
    fixed = dsr.Beamformer(M, Cn); fixed.calcGSCWeights(16000.0, delays); fixed.select(mode)
    Y0 = fixed.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()
    assert np.abs(Y[:, 0] - Y0[:, 0]).max() <= 2e-6 * np.abs(Y0).max()   # the first frame still has zero active weights
    if qc != 1:                                                            # (a forced norm of the active weights need not help)
        assert np.abs(Y[:, -20:]).mean() < np.abs(Y0[:, -20:]).mean()    # the adaptation takes noise out
    bf.updateActiveWeightVecotrs(False)                                   # adaptation off: the fixed GSC
    Y1, _ = bf.gsc_rls(torch.from_numpy(X).to(cuda))
    assert np.abs(Y1.cpu().numpy() - Y0).max() <= 2e-6 * np.abs(Y0).max()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [1, 2])
def test_mvdr_gsc(dsr, oracle, cuda, which):
    """SubbandMVDRGSC (beamformer.cc:2637-2817): w_mvdr - B wa with the blocking matrices of the delay-and-sum vector (1) or of the MVDR
    vector (2), upgradeBlockingMatrix (the cached B wa stays), blockingMatrixOutput -- against the oracle's own pieces."""
    import torch
    rng = np.random.default_rng(40 + which)
    Cn, U, T, M = 6, 2, 12, 32
    F = M // 2 + 1
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(0.6), np.float32(np.pi / 2), mp)
    bf = dsr.Beamformer(M, Cn); bf.calcArrayManifoldVectors(16000.0, delays); bf.setDiffuseNoiseModel(mp, 16000.0, 343740.0)
    bf.divideAllNonDiagonalElements(0.01)
    if which == 2:
        assert bf.calcBlockingMatrix2() is False                            # no MVDR weights yet
    bf.calcMVDRWeights(16000.0, 1e-8); bf.select("mvdr_gsc")
    assert (bf.calcBlockingMatrix1(16000.0, delays) if which == 1 else bf.calcBlockingMatrix2()) is True
    mv = bf.get(1); wq = bf.get(0); B = bf.get(3)
    for f in range(1, F):
        ref, ok = oracle.blocking_matrix(wq[f] if which == 1 else mv[f])
        assert ok and np.abs(B[f] - ref).max() < 1e-12
        if which == 2:
            assert np.abs(wq[f] - mv[f]).max() == 0.0                       # the MVDR vector became the quiescent vector
    wa = (rng.standard_normal((F, Cn - 1)) + 1j * rng.standard_normal((F, Cn - 1))) * 0.1
    for f in range(1, F):
        bf.setActiveWeights_f(f, np.stack([wa[f].real, wa[f].imag], axis=1).reshape(-1))
    X = (rng.standard_normal((U, Cn, T, F)) + 1j * rng.standard_normal((U, Cn, T, F))).astype(np.complex64)
    Y = bf.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()

    def full_of(a):
        f = np.zeros(a.shape[:2] + (M,), np.complex128); f[:, :, :F] = a; f[:, :, F:] = np.conj(a[:, :, 1:F - 1][:, :, ::-1]); return f
    mvfull = np.zeros((M, Cn), complex); mvfull[:F] = mv
    waz = wa.copy(); waz[0] = 0.0
    for u in range(U):
        Yo = oracle.gsc_apply(full_of(X[u]), mvfull, B[:F], waz)
        assert np.abs(Y[u] - Yo[:, :F]).max() <= 2e-6 * np.abs(Yo).max()
    # upgradeBlockingMatrix: new matrices orthogonal to wq - wl; the output does not move until the active weights are set again
    wl = np.einsum("fcj,fj->fc", B[:F], waz)
    bf.upgradeBlockingMatrix()
    B2 = bf.get(3)
    for f in range(1, F):
        ref, ok = oracle.blocking_matrix(wq[f] - wl[f])
        assert ok and np.abs(B2[f] - ref).max() < 1e-12
    Y2 = bf.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()
    assert np.array_equal(Y2, Y)
    Z = bf.blockingMatrixOutput(torch.from_numpy(X).to(cuda), 1).cpu().numpy()
    ref = np.einsum("fc,uctf->utf", np.conj(B2[:F, :, 1]), X.astype(np.complex128))
    assert np.abs(Z - ref).max() <= 2e-6 * np.abs(ref).max()
    bf.zeroActiveWeights()
    Y3 = bf.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()
    bm = dsr.Beamformer(M, Cn); bm.calcArrayManifoldVectors(16000.0, delays); bm.setDiffuseNoiseModel(mp, 16000.0, 343740.0)
    bm.divideAllNonDiagonalElements(0.01); bm.calcMVDRWeights(16000.0, 1e-8); bm.select("mvdr")
    assert np.abs(Y3 - bm.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()).max() <= 1e-6 * np.abs(Y3).max()   # zero active weights: plain MVDR


@pytest.mark.gpu
def test_mvdr_gsc_stream(dsr, oracle, cuda):
    """SubbandMVDRGSCPtr behind the stream protocol (usage order of beamformer.h:396-402)."""
    from dsr.btk import stream as S, beamformer as Bm
    rng = np.random.default_rng(23)
    Cn, T, M = 4, 9, 16
    F = M // 2 + 1
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(0.2), np.float32(np.pi / 2), mp)

    class Frames(object):
        def __init__(self, a):
            self.a = a

        def size(self):
            return self.a.shape[1]

        def __iter__(self):
            return iter(self.a)

    half = (rng.standard_normal((Cn, T, F)) + 1j * rng.standard_normal((Cn, T, F))).astype(np.complex64)
    full = np.zeros((Cn, T, M), np.complex128); full[:, :, :F] = half; full[:, :, F:] = np.conj(half[:, :, 1:F - 1][:, :, ::-1])
    bf = Bm.SubbandMVDRGSCPtr(fftLen=M, halfBandShift=False)
    for c in range(Cn):
        bf.setChannel(S.PyVectorComplexFeatureStreamPtr(Frames(full[c])))
    bf.calcArrayManifoldVectors(16000.0, delays); bf.setDiffuseNoiseModel(mp, 16000.0); bf.setAllLevelsOfDiagonalLoading(0.01)
    assert bf.calcBlockingMatrix2() is False
    bf.calcMVDRWeights(16000.0, 1e-8)
    assert bf.calcBlockingMatrix2() is True
    wa = (rng.standard_normal((F, Cn - 1)) + 1j * rng.standard_normal((F, Cn - 1))) * 0.2
    for f in range(1, F):
        bf.setActiveWeights_f(f, np.stack([wa[f].real, wa[f].imag], axis=1).reshape(-1))
    rows = np.array([np.array(v) for v in bf])
    w = bf._weights(); mv = w.get(1); B = w.get(3)[:F]
    mvfull = np.zeros((M, Cn), complex); mvfull[:F] = mv; wa[0] = 0.0
    Yo = oracle.gsc_apply(full, mvfull, B, wa)
    assert rows.shape == Yo.shape and np.abs(rows - Yo).max() <= 4e-6 * np.abs(Yo).max()
    # SubbandOrthogonalizer on the same beamformer: channel 0 = its output, channel k = column k-1 of the blocking matrices (lower bins;
    # the upper bins keep the mirror of the beamformer's output, as the reference's shared vector does)
    o0 = np.array([np.array(v) for v in Bm.SubbandOrthogonalizerPtr(bf, 0)])
    assert np.array_equal(o0, rows)
    o2 = np.array([np.array(v) for v in Bm.SubbandOrthogonalizerPtr(bf, 2)])
    ref = np.einsum("fc,ctf->tf", np.conj(B[:, :, 1]), full[:, :, :F])
    assert np.abs(o2[:, :F] - ref).max() <= 4e-6 * np.abs(ref).max() and np.array_equal(o2[:, F:], rows[:, F:])


@pytest.mark.gpu
def test_gsc_rls_stream(dsr, oracle, cuda):
    """SubbandGSCRLSPtr (beamformer.i:227-253) behind the stream protocol: setChannel / calcGSCWeights / initPrecisionMatrix / iteration."""
    from dsr.btk import stream as S, beamformer as Bm
    rng = np.random.default_rng(17)
    Cn, T, M = 4, 40, 32
    F = M // 2 + 1
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(0.3), np.float32(np.pi / 2), mp)

    class Frames(object):
        def __init__(self, a):
            self.a = a

        def size(self):
            return self.a.shape[1]

        def __iter__(self):
            return iter(self.a)

    half = (rng.standard_normal((Cn, T, F)) + 1j * rng.standard_normal((Cn, T, F))).astype(np.complex64)
    full = np.zeros((Cn, T, M), np.complex128); full[:, :, :F] = half; full[:, :, F:] = np.conj(half[:, :, 1:F - 1][:, :, ::-1])
    bf = Bm.SubbandGSCRLSPtr(fftLen=M, halfBandShift=False, myu=0.9, sigma2=0.001)
    for c in range(Cn):
        bf.setChannel(S.PyVectorComplexFeatureStreamPtr(Frames(full[c])))
    bf.calcGSCWeights(16000.0, delays)
    with pytest.raises(dsr.DsrError):
        bf.next()                                                           # no precision matrix yet
    bf.reset()
    bf.initPrecisionMatrix(0.02)
    bf.setQuadraticConstraint(0.5, 2)
    rows = np.array([np.array(v) for v in bf])
    w = bf._weights(); wq = w.get(0); B = w.get(3)[:F]
    Yo, _ = oracle.gsc_rls(full, wq, B, 0.9, 0.001, 0.02, 0.5, 2, True, False)
    assert rows.shape == Yo.shape and np.abs(rows - Yo).max() <= 4e-6 * np.abs(Yo).max()


# ------------------------------------------------------------------------------------------- BASELINE sizes
@pytest.mark.gpu
def test_gmm_full_size(dsr, oracle, cuda):
    """BASELINE config 3 at size (39-dim x 4096 Gaussians as 1024 codebooks of 4, 200 000 frames): a sample of frames bit-exact against the
    oracle, every frame independent of its place in the batch (a permutation of the frames permutes the rows), scores finite."""
    import torch
    K, R, D, N = 1024, 4, 39, 200000
    m = synth.gmm_model(K, R, D, seed=12)
    gm = dsr.Gmm(**m)
    g = torch.Generator(device=cuda); g.manual_seed(3)
    x = torch.randn((N, D), generator=g, device=cuda) * 1.5
    sc, am = gm.score(x, mode=0)
    assert bool(torch.isfinite(sc).all())
    perm = torch.randperm(N, generator=g, device=cuda)
    sc2, am2 = gm.score(x[perm].contiguous(), mode=0)
    assert torch.equal(sc2, sc[perm]) and torch.equal(am2, am[perm])
    pick = np.concatenate([np.arange(0, 300), np.arange(N - 300, N), np.random.default_rng(1).integers(0, N, 400)])
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    ref, arg = oracle.gmm_score_opt(cb, m["val"], x[torch.from_numpy(pick).to(cuda)].cpu().numpy())
    assert np.array_equal(sc.cpu().numpy()[pick].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(am.cpu().numpy()[pick].astype(np.int32), arg)
    sc3, am3 = gm.score(x[:50000].contiguous(), mode=2)                  # the MFMA path: mode 0's nearest Gaussian on every frame, the cost to rel 2e-6
    assert torch.equal(am3, am[:50000]) and float((sc3 - sc[:50000]).abs().max() / sc[:50000].abs().max()) < 2e-6


@pytest.mark.gpu
def test_viterbi_full_size(dsr, oracle, cuda, monkeypatch):
    """BASELINE config 4 at size (50 000 states / ~200 000 arcs, 1024 distributions, beam tuned to thousands of active tokens): 300 frames
    bit-exact against the oracle; register path, memory path and every position in a batch larger than the slot count give identical results."""
    import torch
    arcs, fin = synth.random_wfst(50000, 1024, seed=21, outdeg=4, eps_frac=0.1, out_frac=0.05, nWords=5000, nFinal=50)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    gm = dsr.Gmm(**synth.gmm_model(1024, 4, 39, seed=12))
    T, U = 300, 4
    g = torch.Generator(device=cuda); g.manual_seed(5)
    f = torch.randn((U, T + 16, 39), generator=g, device=cuda)
    f = torch.nn.functional.avg_pool1d(f.transpose(1, 2), 9, 1).transpose(1, 2)[:, :T].contiguous() * 3.0
    sc = gm.score(f.reshape(-1, 39), mode=0, want_argmin=False)[0].reshape(U, T, 1024)
    beam = 50.0
    dec = dsr.Decoder(beam=beam, lmScale=12.0, maxActive=65536); dec.set(gd)
    out = dec.decode_batch(sc, maxPath=1024)
    assert np.mean([o["activeHypos"] / T for o in out]) > 1500, "the case is meant to keep thousands of tokens alive"
    assert all(o["registerFrames"] > 0.9 * T for o in out)
    sch = sc.cpu().numpy()
    for u in range(2):
        ro = go.decode(sch[u], beam=beam, lmScale=12.0)
        assert ro["rc"] == 0
        _check_decode(ro, out[u])
    monkeypatch.setenv("DSR_VITERBI_NOFAST", "1")
    dec2 = dsr.Decoder(beam=beam, lmScale=12.0, maxActive=65536); dec2.set(gd)
    monkeypatch.delenv("DSR_VITERBI_NOFAST")
    out2 = dec2.decode_batch(sc, maxPath=1024)
    big = sc.repeat(80, 1, 1)                                              # 320 utterances: more than the 256 decoder slots
    out3 = dec.decode_batch(big, maxPath=1024)
    keys = ["score", "ac", "lm", "status", "activeHypos", "placements", "maxActive", "reachedFinal", "frames"]
    for u in range(U):
        assert all(out[u][k] == out2[u][k] for k in keys) and np.array_equal(out[u]["arcs"], out2[u]["arcs"]) and out2[u]["registerFrames"] == 0
    for v in range(320):
        assert all(out[v % U][k] == out3[v][k] for k in keys) and np.array_equal(out[v % U]["words"], out3[v]["words"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ds", "gsc", "gsc_norm"])
def test_beamformer_half_band_shift(dsr, oracle, cuda, mode):
    """halfBandShift == true apply for SubbandDS / SubbandGSC (beamformer.cc:544-555,1159-1175,1321-1330): all M bins on their own,
    steering half a bin up; SubbandMVDR refuses the flag (:2324-2327) and SubbandGSCRLS::next says "not yet implemented" (:1580-1583), as here."""
    import torch
    M, Cn, T, U = 64, 6, 9, 2
    mp = synth.linear_array(Cn)
    delays = dsr.calcDelaysPolar2(np.float32(0.5), np.float32(1.3), mp)
    bf = dsr.Beamformer(M, Cn, halfBandShift=True)
    if mode == "ds":
        bf.calcArrayManifoldVectors(16000.0, delays)
    else:
        bf.calcGSCWeights(16000.0, delays)
    bf.select(mode)
    wq = bf.get(0)
    assert np.abs(wq - oracle.calc_mainlobe_hbs(16000.0, delays, M)).max() < 1e-15
    rng = np.random.default_rng(77)
    X = (rng.standard_normal((U, Cn, T, M)) + 1j * rng.standard_normal((U, Cn, T, M))).astype(np.complex64)      # all M bins, no symmetry assumed
    B = wa = None
    if mode != "ds":
        B = bf.get(3); wa = (rng.standard_normal((M, Cn - 1)) + 1j * rng.standard_normal((M, Cn - 1))) * 0.05
        for f in range(M):
            bf.setActiveWeights_f(f, np.ascontiguousarray(wa[f]).view(np.float64))
        for f in (0, 5, M - 1):
            Bo, ok = oracle.blocking_matrix(wq[f]); assert ok and np.abs(B[f] - Bo).max() < 1e-12
    assert bf.bins() == M
    Y = bf.apply(torch.from_numpy(X).to(cuda)).cpu().numpy()
    assert Y.shape == (U, T, M)
    for u in range(U):
        Yo = oracle.apply_all_bins(X[u].astype(np.complex128), wq, B, wa, mode == "gsc_norm")
        assert np.abs(Y[u] - Yo).max() <= 2e-5 * np.abs(Yo).max() * np.sqrt(Cn)
    mv = dsr.Beamformer(M, Cn, halfBandShift=True); mv.calcArrayManifoldVectors(16000.0, delays); mv.setDiffuseNoiseModel(mp, 16000.0)
    mv.calcMVDRWeights(16000.0); mv.select("mvdr")
    with pytest.raises(dsr.DsrError) as e:
        mv.apply(torch.from_numpy(X).to(cuda))
    assert e.value.status == 2                                            # jallocation_error "halfBandShift==true is not yet supported"
    if mode == "gsc":
        bf.rlsConfig(0.9, 0.0); bf.initPrecisionMatrix(0.01)
        with pytest.raises(dsr.DsrError):
            bf.gsc_rls(torch.from_numpy(X[:, :, :, :M // 2 + 1].copy()).to(cuda))       # "not yet implemented"


@pytest.mark.gpu
@pytest.mark.parametrize("series_in_memory", [False, True])
def test_wpe_multi_at_benchmark_size(dsr, oracle, cuda, monkeypatch, series_in_memory):
    """Multi-channel WPE at the benchmark's own utterance size: 8 channels x 1257 frames x 10 taps -- an 80 x 80 normal matrix per (subband, channel),
    kept as a packed triangle next to the subband's series of all channels (145 KB of LDS; the square layout needed 192 KB and was refused).  Second case:
    the series read from the transposed copy in memory instead of LDS (what larger tap counts fall back to).  Few subbands: the oracle's cost is per
    subband and the limit being tested is per (channels, frames, taps).  dereverberation.cc:397-620."""
    import torch
    if series_in_memory:
        monkeypatch.setenv("DSR_WPE_SERIES_MEM", "1")
    rng = np.random.default_rng(77)
    U, Cn, N, M = 1, 8, 1257, 8
    F = M // 2 + 1
    lowerN, upperN = 2, 11
    s = rng.standard_normal((U, 1, N, F)) + 1j * rng.standard_normal((U, 1, N, F))
    Y = np.zeros((U, Cn, N, F), np.complex128)
    for c in range(Cn):
        Y[:, c] = s[:, 0] * np.exp(1j * c) + 0.1 * (rng.standard_normal((U, N, F)) + 1j * rng.standard_normal((U, N, F)))
        for k in range(1, 14):
            Y[:, c, k:] += (0.5 + 0.04 * c) ** k * np.roll(s[:, 0], k, axis=1)[:, k:] * np.exp(1j * k * (c + 1))
    Y = Y.astype(np.complex64)
    out, gn = dsr.wpe_multi(torch.from_numpy(Y).to(cuda), M, lowerN, upperN, 2, -20.0, 0.0, 16000.0, filterChan=-1)
    out, gn = out.cpu().numpy(), gn.cpu().numpy()
    f = np.zeros((Cn, N, M), np.complex128); f[:, :, :F] = Y[0]; f[:, :, F:] = np.conj(Y[0][:, :, 1:F - 1][:, :, ::-1])
    wo, wg = oracle.wpe_multi(f, lowerN, upperN, 2, -20.0, 0.0, 16000.0, filterChan=-1)
    assert np.isfinite(gn).all()
    np.testing.assert_allclose(gn[0], wg[:, :F], rtol=2e-6, atol=1e-9)
    assert np.abs(out[0] - wo[:, :, :F]).max() <= 2e-6 * np.abs(wo).max()
    # dereverberation does something: the late part of the response is gone from the output's autocorrelation at the predicted lags
    def late(a):
        return np.mean([np.abs(np.vdot(a[0, :-k, 1], a[0, k:, 1])) for k in range(3, 10)]) / np.real(np.vdot(a[0, :, 1], a[0, :, 1]))
    assert late(out[0]) < 0.9 * late(Y[0].astype(np.complex128))


@pytest.mark.gpu
@pytest.mark.parametrize("K,R,D", [(64, 4, 39), (7, 5, 13), (3, 32, 40)])
def test_gmm_log_lhood(dsr, oracle, cuda, K, R, D):
    """CodebookBasic::logLhood (codebookBasic.cc:557-609) through dsr_gmm_log_lhood: the nearest Gaussian of _scoreOpt, finished as that method does
    (0.5 * min + val[argmin], or 0.5 * min with val == NULL; no codebook scale) -- bit exact."""
    import ctypes as C
    import torch
    m = synth.gmm_model(K, R, D, seed=21)
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((1500, D)) * 1.3).astype(np.float32)
    gm = dsr.Gmm(**m); xd = torch.from_numpy(x).to(cuda)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    L = dsr.load()
    for useVal in (1, 0):
        sc = torch.empty((x.shape[0], K), dtype=torch.float32, device=cuda); am = torch.zeros((x.shape[0], K), dtype=torch.uint8, device=cuda)
        dsr.check(L.dsr_gmm_log_lhood(gm.h, C.c_void_p(xd.data_ptr()), x.shape[0], useVal, C.c_void_p(sc.data_ptr()), C.c_void_p(am.data_ptr()), dsr.cur_stream()))
        ref, arg = oracle.gmm_log_lhood(cb, m["val"] if useVal else None, x)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(am.cpu().numpy().astype(np.int32), arg)
    s0, a0 = gm.score(xd, mode=0)
    assert torch.equal(a0, am)                                             # the same Gaussian as _scoreOpt
    # (with unit codebook scale the two finishes are the same number: halving commutes with the rounding of the sum, 0.5 (min + 2 val) == 0.5 min + val)
    ref1, _ = oracle.gmm_log_lhood(cb, m["val"], x)
    assert np.array_equal(s0.cpu().numpy().view(np.uint32), ref1.view(np.uint32))
    # a codebook scale enters _scoreOpt only
    scale = np.full(K, 1.5, np.float32)
    gs = dsr.Gmm(scale=scale, **m)
    s1, _ = gs.score(xd, mode=0)
    sc2 = torch.empty((x.shape[0], K), dtype=torch.float32, device=cuda)
    dsr.check(L.dsr_gmm_log_lhood(gs.h, C.c_void_p(xd.data_ptr()), x.shape[0], 1, C.c_void_p(sc2.data_ptr()), None, dsr.cur_stream()))
    assert np.array_equal(sc2.cpu().numpy().view(np.uint32), ref1.view(np.uint32)) and not torch.equal(s1, sc2)


@pytest.mark.gpu
def test_decoder_small_boundary_methods(dsr, cuda):
    """_Decoder::setTokenMemoryLimit (decoder.h:396: accepted and kept, there is no token pool here) and writeCTM (decoder.h:398-401: the shipped
    base-template body constructs a j_error without throwing it -- a no-op)."""
    from dsr.asr import decoder as D
    L = dsr.load()
    dec = dsr.Decoder(beam=50.0, lmScale=12.0, maxActive=1024, streams=1)
    dsr.check(L.dsr_decoder_set_token_memory_limit(dec.h, 123456))
    assert L.dsr_decoder_token_memory_limit(dec.h) == 123456
    d = D.DecoderFlyWeightPtr.__new__(D.DecoderFlyWeightPtr)
    assert D.DecoderFlyWeightPtr.writeCTM(d, "conv", "A", "spk", "utt", 0.0, 1.0, "/nonexistent/dir/file.ctm") is None
