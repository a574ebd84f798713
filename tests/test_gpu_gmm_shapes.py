"""Mode 2 of dsr_gmm_score (csrc/k_gmm_mfma.hip, csrc/k_gmm_sp.hip) at every template instance its dispatch can select, on frames that sit on near
ties (tests/gmm_cases.py; tests/test_gmm_cases_cpu.py shows that trusting the expanded form there picks the wrong Gaussian on 30-50 % of them).

Every case asserts the contract of the kernel's header:
  * mode 0's scores and argmins are the oracle's (_scoreOpt) bits;
  * mode 2's argmin is the oracle's on EVERY frame;
  * a mode-2 score is mode 0's bits, or lies within 0.5 |scale_k| (2 dimN + 3) 2^-24 S_n of it, S_n = 2 ivMax |x_n|^2 + termMax in float64 from the
    model -- the header's rounding bound, derived, not measured;
  * where the family sends every entry to the exact re-score, mode 2's scores are mode 0's bits.
Which kernel a case launches (read off gmm_score_mfma / gmm_sp_launch): uniform codebooks of R = 4 at any depth, and of 8 / 16 / 32 at dimN <= 15 or
36..39, with unit scales and the -log w table inside 160 KB of LDS -> k_gmm_mfma_sp<S4, 4, R>; DSR_GMM_SP=0, a non-unit scale, another depth at
R >= 8 or a table too large -> k_gmm_mfma_reg<S4, R>; DSR_GMM_MFMA_SCAN=1 or codebooks of mixed size -> k_gmm_mfma<4 S4>.

Template instance -> the case that launches it (S4 = 4: dimN <= 15, 5: 16..19, 9: 20..35, 10: 36..39, 12: 40..47, 17: 48..64):
  k_gmm_mfma_sp<S4, 4, 4>, every S4          test_every_depth_uniform_four, default path (S4 = 4 also test_large_models[2049])
  k_gmm_mfma_sp<4 | 10, 4, 8 | 16 | 32>      test_wide_codebooks_on_the_sp_depths, default path (dimN 13 | 39)
  k_gmm_mfma_sp<10, 4, 4, DBG != 0>          none: DSR_GMM_SPDBG builds for timing that leave out searches or stores, their output is not a score
  k_gmm_mfma_reg<S4, 4>, every S4            test_every_depth_uniform_four, DSR_GMM_SP=0 (S4 = 4 without the LDS table: test_large_models)
  k_gmm_mfma_reg<5 | 9 | 12 | 17, 8 | 16 | 32>   test_wide_codebooks_off_the_sp_depths (dimN 18 | 20 | 44 | 64)
  k_gmm_mfma_reg<4 | 10, 8 | 16 | 32>        test_wide_codebooks_on_the_sp_depths, DSR_GMM_SP=0
  k_gmm_mfma<16 | 20 | 36 | 40 | 48 | 68>    test_every_depth_uniform_four, DSR_GMM_MFMA_SCAN=1; test_every_depth_ragged_scan
  k_gmm_tie_compact<4>, k_gmm_ties           every sp case / every sp and reg case; their settle-in-place branches: test_tie_list_full"""
import numpy as np
import pytest

from tests import gmm_cases as GC

pytestmark = pytest.mark.gpu

PATHS = {"sp": {}, "reg": {"DSR_GMM_SP": "0"}, "scan": {"DSR_GMM_MFMA_SCAN": "1"}}
SIZES = [1100, 1300, 1203, 1431, 997]                                          # no multiple of 32, 128 or 512
SPECIAL_N = {(16, "unit"): 129, (47, "offset"): 515, (64, "negative"): 1}      # ends inside a tile / a wave / just past a workgroup of 512; one frame


def _n(D, family, i):
    return SPECIAL_N.get((D, family), SIZES[i % len(SIZES)])


def _run(dsr, oracle, cuda, monkeypatch, family, m, N, paths, seed, scale=None, env=None):
    """scores the frames of GC.frames with mode 0 and with mode 2 on every path of `paths`; makes the four assertions of the module docstring on
    each and compares the paths with one another -> {path: (score, argmin) tensors}"""
    import torch
    D = m["mean"].shape[1]
    x, tie, info = GC.frames(family, m, N, seed)
    kw = {} if scale is None else {"scale": scale}
    gm = dsr.Gmm(**m, **kw)
    xd = torch.from_numpy(x).to(cuda)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"], **kw)
    ref, arg = oracle.gmm_score_opt(cb, m["val"], x)
    sc0, am0 = gm.score(xd, mode=0)
    assert np.array_equal(sc0.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and np.array_equal(am0.cpu().numpy().astype(np.int32), arg)
    bound = GC.score_bound(m, x, scale)
    if GC.FAMILIES[family][2]:
        assert GC.best_over_S(m, x) < 1e-3                                     # (of the inputs: every distance is small against S, so every entry is re-scored)
    out = {}
    for p in paths:
        for k in ("DSR_GMM_SP", "DSR_GMM_MFMA_SCAN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in dict(PATHS[p], **(env or {})).items():
            monkeypatch.setenv(k, v)
        sc2, am2 = gm.score(xd, mode=2)
        a2 = am2.cpu().numpy().astype(np.int32); s2 = sc2.cpu().numpy()
        wrong = np.argwhere(a2 != arg)
        assert len(wrong) == 0, "%s: %d of %d argmins differ from the reference's (%d of them on near-tie frames), first (frame, codebook) %s" % (
            p, len(wrong), a2.size, int(tie[wrong[:, 0]].sum()), wrong[0])
        same = s2.view(np.uint32) == ref.view(np.uint32)
        err = np.abs(s2.astype(np.float64) - ref.astype(np.float64))
        print("%s %s D=%d N=%d: %.1f %% of the scores are mode 0's bits, the others off by at most %.2f of the bound" % (
            family, p, D, N, 100.0 * same.mean(), float((err / bound)[~same].max()) if (~same).any() else 0.0))
        assert (same | (err <= bound)).all(), "%s: score off by %.3g of the bound" % (p, float((err / bound)[~same].max()))
        if GC.FAMILIES[family][2]:
            assert torch.equal(sc2, sc0), p
        out[p] = (sc2, am2)
    for k in ("DSR_GMM_SP", "DSR_GMM_MFMA_SCAN"):
        monkeypatch.delenv(k, raising=False)
    ps = list(out)
    for i in range(1, len(ps)):                                                # (an entry on the edge of the radius may be re-scored by one path and not by another)
        assert torch.equal(out[ps[0]][1], out[ps[i]][1])
        assert (np.abs(out[ps[0]][0].cpu().numpy().astype(np.float64) - out[ps[i]][0].cpu().numpy().astype(np.float64)) <= 2.0 * bound).all(), (ps[0], ps[i])
    return out


# ---- 1. every contraction depth (S2 = 16, 20, 36, 40, 48, 68: dimN on both sides of every boundary), every kernel
@pytest.mark.parametrize("family", GC.FAMILY_NAMES)
@pytest.mark.parametrize("D", GC.DEPTH_D)
def test_every_depth_uniform_four(dsr, oracle, cuda, monkeypatch, D, family):
    """37 codebooks of four: k_gmm_mfma_sp<S4, 4, 4>, k_gmm_mfma_reg<S4, 4> and k_gmm_mfma<4 S4> -- the three agree with the reference and with one another"""
    m = GC.model(family, 37, 4, D, seed=3)
    _run(dsr, oracle, cuda, monkeypatch, family, m, _n(D, family, D + GC.FAMILY_NAMES.index(family)), ["sp", "reg", "scan"], seed=10 + D)


@pytest.mark.parametrize("D", GC.DEPTH_D)
def test_every_depth_ragged_scan(dsr, oracle, cuda, monkeypatch, D):
    """codebooks of mixed size (1 to 33 Gaussians; a codebook that crosses a 32-row chunk, chunks that close several) go to the scan kernel k_gmm_mfma<4 S4>"""
    refN = [3, 7, 33, 1, 4, 2, 33, 16, 5, 3, 7, 9, 33, 2]
    family = GC.FAMILY_NAMES[GC.DEPTH_D.index(D) % len(GC.FAMILY_NAMES)]
    m = GC.model(family, len(refN), 0, D, seed=4, refN=refN)
    _run(dsr, oracle, cuda, monkeypatch, family, m, SIZES[D % len(SIZES)], ["sp"], seed=20 + D)      # (no path variable set: the dispatch itself picks the scan kernel)


# ---- 2. codebooks of 8, 16, 32
@pytest.mark.parametrize("family", GC.FAMILY_NAMES)
@pytest.mark.parametrize("D", GC.WIDE_D_REG)
@pytest.mark.parametrize("R,K", GC.WIDE_R)
def test_wide_codebooks_off_the_sp_depths(dsr, oracle, cuda, monkeypatch, R, K, D, family):
    """k_gmm_sp.hip has R >= 8 only at S4 = 4 and 10: these depths reach k_gmm_mfma_reg<5 | 9 | 12 | 17, R> with nothing set"""
    m = GC.model(family, K, R, D, seed=3)
    _run(dsr, oracle, cuda, monkeypatch, family, m, SIZES[(R + D) % len(SIZES)], ["sp"], seed=30 + D + R)


@pytest.mark.parametrize("family", GC.FAMILY_NAMES)
@pytest.mark.parametrize("D", GC.WIDE_D_SP)
@pytest.mark.parametrize("R,K", GC.WIDE_R)
def test_wide_codebooks_on_the_sp_depths(dsr, oracle, cuda, monkeypatch, R, K, D, family):
    """k_gmm_mfma_sp<4 | 10, 4, R> (at R = 32 four mantissa bits carry the index: on positive, negative and mixed distances) and k_gmm_mfma_reg<4 | 10, R>"""
    m = GC.model(family, K, R, D, seed=3)
    _run(dsr, oracle, cuda, monkeypatch, family, m, SIZES[(R + D + 1) % len(SIZES)], ["sp", "reg"], seed=40 + D + R)


# ---- 3. a tie list that fills up many times over: what does not fit is settled in place
@pytest.mark.parametrize("family", ["unit", "negative"])
@pytest.mark.parametrize("tiecap", [2, 5])
@pytest.mark.parametrize("D", [18, 44, 64])
def test_tie_list_full(dsr, oracle, cuda, monkeypatch, D, tiecap, family):
    m = GC.model(family, 37, 4, D, seed=5)
    _run(dsr, oracle, cuda, monkeypatch, family, m, 1300, ["sp", "reg"], seed=50 + D, env={"DSR_GMM_TIECAP": str(tiecap)})


# ---- 4. codebook scales other than one (some exactly one): the model leaves the sp shape for k_gmm_mfma_reg; the scan kernel and k_gmm_ties scale too
@pytest.mark.parametrize("family", ["unit", "far", "negative"])
@pytest.mark.parametrize("K,R,D", [(37, 4, 39), (9, 16, 18)])
def test_codebook_scale(dsr, oracle, cuda, monkeypatch, K, R, D, family):
    m = GC.model(family, K, R, D, seed=6)
    scale = np.random.default_rng(K).uniform(0.5, 2.0, K).astype(np.float32)
    scale[::4] = 1.0
    _run(dsr, oracle, cuda, monkeypatch, family, m, 1100, ["sp", "scan"], seed=60 + D, scale=scale)


# ---- 5. large models
def _sp_lds(G):
    """gmm_sp_lds of k_gmm_sp.hip: the -log w table, four waves' score strips [128 frames][36] and argmin rows [128][36 bytes], 16 spare"""
    return 4 * ((G + 3) & ~3) + 4 * (4 * 32 * 4 * 36) + 4 * 32 * 4 * 36 + 16


@pytest.mark.parametrize("K,N,paths", [(2049, 260, ["sp", "reg"]), (4600, 200, ["sp"])])
def test_large_models(dsr, oracle, cuda, monkeypatch, K, N, paths):
    """G = 8196 Gaussians: 124 960 bytes of LDS for the sp shape, inside its 160 KB - 64, so the default is k_gmm_mfma_sp<4, 4, 4>; with DSR_GMM_SP=0
    k_gmm_mfma_reg<4, 4> runs, and G > 8192 keeps its -log w table in memory (valInLds = 0).  G = 18 400: 165 776 bytes, over the limit: the
    default falls back to k_gmm_mfma_reg<4, 4>, again without the table in LDS.
    Near ties come from 'far' (everything is re-scored: k_gmm_ties at this size); at dimN = 5 the families whose entries are NOT all re-scored
    miss the 30 % flip share test_gmm_cases_cpu.py asks of near-tie inputs (0.27-0.30 measured: with 11 terms the rounding of the frame moves
    the gap as much as the expanded form does), so the kernels' own score path -- the -log w look-up this case is about -- runs on plain frames."""
    import torch
    G = 4 * K
    assert (_sp_lds(G) <= 160 * 1024 - 64) == (K == 2049) and G > 8192
    m = GC.model("far", K, 4, 5, seed=7)
    _run(dsr, oracle, cuda, monkeypatch, "far", m, N, paths, seed=70)
    m = GC.model("unit", K, 4, 5, seed=8)
    x = GC.plain_frames("unit", N, 5, seed=71)
    gm = dsr.Gmm(**m); xd = torch.from_numpy(x).to(cuda)
    ref, arg = oracle.gmm_score_opt(oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"]), m["val"], x)
    sc0, am0 = gm.score(xd, mode=0)
    assert np.array_equal(sc0.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and np.array_equal(am0.cpu().numpy().astype(np.int32), arg)
    bound = GC.score_bound(m, x)
    for p in paths:
        for k, v in PATHS[p].items():
            monkeypatch.setenv(k, v)
        sc2, am2 = gm.score(xd, mode=2)
        s2 = sc2.cpu().numpy()
        same = s2.view(np.uint32) == ref.view(np.uint32)
        assert np.array_equal(am2.cpu().numpy().astype(np.int32), arg)
        assert (same | (np.abs(s2.astype(np.float64) - ref) <= bound)).all()


# ---- 6. scores alone
@pytest.mark.parametrize("D", [18, 39])
def test_scores_without_argmin(dsr, cuda, monkeypatch, D):
    """want_argmin=False: k_gmm_mfma_sp makes a zero-length buffer of the score pointer for its argmin stores, the others test the pointer -- the
    scores are those of the run that also writes argmins, bit for bit, on the three kernels"""
    import torch
    m = GC.model("unit", 37, 4, D, seed=9)
    x, _, _ = GC.frames("unit", m, 1203, seed=80 + D)
    gm = dsr.Gmm(**m); xd = torch.from_numpy(x).to(cuda)
    for p, env in PATHS.items():
        for k in ("DSR_GMM_SP", "DSR_GMM_MFMA_SCAN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sc, am = gm.score(xd, mode=2)
        sc_n, am_n = gm.score(xd, mode=2, want_argmin=False)
        assert am is not None and am_n is None and torch.equal(sc, sc_n), p


# ---- 7. the dimension limit
def test_dimension_limit(dsr, oracle, cuda):
    """dimN = 65: mode 2 refuses with the binding's dimension error and leaves the model usable; mode 0 scores it bit for bit"""
    import torch
    m = GC.model("unit", 5, 4, 65, seed=2)
    x, _, _ = GC.frames("unit", m, 129, seed=90)
    gm = dsr.Gmm(**m); xd = torch.from_numpy(x).to(cuda)
    with pytest.raises(dsr.DsrError) as e:
        gm.score(xd, mode=2)
    assert e.value.status == dsr.E_DIMENSION
    ref, arg = oracle.gmm_score_opt(oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"]), m["val"], x)
    sc0, am0 = gm.score(xd, mode=0)
    assert np.array_equal(sc0.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and np.array_equal(am0.cpu().numpy().astype(np.int32), arg)
    with pytest.raises(dsr.DsrError):
        gm.score(xd, mode=2)                                                    # (still refused, still no damage)
    assert torch.equal(gm.score(xd, mode=0)[0], sc0)
