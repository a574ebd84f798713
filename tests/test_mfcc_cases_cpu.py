"""The cases of tests/mfcc_cases.py are what tests/test_gpu_mfcc_kernels.py takes them for -- conditions on the INPUTS and on the dispatch's size
formulas, checked without a GPU (no kernel is involved):
  * the oracle accepts the configuration: the mel bank exists, every filter has a tap and reads inside the power spectrum;
  * the frame counts are the ones the case names (0 samples, no frame, one frame, 0 < T < delta, Tmax at the tile edge it is there for);
  * the oracle's output on the chosen samples is finite at every stage, and the silence is where the floors need it;
  * each size formula of dsr_mfcc_run's dispatch, stated below and computed from the configuration, falls on the side of its gate the case names,
    and the library's own query (dsr_mfcc_cfg_paths, the helper dsr_mfcc_run launches from) computes the same bytes and picks the named kernel.

The formulas (csrc/k_mfcc.hip, bytes of dynamic LDS; S = 2 delta + 1, Np = ncep rounded up to a multiple of 4, nG = 256 // outDim):
  ldsW = 16 fftLen (1 + 4) + 8 blockLen + 4 (melCoefN + ncep filterN + 3 filterN)     k_mfcc_frames_w when <= 52 KB and fftLen is 256 or 512
  ldsC = 4 Tmax ncep                                                                  k_cmn_lds when <= 64 KB, ncep <= 64 and cmnMode is 1
  ldsB = 4 (outDim (S Np + 4) + (8 nG + 2 delta) Np)                                  k_splice_lda_b when <= 52 KB and nG >= 1
  lds2 = 4 (outDim S Np + (64 + 2 delta) Np)                                          k_splice_lda when <= 160 KB, DSR_E_DIMENSION past it
melCoefN is the number of mel coefficients (the taps of all filters)."""
import numpy as np
import pytest

from tests import mfcc_cases as MC

KB = 1024
GATE = {"ldsW": 52 * KB, "ldsW_next": 52 * KB, "ldsC": 64 * KB, "ldsB": 52 * KB, "lds2": 160 * KB}


def _melbank(oracle, c):
    up = c["up"] if c["up"] > 0 else c["rate"] / 2.0
    assert c["low"] >= 0.0 and 2.0 * up <= c["rate"] and c["low"] <= up                   # (orc_melbank_create returns NULL otherwise)
    return oracle.melbank(c["powN"], c["rate"], c["low"], c["up"], c["filterN"], c["melVersion"])


def formulas(c, melCoefN, Tmax):
    S = 2 * c["delta"] + 1; Np = (c["ncep"] + 3) // 4 * 4
    f = {"ldsW": 16 * c["fftLen"] * (1 + 4) + 8 * c["blockLen"] + 4 * (melCoefN + c["ncep"] * c["filterN"] + 3 * c["filterN"]),
         "ldsC": 4 * Tmax * c["ncep"], "ldsB": 0, "lds2": 16}
    f["ldsW_next"] = f["ldsW"] + 4 * c["filterN"]                                         # with one cepstral coefficient more
    if c["outDim"] > 0:
        nG = 256 // c["outDim"]
        f["ldsB"] = 4 * (c["outDim"] * (S * Np + 4) + (8 * nG + 2 * c["delta"]) * Np)
        f["lds2"] = 4 * (c["outDim"] * S * Np + (64 + 2 * c["delta"]) * Np)
    return f


def paths_from(c, f, env):
    """the dispatch as DESIGN 4.4 and the kernel headers describe it, from the formulas"""
    fr = MC.FRAMES_W if ("DSR_MFCC_PLAIN" not in env and c["fftLen"] in (256, 512) and f["ldsW"] <= GATE["ldsW"]) else MC.FRAMES_PLAIN
    if c["cmnMode"] == 0:
        cm = MC.CMN_NONE
    else:
        cm = MC.CMN_LDS if ("DSR_CMN_PLAIN" not in env and c["cmnMode"] == 1 and c["ncep"] <= 64 and f["ldsC"] <= GATE["ldsC"]) else MC.CMN_PLAIN
    if c["outDim"] <= 0:
        ld = MC.LDA_SPLICE
    elif "DSR_LDA_PLAIN" not in env and c["outDim"] <= 256 and f["ldsB"] <= GATE["ldsB"]:
        ld = MC.LDA_B
    else:
        ld = MC.LDA_PLAIN if f["lds2"] <= GATE["lds2"] else MC.LDA_TOO_LARGE
    return fr, cm, ld


@pytest.mark.parametrize("case", MC.ALL_CASES, ids=lambda c: c["name"])
def test_case_is_what_it_names(dsr, oracle, headset, monkeypatch, case):
    c = case["cfg"]
    # ---- the configuration
    assert c["powN"] in (c["fftLen"], c["fftLen"] // 2 + 1) and 2 <= c["blockLen"] <= c["fftLen"] and c["vtlnVersion"] in (1, 2)
    rows = _melbank(oracle, c)
    for off, coef in rows:
        assert len(coef) >= 1 and np.count_nonzero(coef) >= 1, "a mel filter without a tap"
        assert off >= 0 and off + len(coef) <= c["powN"], "a mel filter reads past the power spectrum"
    melCoefN = sum(len(coef) for _, coef in rows)
    # ---- the frame counts
    y, lens = MC.batch(case, headset)
    assert len(headset) == 134824 and np.abs(headset).max() <= 32768 and y.shape == (len(lens), max(max(lens), 1))
    T = [oracle.lib().orc_sample_num_blocks(n, c["blockLen"], c["shiftLen"], c["padZeros"]) for n in lens]
    assert T == [MC.raw_frames(n, c) for n in lens]
    Tmax = MC.tmax_of(case)
    for spec, n, t in zip(case["frames"], lens, T):
        if spec == "empty":
            assert n == 0 and t == 0
        elif spec == "short":
            assert 0 < n < c["blockLen"] and (t == 0 if not c["padZeros"] else t >= 1)
        else:
            assert t == spec and MC.raw_frames(n - 1, c) == spec - 1                      # the shortest utterance of that many frames
    assert case["frames"][0] == "empty" and case["frames"][1] == "short" and 1 in T and Tmax == max(T) == case["frames"][-1]
    if c["delta"] > 1 and Tmax >= c["delta"]:
        assert any(0 < t < c["delta"] for t in T), "no utterance with 0 < T < delta"
    # ---- the oracle's output
    cfg = oracle.mfcc_cfg(lda=MC.lda_of(case), **MC.oracle_kw(case))
    for u, n in enumerate(lens):
        for stage in (4, 3, 1, 2, 0):
            ref = oracle.mfcc_chain(y[u, :n], cfg, stage=stage)
            assert ref.shape[0] == (MC.chain_frames(n, c) if stage == 0 else T[u]) and np.isfinite(ref).all(), (u, stage)
    # ---- the size formulas and the kernels they select
    f = formulas(c, melCoefN, Tmax)
    for name, inside in case["gates"].items():
        assert (f[name] <= GATE[name]) == inside, (name, f[name], GATE[name])
    for k in ("DSR_MFCC_PLAIN", "DSR_CMN_PLAIN", "DSR_LDA_PLAIN", "DSR_LDA_FB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    want = paths_from(c, f, case["env"])
    for e, w in zip(case["expect"], want):
        assert e is None or e == w, (case["expect"], want)
    assert any(e is not None for e in case["expect"])
    got, lds = dsr.mfcc_cfg_paths(Tmax, **c)
    assert got == want and lds == {k: f[k] for k in ("ldsW", "ldsC", "ldsB", "lds2")}, (got, want, lds, f)


def test_path_codes_are_the_headers(dsr):
    assert (MC.FRAMES_PLAIN, MC.FRAMES_W) == (dsr.MFCC_FRAMES_PLAIN, dsr.MFCC_FRAMES_W)
    assert (MC.CMN_NONE, MC.CMN_PLAIN, MC.CMN_LDS) == (dsr.MFCC_CMN_NONE, dsr.MFCC_CMN_PLAIN, dsr.MFCC_CMN_LDS)
    assert (MC.LDA_TOO_LARGE, MC.LDA_SPLICE, MC.LDA_PLAIN, MC.LDA_B) == (dsr.MFCC_LDA_TOO_LARGE, dsr.MFCC_LDA_SPLICE, dsr.MFCC_LDA_PLAIN, dsr.MFCC_LDA_B)
    import os
    import re
    from tests.conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "dsr.h")).read()
    for name, val in (("FRAMES_PLAIN", 0), ("FRAMES_W", 1), ("CMN_NONE", 0), ("CMN_PLAIN", 1), ("CMN_LDS", 2), ("LDA_TOO_LARGE", -1),
                      ("LDA_SPLICE", 0), ("LDA_PLAIN", 1), ("LDA_B", 2)):
        assert re.search(r"\bDSR_MFCC_%s\s*=\s*%d\b" % (name, val), hdr), name


def test_switches_are_read_on_every_call(dsr, monkeypatch):
    """one process can run both kernels of each pair: the query (and dsr_mfcc_run, which launches from the same helper) follows the environment"""
    kw = dict(MC.DEFAULTS, outDim=39)
    for k in ("DSR_MFCC_PLAIN", "DSR_CMN_PLAIN", "DSR_LDA_PLAIN"):
        monkeypatch.delenv(k, raising=False)
    assert dsr.mfcc_cfg_paths(100, **kw)[0] == (MC.FRAMES_W, MC.CMN_LDS, MC.LDA_B)
    monkeypatch.setenv("DSR_MFCC_PLAIN", "1")
    assert dsr.mfcc_cfg_paths(100, **kw)[0] == (MC.FRAMES_PLAIN, MC.CMN_LDS, MC.LDA_B)
    monkeypatch.setenv("DSR_CMN_PLAIN", "1")
    assert dsr.mfcc_cfg_paths(100, **kw)[0] == (MC.FRAMES_PLAIN, MC.CMN_PLAIN, MC.LDA_B)
    monkeypatch.setenv("DSR_LDA_PLAIN", "1")
    assert dsr.mfcc_cfg_paths(100, **kw)[0] == (MC.FRAMES_PLAIN, MC.CMN_PLAIN, MC.LDA_PLAIN)
    monkeypatch.delenv("DSR_MFCC_PLAIN"); monkeypatch.delenv("DSR_CMN_PLAIN"); monkeypatch.delenv("DSR_LDA_PLAIN")
    assert dsr.mfcc_cfg_paths(100, **kw)[0] == (MC.FRAMES_W, MC.CMN_LDS, MC.LDA_B)


def test_tile_edges_are_the_named_ones():
    """Tmax of the _w cases covers 1, 31, 32, 33, 65 at both FFT lengths; the register-blocked transform's cases sit one short of, on and one
    past 4 blocks of FB = 8 nG frames; block and shift lengths cover the edges the pre-emphasis has"""
    for fft in (256, 512):
        cs = [c for c in MC.W_CASES if c["cfg"]["fftLen"] == fft]
        assert {MC.tmax_of(c) for c in cs} == {1, 31, 32, 33, 65}
        bl = {c["cfg"]["blockLen"] for c in cs}
        assert fft in bl and any(b % 64 for b in bl) and (fft == 256 or {200, 320, 400} <= bl)
        assert any(c["cfg"]["shiftLen"] == c["cfg"]["blockLen"] for c in cs) and any(c["cfg"]["shiftLen"] == c["cfg"]["blockLen"] + 37 for c in cs)
        assert any(c["cfg"]["shiftLen"] in (80, 160) for c in cs)
        assert any(c["cfg"]["mu"] < 0 for c in cs) and any(c["cfg"]["padZeros"] for c in cs) and any(c["cfg"]["powN"] == fft for c in cs)
        assert {c["cfg"]["vtlnVersion"] for c in cs if c["cfg"]["vtlnRatio"] != 1.0 and c["cfg"]["powN"] == fft // 2 + 1} == {1, 2}
        assert any(c["cfg"]["sphinxFlooring"] and c["silence"] for c in cs)
    for c in MC.PLAIN_FFT:
        assert c["cfg"]["blockLen"] < c["cfg"]["fftLen"] and c["cfg"]["blockLen"] % 64 and 40 <= MC.tmax_of(c) <= 48
    assert {c["cfg"]["fftLen"] for c in MC.PLAIN_FFT} == {32, 64, 128, 1024, 2048, 4096}
    seen = {}
    for c in MC.LDA_B_CASES:
        o = c["cfg"]["outDim"]; FB = 8 * (256 // o)
        assert MC.tmax_of(c) in (4 * FB - 1, 4 * FB, 4 * FB + 1)
        seen.setdefault((o, c["cfg"]["ncep"], c["cfg"]["delta"]), set()).add(MC.tmax_of(c) - 4 * FB)
        T = [MC.raw_frames(n, c["cfg"]) for n in MC.lens_of(c)]
        assert any(t % 8 and 8 < t < MC.tmax_of(c) for t in T), "no utterance ends inside an 8-frame run"
        if c["cfg"]["delta"] > 0:
            assert c["cfg"]["delta"] in T
    assert {k[0] for k in seen} == {1, 39, 64, 100, 128, 256} and {k[1] for k in seen} >= {12, 13, 16} and {k[2] for k in seen} == {0, 1, 2, 7}
    assert sum(v == {-1, 0, 1} for v in seen.values()) >= 6


def test_silence_reaches_the_floors(oracle, headset):
    """the sphinx cases have mel energies below the 1e-5 floor (log-mel of exactly -5) next to live frames; the normalisation cases have a constant
    cepstral dimension (DCT row filterN) in a live utterance and a silent utterance, both with variance below the 1e-4 floor"""
    for case in MC.W_CASES:
        if not case["cfg"]["sphinxFlooring"]:
            continue
        y, lens = MC.batch(case, headset)
        cfg = oracle.mfcc_cfg(**MC.oracle_kw(case))
        lm = oracle.mfcc_chain(y[4, :lens[4]], cfg, stage=3)
        floored = (lm == np.float32(-5.0)).all(1)
        assert 5 <= floored.sum() < len(lm) and (lm[~floored] > -5.0).any()
    for case in MC.CMN_CASES:
        c = case["cfg"]
        if c["ncep"] <= c["filterN"]:
            continue
        y, lens = MC.batch(case, headset)
        cfg = oracle.mfcc_cfg(**MC.oracle_kw(case))
        cep = oracle.mfcc_chain(y[-1, :lens[-1]], cfg, stage=1)
        _, _, var = oracle.cmn_batch(cep, 1.0)
        assert var[c["filterN"]] < 1e-4 and (var[:c["filterN"]] > 1e-4).all()
        sil = oracle.mfcc_chain(y[4, :lens[4]], cfg, stage=1)
        assert len(sil) >= 2 and (oracle.cmn_batch(sil, 1.0)[2] < 1e-4).all()
