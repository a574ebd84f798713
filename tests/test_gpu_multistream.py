"""Multi-stream decoding on the device (csrc/ms_kernels.hip, csrc/multistream.cpp through dsr._ms and dsr.asr.gaussian): the combination of two
score matrices on every path of its dispatch, bit for bit against tests/ms_np.py; no fused multiply-add; a two-model decode through the operator
face and through the batch face against the oracle's decoder fed with the combined scores; the errors.  Every comparison of scores is
np.array_equal: the arithmetic is fully specified, there is no tolerance."""
import ctypes as C
import gc
import importlib
import os
import sys

import numpy as np
import pytest

import dsr._ms as M                                        # the product: without it nothing here can pass
from tests import ms_cases, ms_np, synth

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
LDS_SHAPES = [(1, 1), (5, 3), (24, 6), (260, 7), (24, 24)]


def _gmm(dsr, K, D=2):
    """a model of K one-Gaussian states named ds0 .. ds<K-1>: the combiner takes only names and counts from it"""
    return dsr.Gmm(refN=np.ones(K, np.int32), mean=np.zeros((K, D), np.float32), ivar=np.ones((K, D), np.float32), det=np.zeros(K, np.float32),
                   val=np.zeros(K, np.float32))


def _combiner(dsr, gA, gV, table, wA=0.95, wV=0.05):
    """a MultiStream whose resolved table is `table`: audio state ds<k> is mapped to video state ds<table[k]>"""
    ms = M.MultiStream(gA, gV, M.DistribMap({"ds%d" % k: "ds%d" % t for k, t in enumerate(table)}), wA, wV)
    assert np.array_equal(ms.table, table)
    return ms


def _guarded(torch, cuda, host, off):
    """host [N][K] on the device inside a larger allocation: a front guard of a multiple of four floats, `off` floats of misalignment, the data, a
    guard row behind -- all guards hold the sentinel.  -> (whole buffer, the [N][K] view)"""
    N, K = host.shape
    front = 4 * ((K + 3) // 4) + off
    buf = torch.full((front + N * K + K + 4,), float(SENTINEL), dtype=torch.float32, device=cuda)
    view = buf[front:front + N * K].view(N, K)
    view.copy_(torch.from_numpy(host))
    assert buf.data_ptr() % 16 == 0 and (view.data_ptr() % 16 == 0) == (off == 0) and view.is_contiguous()
    return buf, view


def _guards_intact(buf, view):
    h = buf.cpu().numpy(); n = view.numel(); front = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((h[:front] == SENTINEL).all() and (h[front + n:] == SENTINEL).all())


def _run_shape(dsr, cuda, KA, KV, Ns, expect_paths):
    import torch
    gA, gV = _gmm(dsr, KA), _gmm(dsr, KV)
    rng = np.random.default_rng(1000 * KA + KV)
    seen = set()
    for tname, table in ms_cases.tables(KA, KV, seed=KA + KV).items():
        ms = _combiner(dsr, gA, gV, table)
        if tname == "many_to_one":
            assert table.max() == KV - 1 and (KV < 3 or len(set(table.tolist())) < KV)
        for N in Ns:
            sA, sV = ms_cases.scores(rng, (N, KA)), ms_cases.scores(rng, (N, KV))
            for wi, (wA, wV) in enumerate(ms_cases.WEIGHTS):
                ms.setWeights(wA, wV)
                ref = ms_np.combine(sA, sV, table, wA, wV)
                # (offset of sA / out, offset of sV) in floats from a 16-byte aligned base; every weight pair runs aligned, they share the rest
                for offA, offV in ([(0, 0), (1, 0), (0, 1), (1, 1)] if wi in (0, 3) else [(0, 0)]):
                    path = M.combine_path(KA, KV, offA == 0)[0]; seen.add(path)
                    bV, dV = _guarded(torch, cuda, sV, offV)
                    # out of place: the inputs are unchanged, nothing outside out's N rows is written
                    bA, dA = _guarded(torch, cuda, sA, offA); bO, dO = _guarded(torch, cuda, np.full((N, KA), SENTINEL, np.float32), offA)
                    got = ms.combine(dA, dV, out=dO)
                    assert got is dO and np.array_equal(dO.cpu().numpy(), ref), (KA, KV, tname, N, wA, wV, offA, offV, "out of place")
                    assert np.array_equal(dA.cpu().numpy(), sA) and np.array_equal(dV.cpu().numpy(), sV)
                    assert _guards_intact(bO, dO) and _guards_intact(bA, dA) and _guards_intact(bV, dV)
                    # in place
                    ms.combine(dA, dV, out=dA)
                    assert np.array_equal(dA.cpu().numpy(), ref), (KA, KV, tname, N, wA, wV, offA, offV, "in place")
                    assert np.array_equal(dV.cpu().numpy(), sV) and _guards_intact(bA, dA) and _guards_intact(bV, dV)
    assert seen == expect_paths, (seen, expect_paths)


@pytest.mark.parametrize("KA,KV", LDS_SHAPES)
def test_combine_lds_paths(dsr, cuda, KA, KV):
    path, R, lds = M.combine_path(KA, KV, True)
    assert path == (M.VECTOR_LDS if KA % 4 == 0 else M.SCALAR_LDS) and lds > 0
    _run_shape(dsr, cuda, KA, KV, [1, R, R + 1, 2 * R + 3], {M.VECTOR_LDS, M.SCALAR_LDS} if KA % 4 == 0 else {M.SCALAR_LDS})


def test_combine_gather_path(dsr, cuda):
    KV = M.LDS_BUDGET // 4 + 1                                                        # one video row alone exceeds the LDS budget
    assert M.combine_path(8, KV, True)[0] == M.GATHER and M.combine_path(8, KV - 1, True)[0] == M.VECTOR_LDS
    _run_shape(dsr, cuda, 8, KV, [3], {M.GATHER})


def test_combine_largest_lds_tile(dsr, cuda):
    """the widest video row the LDS paths take (one row fills the budget), at a row count that is no multiple of the tile, sV off alignment"""
    import torch
    KV, KA = M.LDS_BUDGET // 4, 12
    assert M.combine_path(KA, KV, True)[:2] == (M.VECTOR_LDS, 1)
    rng = np.random.default_rng(5)
    table = rng.integers(0, KV, KA).astype(np.int32); table[3] = KV - 1; table[7] = 0
    ms = _combiner(dsr, _gmm(dsr, KA), _gmm(dsr, KV), table, 0.3, 1.7)
    sA, sV = ms_cases.scores(rng, (3, KA)), ms_cases.scores(rng, (3, KV))
    for offV in (0, 1, 2, 3):
        bV, dV = _guarded(torch, cuda, sV, offV)
        got = ms.combine(torch.from_numpy(sA).to(cuda), dV)
        assert np.array_equal(got.cpu().numpy(), ms_np.combine(sA, sV, table, 0.3, 1.7)), offV
        assert _guards_intact(bV, dV)


def test_combine_past_2_31_elements(dsr, cuda):
    """element indices past 2^31 and byte offsets past 2^33: in place at [2^21 + 3][1024] x [.][64], rows at the start, around the 2^31st element
    and at the end against the restatement"""
    import torch
    KA, KV, N = 1024, 64, (1 << 21) + 3
    table = ((np.arange(KA) * 7 + 3) % KV).astype(np.int32)
    ms = _combiner(dsr, _gmm(dsr, KA), _gmm(dsr, KV), table, 0.3, 1.7)
    g = torch.Generator(device=cuda); g.manual_seed(9)
    sA = torch.randn((N, KA), dtype=torch.float32, device=cuda, generator=g).mul_(100.0)
    sV = torch.randn((N, KV), dtype=torch.float32, device=cuda, generator=g).mul_(100.0)
    R = M.combine_path(KA, KV, True)[1]
    spans = [(0, 2 * R + 1), ((1 << 21) - R - 1, (1 << 21) + R + 1), (N - R - 2, N)]
    before = [(sA[a:b].cpu().numpy(), sV[a:b].cpu().numpy()) for a, b in spans]
    ms.combine(sA, sV, out=sA)
    for (a, b), (hA, hV) in zip(spans, before):
        assert np.array_equal(sA[a:b].cpu().numpy(), ms_np.combine(hA, hV, table, 0.3, 1.7)), (a, b)


@pytest.mark.parametrize("wA,wV", ms_cases.FMA_WEIGHTS)
def test_no_contraction(dsr, cuda, wA, wV):
    """the near-cancellation arrays of tests/ms_cases.py give exactly the unfused bits: neither product is contracted into the sum (a build of
    the kernel file without -ffp-contract=off fails here, see test_ms_np_cpu.test_cancellation_set_tells_a_fused_multiply_add for the counts)"""
    import torch
    c = ms_cases.fma_case(wA, wV)
    K = ms_cases.FMA_COLS
    ms = _combiner(dsr, _gmm(dsr, K), _gmm(dsr, K), np.arange(K, dtype=np.int32), wA, wV)
    a, v = torch.from_numpy(c["a"]).to(cuda), torch.from_numpy(c["v"]).to(cuda)
    got = ms.combine(a, v).cpu().numpy()
    differs = (c["fmaA"] != c["unfused"]) | (c["fmaV"] != c["unfused"])
    assert differs.sum() >= 64
    assert np.array_equal(got[differs], c["unfused"][differs]) and np.array_equal(got, c["unfused"])
    # the scalar path (sA off alignment) has the same arithmetic
    buf, av = _guarded(torch, cuda, c["a"], 1)
    assert np.array_equal(ms.combine(av, v).cpu().numpy(), c["unfused"])


def test_set_weights_takes_effect_on_the_next_call(dsr, cuda):
    import torch
    KA, KV = 24, 6
    table = (np.arange(KA) % KV).astype(np.int32)
    ms = _combiner(dsr, _gmm(dsr, KA), _gmm(dsr, KV), table)
    assert ms.weights() == (0.95, 0.05)                                              # the reference's defaults (distribBasic.h:137)
    rng = np.random.default_rng(8)
    sA, sV = ms_cases.scores(rng, (19, KA)), ms_cases.scores(rng, (19, KV))
    dA, dV = torch.from_numpy(sA).to(cuda), torch.from_numpy(sV).to(cuda)
    r0 = ms.combine(dA, dV).cpu().numpy()
    assert np.array_equal(r0, ms_np.combine(sA, sV, table, 0.95, 0.05))
    ms.setWeights(0.3, 1.7)
    r1 = ms.combine(dA, dV).cpu().numpy()
    assert np.array_equal(r1, ms_np.combine(sA, sV, table, 0.3, 1.7)) and not np.array_equal(r0, r1)
    ms.setWeights(1.0, 0.0)
    assert ms.weights() == (1.0, 0.0) and np.array_equal(ms.combine(dA, dV).cpu().numpy().view(np.int32), sA.view(np.int32))   # sA bit for bit


# ------------------------------------------------------------------------------------------------------------------------------------------
# end to end through the operator face: the shape of test_gpu_streams.test_decode_like_decodeTest with two chains and two models

KA_E, KV_E = 24, 6


class _E2E:
    pass


@pytest.fixture(scope="module")
def e2e(dsr, oracle, cuda, headset, tmp_path_factory):
    from dsr.btk.feature import (SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr, MelFeaturePtr, LogFeaturePtr,
                                 CepstralFeaturePtr, FeatureSetPtr)
    from dsr.asr.dictionary import LexiconPtr
    from dsr.asr.gaussian import CodebookSetBasicPtr, DistribSetBasicPtr, DistribMapPtr
    from dsr.asr.decoder import WFSTFlyWeightPtr
    tmp = tmp_path_factory.mktemp("ms")
    e = _E2E(); e.tmp = tmp

    def model(tag, K, R, D, seed, feature, scale, shift):
        m = synth.gmm_model(K, R, D, seed=seed); m["mean"] = m["mean"] * scale + shift
        cbf, dsf = str(tmp / (tag + "cb.bin")), str(tmp / (tag + "ds.bin"))
        dsr.Gmm(**m).save(cbf, dsf)
        open(tmp / (tag + "cb.desc"), "w").write("".join("%-25s%-20s%-10d%-3d%-10s\n" % ("cb%d" % k, feature, R, D, "DIAGONAL") for k in range(K)))
        open(tmp / (tag + "ds.desc"), "w").write("".join("%-25s%-25s\n" % ("ds%d" % k, "cb%d" % k) for k in range(K)))
        return m, cbf, dsf

    e.mA, cbA, dsA = model("a", KA_E, 8, 13, 5, "Cepstral", 20.0, 0.0)
    e.mV, cbV, dsV = model("v", KV_E, 4, 8, 6, "LogMel", 3.0, 12.0)
    e.inlex = ["eps"] + ["ds%d" % k for k in range(KA_E)]; e.inlex[4] = "SIL-m"
    e.outlex = ["eps", "</s>"] + ["w%d" % i for i in range(50)]
    open(tmp / "in.lex", "w").write("\n".join(e.inlex) + "\n"); open(tmp / "out.lex", "w").write("\n".join(e.outlex) + "\n")
    arcs, fin = synth.random_wfst(400, KA_E, seed=4, nWords=51, out_frac=0.2)
    e.go = oracle.Wfst()
    with open(tmp / "g.fsm", "w") as f:
        for a in arcs:
            f.write("%d %d %d %d %.9g\n" % a); e.go.add_arc(*a)
        for s, c in fin:
            f.write("%d %.9g\n" % (s, c)); e.go.add_final(s, c)

    def power(samp):
        return SpectralPowerFeaturePtr(FFTFeaturePtr(HammingFeaturePtr(samp), fftLen=512), powN=257)
    e.sampA = SampleFeaturePtr(blockLen=320, shiftLen=160); e.sampV = SampleFeaturePtr(blockLen=320, shiftLen=160)
    e.featA = CepstralFeaturePtr(LogFeaturePtr(MelFeaturePtr(power(e.sampA), powN=257, filterN=30)), ncep=13)
    e.featV = LogFeaturePtr(MelFeaturePtr(power(e.sampV), powN=257, filterN=8))
    fsA = FeatureSetPtr(); fsA.add(e.featA); fsV = FeatureSetPtr(); fsV.add(e.featV)
    e.dssA = DistribSetBasicPtr(CodebookSetBasicPtr(str(tmp / "acb.desc"), fsA, cbA), str(tmp / "ads.desc"), dsA)
    e.dssV = DistribSetBasicPtr(CodebookSetBasicPtr(str(tmp / "vcb.desc"), fsV, cbV), str(tmp / "vds.desc"), dsV)
    # the map 24 -> 6, written to a file and read back
    e.table = ((np.arange(KA_E) * 5 + 2) % KV_E).astype(np.int32); e.table[7] = KV_E - 1
    w = DistribMapPtr()
    for k in range(KA_E):
        w.add("ds%d" % k, "ds%d" % e.table[k])
    w.write(str(tmp / "map.bin"))
    e.map = DistribMapPtr(); e.map.read(str(tmp / "map.bin"))
    assert len(e.map) == KA_E and e.map["ds7"] == "ds%d" % (KV_E - 1) and e.map.mapped("ds0") == "ds2"
    e.wfst = WFSTFlyWeightPtr(LexiconPtr("state"), LexiconPtr("in", str(tmp / "in.lex")), LexiconPtr("out", str(tmp / "out.lex")))
    e.wfst.read(str(tmp / "g.fsm"), binary=False)
    e.x = headset[20000:36000]
    e.sampA.setSamples(e.x, 16000); e.sampV.setSamples(e.x, 16000)
    # the oracle's two score matrices on the device features, once
    XA = np.stack([np.array(v) for v in e.featA]); XV = np.stack([np.array(v) for v in e.featV])
    assert XA.shape[1] == 13 and XV.shape[1] == 8 and XA.shape[0] == XV.shape[0]
    e.soA, _ = oracle.gmm_score_opt(oracle.Codebooks(e.mA["refN"], e.mA["mean"], e.mA["ivar"], e.mA["det"]), e.mA["val"], XA)
    e.soV, _ = oracle.gmm_score_opt(oracle.Codebooks(e.mV["refN"], e.mV["mean"], e.mV["ivar"], e.mV["det"]), e.mV["val"], XV)
    return e


KW = dict(beam=80.0, lmScale=12.0, silPenalty=0.5)


def test_two_model_decode_through_the_operator_face(dsr, oracle, cuda, e2e):
    from dsr.asr.gaussian import DistribSetMultiStreamPtr
    from dsr.asr.decoder import DecoderFlyWeightPtr
    e = e2e
    e.sampA.setSamples(e.x, 16000); e.sampV.setSamples(e.x, 16000)
    dss = DistribSetMultiStreamPtr(e.dssA, e.dssV, e.map)                               # default weights 0.95 / 0.05
    assert dss.ndists() == KA_E and dss.index("ds7") == 7 and dss.find("ds7").name() == "ds7" and dss[3].name() == "ds3"
    assert [d.name() for d in dss] == ["ds%d" % k for k in range(KA_E)]
    assert (dss.find(0).audioWeight(), dss.find(0).videoWeight()) == (0.95, 0.05)
    with pytest.raises(dsr.DsrError) as ex:
        dss.find("nope")
    assert ex.value.status == 11
    d = DecoderFlyWeightPtr(dss, **KW); d.set(e.wfst)
    score = d.decode(); hyp = d.bestHypo()
    soV = e.soV
    so = ms_np.combine(e.soA, soV, e.table, 0.95, 0.05)
    ro = e.go.decode(so, silenceX=4, **KW)
    assert score == ro["score"] and np.array_equal(d.bestArcs(), ro["arcs"])
    assert hyp == "".join(e.outlex[w] + " " for w in ro["words"]) and d._last["frames"] == so.shape[0] - 1
    # find(k).score(t): the same bits the decoder consumed, through the stream protocol
    dss.resetFeature(); dss.resetCache()
    for t in (0, 1, 2):
        for k in (0, 7, KA_E - 1):
            assert dss.find(k).score(t) == so[t, k], (t, k)
    assert e.dssA.find(7).score(2) == e.soA[2, 7]                                       # the child's own row of that frame is the audio score
    with pytest.raises(dsr.DsrError) as ex:
        dss.find(0).score(9)                                                            # out of order: jindex_error
    assert ex.value.status == 6
    # another weight pair changes the score; it takes effect on the cached frame too
    dss.setWeights(0.3, 1.7)
    assert dss.find(7).score(2) == ms_np.combine(e.soA, soV, e.table, 0.3, 1.7)[2, 7]
    s2 = d.decode()
    r2 = e.go.decode(ms_np.combine(e.soA, soV, e.table, 0.3, 1.7), silenceX=4, **KW)
    assert s2 == r2["score"] and np.array_equal(d.bestArcs(), r2["arcs"]) and s2 != score
    # weights (1, 0) reproduce the audio-only decoder's result exactly
    dss.setWeights(1.0, 0.0)
    s1 = d.decode(); a1 = d.bestArcs().copy(); h1 = d.bestHypo()
    da = DecoderFlyWeightPtr(e.dssA, **KW); da.set(e.wfst)
    sa = da.decode()
    r1 = e.go.decode(e.soA, silenceX=4, **KW)
    assert s1 == sa == r1["score"] and np.array_equal(a1, da.bestArcs()) and np.array_equal(a1, r1["arcs"]) and h1 == da.bestHypo()


def test_two_model_lattice_and_gamma_probs(dsr, oracle, cuda, e2e):
    from dsr.asr.gaussian import DistribSetMultiStreamPtr
    from dsr.asr.decoder import DecoderFlyWeightPtr
    e = e2e
    e.sampA.setSamples(e.x, 16000); e.sampV.setSamples(e.x, 16000)
    dss = DistribSetMultiStreamPtr(e.dssA, e.dssV, e.map, 0.8, 0.4)
    d = DecoderFlyWeightPtr(dss, **KW); d.set(e.wfst)
    score = d.decode()
    so = ms_np.combine(e.soA, e.soV, e.table, 0.8, 0.4)
    ro = e.go.decode(so, silenceX=4, lattice=True, eosX=1, **KW)
    assert score == ro["score"]
    Ld = d.lattice().data
    for k in ("nodeFinal", "from", "to", "in", "out", "start", "end"):
        assert np.array_equal(Ld[k], ro["lattice"][k]), k
    assert np.array_equal(Ld["ac"].view(np.int64), ro["lattice"]["ac"].view(np.int64)) and np.array_equal(Ld["lm"].view(np.int64), ro["lattice"]["lm"].view(np.int64))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    olat = importlib.import_module("oracle_lattice")
    lat = d.lattice(); O = olat.Lattice.from_arrays(ro["lattice"])
    for ed in O.allEdges:                                                               # _updateAcNode (lattice.cc:392-409) on the combined scores
        if ed.input != 0 and not ed.prev.final:
            acc = 0.0
            for t in range(ed.start, ed.end + 1):
                acc += float(so[t, ed.input - 1])
            ed.ac = acc
    g1 = lat.gammaProbsDist(dss, 1.0 / 12.0, 12.0, 0.0, 0.5, "SIL-m"); O._clearSorted(); g0 = O.gammaProbs(1.0 / 12.0, 12.0, 0.0, 0.5, 4)
    assert g1 == g0
    sa, sb = lat.state(), O.state()
    for k in ("gamma", "fwd", "bwd"):
        assert np.array_equal(sa[k].view(np.int64), sb[k].view(np.int64)), k


def test_decode_ends_with_the_shorter_stream(dsr, oracle, cuda, e2e):
    from dsr.asr.gaussian import DistribSetMultiStreamPtr
    from dsr.asr.decoder import DecoderFlyWeightPtr
    e = e2e
    TA = e.soA.shape[0]; TV = TA - 30
    e.sampA.setSamples(e.x, 16000); e.sampV.setSamples(e.x[:len(e.x) - 30 * 160], 16000)  # a video source 30 frames shorter
    dss = DistribSetMultiStreamPtr(e.dssA, e.dssV, e.map)
    d = DecoderFlyWeightPtr(dss, **KW); d.set(e.wfst)
    score = d.decode()
    so = ms_np.combine(e.soA[:TV], e.soV[:TV], e.table, 0.95, 0.05)  # the oracle on the truncated matrices
    ro = e.go.decode(so, silenceX=4, **KW)
    assert d._last["frames"] == TV - 1 and score == ro["score"] and np.array_equal(d.bestArcs(), ro["arcs"])
    # the streams end together for the pull protocol too
    dss.resetFeature()
    assert dss.find(1).score(0) == so[0, 1]
    # an empty video source: jiterator_error, status 9
    e.sampV.setSamples(np.zeros(100, np.float32), 16000)
    res = dsr.DecodeResult()
    assert dsr.load().dsr_decoder_decode_stream(d._dec.h, dss._ds, C.byref(res), None, None, 0) == 9
    with pytest.raises(StopIteration):
        d.decode()
    dss.resetFeature()
    with pytest.raises(StopIteration):
        dss.find(0).score(0)


def test_batch_face(dsr, oracle, cuda):
    """U = 3 ragged utterances: Gmm.score twice, MultiStream.combine in place, decode_batch; each utterance equals the oracle"""
    import torch
    U, Tmax, KA, KV = 3, 40, 24, 6
    mA, mV = synth.gmm_model(KA, 4, 13, seed=31), synth.gmm_model(KV, 2, 8, seed=32)
    gA, gV = dsr.Gmm(**mA), dsr.Gmm(**mV)
    table = ((np.arange(KA) * 5 + 1) % KV).astype(np.int32)
    ms = _combiner(dsr, gA, gV, table, 0.7, 0.6)
    rng = np.random.default_rng(33)
    xA, xV = rng.standard_normal((U * Tmax, 13)).astype(np.float32), rng.standard_normal((U * Tmax, 8)).astype(np.float32)
    nfr = [Tmax, Tmax - 7, 2]
    arcs, fin = synth.random_wfst(300, KA, seed=34)
    go, gd = oracle.Wfst(), dsr.Wfst()
    for a in arcs:
        go.add_arc(*a); gd.add_arc(*a)
    for s, c in fin:
        go.add_final(s, c); gd.add_final(s, c)
    sc = ms.score(torch.from_numpy(xA).to(cuda), torch.from_numpy(xV).to(cuda))
    assert tuple(sc.shape) == (U * Tmax, KA)
    soA, _ = oracle.gmm_score_opt(oracle.Codebooks(mA["refN"], mA["mean"], mA["ivar"], mA["det"]), mA["val"], xA)
    soV, _ = oracle.gmm_score_opt(oracle.Codebooks(mV["refN"], mV["mean"], mV["ivar"], mV["det"]), mV["val"], xV)
    so = ms_np.combine(soA, soV, table, 0.7, 0.6)
    assert np.array_equal(sc.cpu().numpy(), so)
    dec = dsr.Decoder(beam=60.0, lmScale=12.0, maxActive=8192, streams=2); dec.set(gd)
    out = dec.decode_batch(sc.view(U, Tmax, KA), torch.tensor(nfr, dtype=torch.int32, device=cuda))
    for u in range(U):
        ro = go.decode(so.reshape(U, Tmax, KA)[u, :nfr[u]], beam=60.0, lmScale=12.0)
        assert out[u]["status"] == 0 and out[u]["score"] == ro["score"] and np.array_equal(out[u]["arcs"], ro["arcs"]), u


def test_errors(dsr, oracle, cuda, e2e):
    import torch
    from dsr.asr.gaussian import DistribSetMultiStreamPtr, DistribMapPtr
    from dsr.asr.decoder import DecoderFlyWeightPtr
    e = e2e; L = dsr.load()
    with pytest.raises(dsr.DsrError) as ex:
        DistribSetMultiStreamPtr(e.dssA, e.dssV)                                        # by name: the video set has no ds6
    assert ex.value.status == 11
    part = DistribMapPtr()
    for k in range(KA_E - 1):
        part.add("ds%d" % k, "ds0")
    with pytest.raises(dsr.DsrError) as ex:
        DistribSetMultiStreamPtr(e.dssA, e.dssV, part)                                  # the map lacks ds23
    assert ex.value.status == 6 and "No mapping for ds23" in str(ex.value)
    part.add("ds23", "absent")
    with pytest.raises(dsr.DsrError) as ex:
        DistribSetMultiStreamPtr(e.dssA, e.dssV, part)                                  # mapped to a name the video set lacks
    assert ex.value.status == 11
    with pytest.raises(dsr.DsrError) as ex:
        M.MultiStream(dsr.Gmm(**e.mA), dsr.Gmm(**e.mV))
    assert ex.value.status == 11
    assert L.dsr_distribset_set_weights(e.dssA._ds, 0.5, 0.5) == 15                     # a plain set
    a, v = C.c_double(), C.c_double()
    assert L.dsr_distribset_get_weights(e.dssA._ds, C.byref(a), C.byref(v)) == 15
    # N = 0 is a no-op; null arguments
    table = (np.arange(KA_E) % KV_E).astype(np.int32)
    ms = _combiner(dsr, dsr.Gmm(**e.mA), dsr.Gmm(**e.mV), table)
    sA = torch.full((2, KA_E), float(SENTINEL), device=cuda); sV = torch.zeros((2, KV_E), device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.dsr_ms_combine(ms.h, p(sA), p(sV), 0, p(sA), None) == 0 and bool((sA == float(SENTINEL)).all())
    assert tuple(ms.combine(sA[:0], sV[:0]).shape) == (0, KA_E)
    assert L.dsr_ms_combine(ms.h, p(sA), p(sV), -1, p(sA), None) == 13
    assert L.dsr_ms_combine(ms.h, p(sA), p(sV), 2, p(sV), None) == 13                  # out never aliases sV
    for st in (L.dsr_ms_combine(None, p(sA), p(sV), 2, p(sA), None), L.dsr_ms_combine(ms.h, None, p(sV), 2, p(sA), None),
               L.dsr_ms_combine(ms.h, p(sA), None, 2, p(sA), None), L.dsr_ms_combine(ms.h, p(sA), p(sV), 2, None, None),
               L.dsr_ms_set_weights(None, 1.0, 0.0), L.dsr_ms_table(ms.h, None),
               L.dsr_distribset_create_multistream(e.dssA._ds, None, None, 0.5, 0.5, C.byref(C.c_void_p())),
               L.dsr_distribset_create_multistream(e.dssA._ds, e.dssV._ds, e.map._map.h, 0.5, 0.5, None)):
        assert st == 13 and L.dsr_last_error() == b"null argument"
    assert bool((sA == float(SENTINEL)).all())
    # a multi-stream set is no child of another
    e.sampA.setSamples(e.x, 16000); e.sampV.setSamples(e.x, 16000)
    dss = DistribSetMultiStreamPtr(e.dssA, e.dssV, e.map)
    h = C.c_void_p()
    assert L.dsr_distribset_create_multistream(dss._ds, e.dssV._ds, None, 0.5, 0.5, C.byref(h)) == 15
    # after destroying the multi-stream set its children still decode
    d = DecoderFlyWeightPtr(dss, **KW); d.set(e.wfst); d.decode()
    del d, dss; gc.collect()
    da = DecoderFlyWeightPtr(e.dssA, **KW); da.set(e.wfst)
    r1 = e.go.decode(e.soA, silenceX=4, **KW)
    assert da.decode() == r1["score"] and np.array_equal(da.bestArcs(), r1["arcs"])
    e.dssV.resetFeature()
    assert np.isfinite(e.dssV.find(0).score(0))
