"""All-pass transform speaker adaptation on the device (include/dsr.h section 13, csrc/apt_kernels.hip, csrc/apt.cpp) against tests/apt_np.py, the
numpy restatement of the one-parameter BLT / SLAPT slice of asr/adapt/transform.cc ("tr") and asr/train/estimateAdapt.cc ("eA").

Tolerances -- derived, not tuned.
  Matrix, apply.  Bit for bit: k_apt_matrix and k_apt_apply do the restatement's operations in its order.
  Likelihood.  apt_np.lhood_bound: eA:1613-1616 holds no float rounding that the device skips (0 x 2^-24); the two fp64 sums over the n used
  Gaussians are reordered (2 n 2^-53 of the sum of the terms' magnitudes).  With a bias, eA:1592-1596 round the two float accumulators of
  every component after every Gaussian: 2 n float roundings a component that the device's fp64 sums skip, (n + 1) 2^-24 of the terms'
  magnitudes for either accumulator; that moves the bias (apt_np.bias_bound), the bias moves float(t + b) by at most as much plus a float
  rounding either side, and a likelihood term by (|sumO| + |c trn|) iv per unit.  All divided by the counts.
  Search.  The restated bracket + brentsMethod replayed on the DEVICE's likelihoods must ask for the device's points, as doubles bit for bit,
  and end at the stored parameter: a comparison that a last-bit difference of two likelihoods could flip is never made.
  Recovery.  |alpha^ - alpha*| <= 4 (0.01 |alpha*| + 1e-10): the interval Brent's method stops at is at most 2 tol2 wide (eA:199-200).
The largest fraction of the likelihood bound seen is printed (-s); DESIGN 4.8g records that of a run."""
import numpy as np
import pytest

from dsr._capi import APT_RAPT, APT_SLAPT, Apt, DsrError
from tests import adapt_np as A
from tests import apt_cases as Cs
from tests import apt_np as P

pytestmark = pytest.mark.gpu
f32 = np.float32
KINDS = [APT_RAPT, APT_SLAPT]
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _gmm(dsr, m, classes):
    g = dsr.Gmm(**m.as_kwargs()); g.set_reg_classes(classes)
    return g


def _case(dsr, si, ti, kind):
    """one estimate per (shape, tree, kind), shared by the checks that read it: the bias type and the number of slots rotate with the case;
    the threshold backs some leaves off"""
    key = (si, ti, kind)
    if key not in _cache:
        L, nSub = Cs.SHAPES[si]; leaves = Cs.TREES[ti]; sizes = Cs.sizes_for(si, ti); biasType = (si + ti + kind) % 3
        S = 3 if sum(sizes) < 200 else 1
        m, classes = Cs.model(L, nSub, sizes, leaves, seed=100 * si + ti)
        c, sumO = Cs.stats(m, S, seed=7 + 100 * si + ti)
        g = _gmm(dsr, m, classes); h = Apt(g, S, kind, L, nSub, biasType)
        for s in range(S):
            h.set_stats(s, c=c[s], sumO=sumO[s])
        threshold = 60.0 if len(leaves) > 1 else -1.0e30
        h.estimate(threshold)
        _cache[key] = dict(L=L, nSub=nSub, leaves=leaves, sizes=sizes, biasType=biasType, S=S, m=m, classes=classes, c=c, sumO=sumO, g=g, h=h,
                           threshold=threshold)
    return _cache[key]


CASES = [(si, ti) for si in range(len(Cs.SHAPES)) for ti in range(len(Cs.TREES))]


# ---- 1. the matrix ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Cs.SHAPES)
def test_matrix_is_the_restatement_bit_for_bit(dsr, cuda, shape):
    L, nSub = shape
    m, classes = Cs.model(L, nSub, [3], [1], seed=1); g = _gmm(dsr, m, classes)
    for kind, plist in ((APT_RAPT, [(a,) for a in Cs.BLT_ALPHAS]), (APT_SLAPT, Cs.SLAPT_PARAMS)):
        h = Apt(g, 1, kind, L, nSub, 0)
        for p in plist:
            h.set_params(0, 1, p)
            got = h.matrix(0, 1); want = P.matrix(kind, p, L)
            assert np.array_equal(_bits(got), _bits(want)), (kind, p, np.abs(got - want).max())
    assert np.array_equal(P.matrix(APT_RAPT, [0.0], L), np.eye(L))


# ---- 2. apply -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(13, 3), (17, 1), (2, 1)])
def test_apply_is_the_restatement_bit_for_bit(dsr, cuda, kind, shape):
    import torch
    L, nSub = shape; D = L * nSub; leaves, sizes, S = [4, 5, 3], [90, 5, 257], 2
    m, classes = Cs.model(L, nSub, sizes, leaves, seed=31); g = _gmm(dsr, m, classes)
    h = Apt(g, S, kind, L, nSub, 2); rng = np.random.default_rng(5); want = []
    for s in range(S):
        ref = P.Params()
        for rc, nb in ((2, D), (3, L), (5, 0)):                                         # class 4 takes its parent's; three bias sizes
            conf = [rng.uniform(-0.4, 0.4)] if kind == APT_RAPT or s == 0 else list(rng.uniform(-0.1, 0.1, 3))
            bias = rng.standard_normal(nb).astype(f32)
            h.set_params(s, rc, conf, bias); p = ref.findAPT(rc, kind); p.conf = np.array(conf); p.bias = bias
        want.append(P.transform_tree(ref, classes, m.mean, L, nSub))
    allm = h.adapt_all().cpu().numpy()
    for s in range(S):
        assert np.array_equal(_bits(allm[s]), _bits(want[s]))
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((70, D)).astype(f32)).to(cuda)
    before = [g.score(x, mode=k)[0].cpu().numpy() for k in (0, 1, 2)]
    h.adapt(1)
    assert np.array_equal(_bits(g.params()["mean"]), _bits(want[1]))
    kw = m.as_kwargs(); kw["mean"] = want[1]; fresh = dsr.Gmm(**kw)
    for k in (0, 1, 2):                                                                 # every scoring mode follows at once
        a = g.score(x, mode=k)[0].cpu().numpy(); b = fresh.score(x, mode=k)[0].cpu().numpy()
        assert np.array_equal(a, b) and not np.array_equal(a, before[k]), k
    h.adapt(0)                                                                          # from the ORIGINAL means, not from speaker 1's
    assert np.array_equal(_bits(g.params()["mean"]), _bits(want[0]))
    h.reset_mean()
    assert np.array_equal(_bits(g.params()["mean"]), _bits(m.mean))
    for k in (0, 1, 2):
        assert np.array_equal(g.score(x, mode=k)[0].cpu().numpy(), before[k])
    st = h.store(0); conf, bias = st.findAPT(5, kind, False); st.clear(); st.set(5, kind, conf, bias)
    for call in (lambda: h.adapt(0), h.adapt_all):                                      # classes 4 and 3 have no node: jkey_error
        with pytest.raises(DsrError) as e:
            call()
        assert e.value.status == 11
    assert np.array_equal(_bits(g.params()["mean"]), _bits(m.mean))


# ---- 3. the likelihood ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("si, ti", CASES)
def test_trace_likelihoods_within_the_bound(dsr, cuda, si, ti, kind):
    k = _case(dsr, si, ti, kind); h = k["h"]; worst = 0.0; n = 0
    for s, node in sorted(set((p[0], p[1]) for p in h.plan())):
        st = P.Stats(k["m"].mean, k["m"].cv, k["c"][s], k["sumO"][s], A.node_gaussians(k["classes"], node), k["L"], k["nSub"], k["biasType"])
        pts, vals, _ = h.trace(s, node)
        assert 3 <= len(pts) <= 40
        for x, v in zip(pts, vals):
            want = P.calc_log_lhood(kind, x, st); bound = P.lhood_bound(kind, x, st)
            assert np.isfinite(v) and abs(v - want) <= bound, (s, node, x, v, want, bound)
            assert bound <= 1.0e-2 * abs(want)                                          # a sanity check of the bound, not a tolerance
            worst = max(worst, abs(v - want) / bound); n += 1
    print("L=%d x %d tree=%s sizes=%s S=%d kind=%d bias=%d: %d points, worst |dev - ref| / bound %.3f" % (
        k["L"], k["nSub"], k["leaves"], k["sizes"], k["S"], kind, k["biasType"], n, worst))


# ---- 4. the search, by replay ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("si, ti", CASES)
def test_search_replayed_on_the_device_likelihoods(dsr, cuda, si, ti, kind):
    k = _case(dsr, si, ti, kind); h = k["h"]
    for s, node, leaf in h.plan():
        pts, vals, biases = h.trace(s, node)
        replay = P.Replay(pts, vals)
        x, seen, _ = P.line_search(kind, replay)
        assert replay.i == len(pts) and np.array_equal(_bits(np.array(seen)), _bits(pts))
        conf, bias = h.get_params(s, leaf)                                              # stored under the LEAF's class
        assert conf.shape == (1,) and _bits(conf)[0] == _bits(np.array([x]))[0]
        at = x if kind == APT_RAPT else pts[-1]                                         # eA:1667-1668 / eA:1926
        st = P.Stats(k["m"].mean, k["m"].cv, k["c"][s], k["sumO"][s], A.node_gaussians(k["classes"], node), k["L"], k["nSub"], k["biasType"])
        want, info = P.calc_bias(P.matrix(kind, [at], k["L"]), st, track=True)
        assert bias.shape == want.shape == (st.bSize,)
        if st.bSize:
            assert np.all(np.abs(bias.astype(np.float64) - want.astype(np.float64)) <= P.bias_bound(info, want))
            e = max(j for j in range(len(pts)) if _bits(pts[j:j + 1])[0] == _bits(np.array([at]))[0])
            assert np.array_equal(_bits(bias), _bits(biases[e]))


# ---- 5. recovery -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", Cs.RECOVERY_SHAPES)
def test_recovery(dsr, cuda, kind, shape):
    """one slot per alpha*: statistics c float(A(alpha*) mu), no bias"""
    L, nSub, G = shape
    m, classes = Cs.model(L, nSub, [G], [1], seed=5, decay=True); g = _gmm(dsr, m, classes)
    h = Apt(g, len(Cs.RECOVERY_ALPHAS), kind, L, nSub, 0)
    for s, alpha in enumerate(Cs.RECOVERY_ALPHAS):
        c, sumO = Cs.recovery_stats(kind, m, L, nSub, alpha, seed=9); h.set_stats(s, c=c, sumO=sumO)
    h.estimate(0.0)
    for s, alpha in enumerate(Cs.RECOVERY_ALPHAS):
        conf, bias = h.get_params(s, 1)
        print("kind %d shape %s alpha* %g: alpha^ %.9g, |diff| / bound %.3f, %d evaluations" % (
            kind, shape, alpha, conf[0], abs(conf[0] - alpha) / Cs.recovery_bound(alpha), len(h.trace(s, 1)[0])))
        assert len(bias) == 0 and abs(conf[0] - alpha) <= Cs.recovery_bound(alpha)


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_estimates_give_the_same_bits(dsr, cuda, kind):
    k = _case(dsr, 1, 2, kind); h = k["h"]
    assert any(p[1] != p[2] for p in h.plan())                                          # the leaf of one Gaussian is backed off to the root
    pairs = sorted(set((p[0], p[1]) for p in h.plan())); first = [h.trace(s, node) for s, node in pairs]
    params = [h.get_params(p[0], p[2]) for p in h.plan()]
    h.estimate(k["threshold"])
    for (s, node), was in zip(pairs, first):
        for a, b in zip(h.trace(s, node), was):
            assert np.array_equal(_bits(a), _bits(b))
    for p, was in zip(h.plan(), params):
        now = h.get_params(p[0], p[2])
        assert np.array_equal(_bits(now[0]), _bits(was[0])) and np.array_equal(_bits(now[1]), _bits(was[1]))


# ---- 7. plan, back-off, flagged slots, files -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("si, ti", CASES)
def test_plan_and_file(dsr, cuda, tmp_path, si, ti, kind):
    k = _case(dsr, si, ti, kind); h = k["h"]; want = []
    _, nodes = A.tree_nodes(k["classes"])
    assert h.nodes()[0] == nodes and [n for n, l in zip(*h.nodes()) if l] == sorted(k["leaves"])
    for s in range(k["S"]):
        plan, ttl = P.plan_tree(k["classes"], k["c"][s], k["threshold"], s); want += plan
        for node in nodes:
            assert h.ttl_frames(s, node) == ttl[node]                                   # a double sum in model order, as there
    assert [tuple(int(v) for v in p) for p in h.plan()] == want
    for s in range(k["S"]):
        assert h.speaker_status(s) == 0 and h.store(s).indices() == sorted(k["leaves"]) and h.store(s).type() == kind
        ref = P.Params()
        for leaf in k["leaves"]:
            p = ref.findAPT(leaf, kind); p.conf, p.bias = h.get_params(s, leaf)
        out = str(tmp_path / ("s%d.par" % s)); h.write(s, out)
        assert open(out).read() == ref.text()
        h2 = dsr.AptParams(out); assert h2.indices() == sorted(k["leaves"])
        t = dsr.ParamTree()                                                             # the MLLR tree keeps refusing these files
        with pytest.raises(DsrError) as e:
            t.read(out)
        assert e.value.status == 15


@pytest.mark.parametrize("kind", KINDS)
def test_a_slot_with_a_nan_statistic_keeps_its_parameters(dsr, cuda, kind):
    L, nSub = 13, 3
    m, classes = Cs.model(L, nSub, [9, 9], [2, 3], seed=21); g = _gmm(dsr, m, classes)
    c, sumO = Cs.stats(m, 3, seed=22, mmi=False); sumO[1, 4, 1] = np.nan
    h = Apt(g, 3, kind, L, nSub, 1)
    for s in range(3):
        h.set_stats(s, c=c[s], sumO=sumO[s])
    h.set_params(1, 5, [0.125], np.arange(L, dtype=f32))
    with pytest.raises(DsrError) as e:
        h.estimate(0.0)
    assert e.value.status == 4                                                          # jconsistency_error
    assert [h.speaker_status(s) for s in range(3)] == [0, 4, 0]
    conf, bias = h.get_params(1, 5)
    assert h.store(1).indices() == [5] and conf[0] == 0.125 and np.array_equal(bias, np.arange(L, dtype=f32))
    assert h.store(0).indices() == [2, 3] and h.store(2).indices() == [2, 3]
    bad = int(classes[4])
    pts, vals, _ = h.trace(1, bad)
    assert len(pts) == 1 and np.isnan(vals[0])                                          # bracket's first evaluation (eA:122)
    for s in (0, 2):                                                                    # the others are what they are alone
        st = P.Stats(m.mean, m.cv, c[s], sumO[s], A.node_gaussians(classes, 2), L, nSub, 1)
        pts, vals, _ = h.trace(s, 2)
        assert abs(vals[-1] - P.calc_log_lhood(kind, pts[-1], st)) <= P.lhood_bound(kind, pts[-1], st)


# ---- 8. what is refused ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dsr, cuda):
    L, nSub = 13, 3
    m, classes = Cs.model(L, nSub, [5, 4], [2, 3], seed=1); g = _gmm(dsr, m, classes)
    for args, status in (((g, 1, 3, L, nSub, 0), 13), ((g, 1, APT_SLAPT, L, 4, 0), 13), ((g, 1, APT_SLAPT, 12, nSub, 0), 5),
                         ((g, 1, APT_SLAPT, 39, 1, 3), 15), ((g, 0, APT_SLAPT, L, nSub, 0), 13), ((g, 1, APT_SLAPT, 39, 1, 0), 0)):
        if status == 0:
            Apt(*args); continue
        with pytest.raises(DsrError) as e:
            Apt(*args)
        assert e.value.status == status, args[1:]
    h = Apt(g, 1, APT_RAPT, L, nSub, 0)
    with pytest.raises(DsrError) as e:
        h.set_param_n(2)                                                                # the Newton search is not implemented
    assert e.value.status == 13
    h.set_param_n(1)
    for conf in ([0.1, 0.2, 0.3], [1.0], [-1.5]):                                       # RAPT beyond the bilinear transform; |mu| >= 1
        h.store(0).clear(); h.set_params(0, 1, conf)
        for call in (lambda: h.matrix(0, 1), lambda: h.adapt(0)):
            with pytest.raises(DsrError) as e:
                call()
            assert e.value.status == 13
    c, sumO = Cs.stats(m, 1, seed=2, mmi=False); h.set_stats(0, c=c[0], sumO=sumO[0])
    h.store(0).clear(); h.set_params(0, 1, [0.1, 0.2, 0.3])
    with pytest.raises(DsrError) as e:
        h.estimate(0.0)                                                                 # " No. of all-pass parameters (3) is incorrect."
    assert e.value.status == 4 and h.store(0).indices() == [1]
    h.store(0).clear(); h.store(0).set(1, APT_SLAPT, [0.1])
    with pytest.raises(DsrError) as e:
        h.estimate(0.0)                                                                 # "Tree not instantiated with RAPT parameters."
    assert e.value.status == 4
    h2 = Apt(g, 1, APT_SLAPT, L, nSub, 2); h2.set_stats(0, c=c[0], sumO=sumO[0]); h2.set_params(0, 2, [0.1], np.zeros(L, f32))
    with pytest.raises(DsrError) as e:
        h2.estimate(0.0)                                                                # "Feature lengths (13 vs. 39) do not match."
    assert e.value.status == 5
    assert h2.store(0).indices() == [2]
    h2.store(0).clear(); h2.set_params(0, 1, [0.1], np.zeros(7, f32))
    with pytest.raises(DsrError) as e:
        h2.adapt(0)                                                                     # a bias of 7 entries for sub-features of 13
    assert e.value.status == 4
    g0 = dsr.Gmm(**m.as_kwargs()); h3 = Apt(g0, 1, APT_SLAPT, L, nSub, 0); h3.set_stats(0, c=c[0], sumO=sumO[0])
    with pytest.raises(DsrError) as e:
        h3.estimate(0.0)                                                                # no regression classes: class 0
    assert e.value.status == 6


# ---- the reference's names -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_reference_names_two_pass_adaptation(dsr, cuda, tmp_path, kind):
    """dsr.asr.adapt / dsr.asr.train under the reference's names: accumulate(path), EstimatorTreeSLAPTPtr / EstimatorTreeBLTPtr +
    estimateAdaptationParameters, writeParams, adaptCbk from the tree and from the written file, resetMean; the transformers on their own"""
    import torch
    from tests import train_np as T
    from dsr.btk.feature import (SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr, MelFeaturePtr, LogFeaturePtr,
                                 CepstralFeaturePtr, FeatureSetPtr)
    from dsr.asr.adapt import APTParamTreePtr, BLTTransformer, RAPTParam, SLAPTParam, SLAPTTransformer, adaptCbk
    from dsr.asr.train import CodebookSetTrainPtr, DistribSetTrainPtr, EstimatorTreeBLTPtr, EstimatorTreeSLAPTPtr, estimateAdaptationParameters
    K, R, D = 4, 6, 13; rng = np.random.default_rng(5)
    m = T.random_model([R] * K, D, seed=90, spread=3.0)
    m.mean = (m.mean / (1.0 + np.arange(D))[None, :] ** 2).astype(f32)
    classes = np.repeat(np.array([2, 3, 3, 2], np.uint16), R)
    g0 = dsr.Gmm(**m.as_kwargs()); g0.set_reg_classes(classes)
    cbf, dsf = str(tmp_path / "cb.bin"), str(tmp_path / "ds.bin"); g0.save(cbf, dsf)
    open(tmp_path / "cb.desc", "w").write("".join("%-25s%-20s%-10d%-3d%-10s\n" % ("cb%d" % k, "Cepstral", R, D, "DIAGONAL") for k in range(K)))
    open(tmp_path / "ds.desc", "w").write("".join("%-25s%-25s\n" % ("ds%d" % k, "cb%d" % k) for k in range(K)))
    samp = SampleFeaturePtr(blockLen=320, shiftLen=160)
    feat = CepstralFeaturePtr(LogFeaturePtr(MelFeaturePtr(SpectralPowerFeaturePtr(FFTFeaturePtr(HammingFeaturePtr(samp), fftLen=512), powN=257),
                                                         powN=257, filterN=30)), ncep=13)
    fs = FeatureSetPtr(); fs.add(feat)
    cbs = CodebookSetTrainPtr(str(tmp_path / "cb.desc"), fs, cbf)
    dss = DistribSetTrainPtr(cbs, str(tmp_path / "ds.desc"), dsf)
    cbs.setSubFeatures(13, 1)
    ids = np.repeat(np.arange(K), 150); rng.shuffle(ids)
    warped = m.copy(); warped.mean = P.transform(P.matrix(kind, [0.15], D), m.mean, 1)
    x = np.concatenate([T.sample(warped, int(k), 1, rng) for k in ids]).astype(f32)
    dss.setFeatures(torch.from_numpy(x).to(cuda))
    before = dss.accumulate(["ds%d" % k for k in ids], 1.0)
    pt = APTParamTreePtr()
    with pytest.raises(DsrError) as e:
        EstimatorTreeSLAPTPtr(cbs, pt, "CepstraOnly", paramN=9)                         # the reference's default: its Newton search
    assert e.value.status == 13
    Tree = EstimatorTreeBLTPtr if kind == APT_RAPT else EstimatorTreeSLAPTPtr
    tree = Tree(cbs, pt, "CepstraOnly", threshold=250.0)
    estimateAdaptationParameters(tree)
    assert pt.indices() == [2, 3] and pt.type() == kind and abs(tree.ttlFrames() - 2 * len(ids)) < 1e-6 * len(ids)
    own = P.Params()
    for rc in (2, 3):
        conf, bias = pt.findAPT(rc, kind, False); p = own.findAPT(rc, kind); p.conf, p.bias = conf, bias
        assert len(conf) == 1 and len(bias) == 13
    out = str(tmp_path / "spk.apt"); tree.writeParams(out)
    assert open(out).read() == own.text()
    adaptCbk(cbs, pt)
    want = P.transform_tree(own, classes, m.mean, 13, 1)
    assert np.array_equal(_bits(dss.gmm.params()["mean"]), _bits(want))
    cbs.zeroAccus(); dss.zeroAccus()
    assert dss.accumulate(["ds%d" % k for k in ids], 1.0) < before
    cbs.resetMean()
    assert np.array_equal(_bits(dss.gmm.params()["mean"]), _bits(m.mean))
    adaptCbk(cbs, APTParamTreePtr(out))                                                 # second pass from the file: %g keeps six digits
    assert np.allclose(dss.gmm.params()["mean"], want, rtol=0, atol=1e-3)
    par = (RAPTParam if kind == APT_RAPT else SLAPTParam)(own.map[2].conf, own.map[2].bias, 2)
    tr = par.transformer(13, 1)
    assert isinstance(tr, BLTTransformer if kind == APT_RAPT else SLAPTTransformer)
    A2 = P.matrix(kind, own.map[2].conf, 13)
    assert np.array_equal(_bits(tr.matrix()), _bits(A2))
    assert np.array_equal(_bits(tr.transform(m.mean[:5])), _bits(P.transform(A2, m.mean[:5], 1, own.map[2].bias)))
    assert np.array_equal(_bits(tr.transform(m.mean[:5], useBias=False)), _bits(P.transform(A2, m.mean[:5], 1)))
    with pytest.raises(DsrError) as e:
        BLTTransformer(1.0, 13, 1)                                                      # "Mu value (1) is not < 1.0"
    assert e.value.status == 13
