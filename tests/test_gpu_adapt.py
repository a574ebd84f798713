"""MLLR speaker adaptation on the device (include/dsr.h section 10, csrc/k_mllr.hip, csrc/adapt.cpp) against tests/adapt_np.py, the numpy
restatement of the MLLR branch of asr/adapt/transform.cc ("tr") and asr/train/estimateAdapt.cc ("eA").

Tolerances -- derived, not tuned.
  Statistics.  A term of G_i is, in the reference, float(c) * iv * xi_m * xi_n with a float rounding after the cast and after each of the three
  products (eA:2136-2148: `float ck`, `float term = ck * invVar`, `term * mn_m * mn_n` are all float): four roundings that the fp64
  contraction skips, 4 * 2^-24 relative to the sum of the terms' magnitudes.  A term of z_i is float(sumO * iv) * xi_n (eA:2113-2117: the
  product sumO * invVar is double and rounded once into `float term`, then `term * mn` is a float product): 2 * 2^-24.  The sum over n
  Gaussians is reordered in fp64: n * 2^-53 of the same.  ttlFrames is a plain fp64 sum, reordered by chunk and leaf: 2 n 2^-53 sum |c|.
  Solves.  Against numpy.linalg.svd on the device-made G, z with the margins the test docstrings state.
The largest ratios seen are printed (-s); DESIGN 4.8d records those of a run."""
import numpy as np
import pytest

from dsr._capi import DsrError, Mllr, Trainer
from tests import adapt_np as A
from tests import train_np as T

pytestmark = pytest.mark.gpu
f32 = np.float32
TREES = [[1], [2, 3], [4, 5, 3], [2, 7]]
SIZES = [1, 3, 4, 5, 63, 64, 65, 257]                   # Gaussians per leaf: around the MFMA k-step (4) and the chunk (64), several chunks
DIMS = [1, 3, 15, 16, 39, 40]


def _refNs(G, most=50):
    r = [most] * (G // most)
    if G % most:
        r.append(G % most)
    return r


def _model(dsr, D, leafSizes, leaves, seed):
    """a model whose Gaussians carry the classes `leaves`, leafSizes[j] of them in class leaves[j], shuffled over the codebooks"""
    rng = np.random.default_rng(seed); G = int(sum(leafSizes))
    m = T.random_model(_refNs(G), D, seed)
    classes = rng.permutation(np.concatenate([np.full(n, l, np.uint16) for n, l in zip(leafSizes, leaves)]))
    g = dsr.Gmm(**m.as_kwargs()); g.set_reg_classes(classes)
    return m, g, classes


def _stats(m, S, seed, mmi=True):
    """per speaker counts with exact zeros (whose sumO is not zero), counts that round to float zero, and negative counts (MMI)"""
    rng = np.random.default_rng(seed); c = rng.uniform(0.5, 30.0, (S, m.G))
    if mmi:
        kind = rng.random((S, m.G))
        c[kind < 0.10] = 0.0; c[(kind >= 0.10) & (kind < 0.13)] = 1.0e-50; c[(kind >= 0.13) & (kind < 0.30)] *= -1.0
    sumO = (np.abs(c) + 1.0)[:, :, None] * (m.mean[None].astype(np.float64) + 0.7 * rng.standard_normal((S, m.G, m.D)))
    return c, sumO


def _sizes_for(di, ti):
    """every D meets every leaf size once: the eight leaves of the four trees take the eight sizes, rotated by the dimension's index"""
    first = sum(len(t) for t in TREES[:ti])
    return [SIZES[(first + j + di) % len(SIZES)] for j in range(len(TREES[ti]))]


@pytest.mark.parametrize("ti", range(len(TREES)))
@pytest.mark.parametrize("di", range(len(DIMS)))
def test_statistics_match_the_restatement(dsr, cuda, di, ti):
    D, leaves = DIMS[di], TREES[ti]; sizes = _sizes_for(di, ti); S = 3 if len(leaves) < 3 and sum(sizes) < 200 else 1
    m, g, classes = _model(dsr, D, sizes, leaves, seed=100 * di + ti)
    c, sumO = _stats(m, S, seed=7 + 100 * di + ti)
    h = Mllr(g, S)
    for s in range(S):
        h.set_stats(s, c=c[s], sumO=sumO[s])
    h.estimate(-1.0e30)
    _, nodes = A.tree_nodes(classes)
    assert h.nodes()[0] == nodes and [n for n, l in zip(*h.nodes()) if l] == sorted(leaves)
    worstG = worstZ = 0.0
    for s in range(S):
        for node in nodes:
            gs = A.node_gaussians(classes, node)
            G, Z, ttl, aG, aZ, used = A.calc_stats(m.mean, m.cv, c[s], sumO[s], gs, track=True)
            assert abs(h.ttl_frames(s, node) - ttl) <= 2 * len(gs) * 2.0 ** -53 * np.abs(c[s][gs]).sum()
            bG = (4 * 2.0 ** -24 + used * 2.0 ** -53) * aG; bZ = (2 * 2.0 ** -24 + used * 2.0 ** -53) * aZ
            for i in range(D):
                Gd, zd = h.stats(s, node, i)
                assert np.array_equal(Gd, Gd.T)
                eG = np.abs(Gd - G[i]); eZ = np.abs(zd - Z[i])
                assert np.all(eG <= bG[i]) and np.all(eZ <= bZ[i]), (s, node, i, float((eG - bG[i]).max()), float((eZ - bZ[i]).max()))
                if used:
                    worstG = max(worstG, float((eG[bG[i] > 0] / bG[i][bG[i] > 0]).max())); worstZ = max(worstZ, float((eZ[bZ[i] > 0] / bZ[i][bZ[i] > 0]).max()))
    print("D=%d tree=%s sizes=%s S=%d: worst |dev - ref| / bound  G %.3f  z %.3f" % (D, leaves, sizes, S, worstG, worstZ))


def test_same_call_twice_gives_the_same_bits(dsr, cuda):
    D, leaves, sizes = 39, [4, 5, 3], [65, 130, 7]
    m, g, classes = _model(dsr, D, sizes, leaves, seed=5)
    c, sumO = _stats(m, 2, seed=6)
    h = Mllr(g, 2)
    for s in range(2):
        h.set_stats(s, c=c[s], sumO=sumO[s])
    runs = []
    for _ in range(2):
        h.estimate(100.0)
        runs.append(([h.stats(s, n, i) for s in range(2) for n in (1, 2, 5) for i in (0, 17, 38)], [h.ttl_frames(s, n) for s in range(2) for n in (1, 2, 3, 4, 5)],
                     h.plan().copy(), [h.transform(s, l) for s in range(2) for l in leaves]))
    for (Ga, za), (Gb, zb) in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(Ga, Gb) and np.array_equal(za, zb)
    assert runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][3], runs[1][3]))


def test_class_zero_is_refused(dsr, cuda):
    m, g, classes = _model(dsr, 3, [5, 4], [2, 3], seed=1)
    cl = classes.copy(); cl[3] = 0; g.set_reg_classes(cl)
    h = Mllr(g, 1)
    with pytest.raises(DsrError) as e:
        h.estimate(0.0)
    assert e.value.status == 6                                                          # jindex_error of _setNode(0), tr:2019-2023
    m2 = T.random_model([3], 3, 2); g2 = dsr.Gmm(**m2.as_kwargs())                      # no table at all: regClass() is 0 for everybody
    assert g2.reg_classes() is None
    with pytest.raises(DsrError) as e:
        Mllr(g2, 1).estimate(0.0)
    assert e.value.status == 6


def _eta(G, w, z):
    return np.linalg.norm(G @ w - z) / (np.linalg.norm(G, 2) * np.linalg.norm(w) + np.linalg.norm(z))


@pytest.mark.parametrize("D", [1, 3, 15, 16, 39, 40])
def test_solve_against_lapack_on_the_device_made_statistics(dsr, cuda, D):
    """Leaf 2 has 2 (D + 1) + 3 Gaussians (full rank), leaf 3 has (D + 1) // 2 (deficient); positive counts.  Both are solved at themselves.
    Full rank: the normwise backward error of the device's w_i is within 8x LAPACK's (numpy.linalg.svd with the same 1e-7 rule) on the same
    G_i, z_i -- ten-odd Jacobi sweeps against one reduction.  Deficient: the kept rank is numpy's and the distance to numpy's truncated solution
    is within 8x the larger of numpy's own SVD-route / eigh-route difference and (D + 1) 2^-53 sigma_1 / sigma_r."""
    n = D + 1; sizes = [2 * n + 3, max(1, n // 2)]
    m, g, classes = _model(dsr, D, sizes, [2, 3], seed=40 + D)
    c, sumO = _stats(m, 1, seed=50 + D, mmi=False)
    h = Mllr(g, 1); h.set_stats(0, c=c[0], sumO=sumO[0]); h.estimate(-1.0e30)
    assert [tuple(r) for r in h.plan()] == [(0, 2, 2, 0), (0, 3, 3, 0)]
    worst = [0.0, 0.0]
    for leaf, full in ((2, True), (3, False)):
        W = h.transform(0, leaf)
        for i in range(D):
            Gi, zi = h.stats(0, leaf, i)
            sv = np.linalg.svd(Gi, compute_uv=False); ratio = sv / sv[0]
            assert not np.any((ratio >= 1e-9) & (ratio <= 1e-5)), ratio                # precondition: no singular value near the 1e-7 rule
            wn, rank = A.svd_solve(Gi, zi)
            if full:
                assert rank == n
                ed, en = _eta(Gi, W[i], zi), _eta(Gi, wn, zi)
                assert ed <= 8 * max(en, 2.0 ** -53), (leaf, i, ed, en)
                worst[0] = max(worst[0], ed / max(en, 2.0 ** -53))
            else:
                assert rank == sizes[1] < n or D == 1
                lam, V = np.linalg.eigh(Gi); keep = np.abs(lam) / np.abs(lam).max() >= 1e-7
                assert keep.sum() == rank
                we = V[:, keep] @ ((V[:, keep].T @ zi) / lam[keep])
                allow = 8 * max(np.linalg.norm(wn - we), n * 2.0 ** -53 * sv[0] / sv[rank - 1] * np.linalg.norm(wn))
                err = np.linalg.norm(W[i] - wn)
                assert err <= allow, (leaf, i, err, allow)
                # the device kept the same rank: its w lies in the range of the kept eigenvectors
                out = W[i] - V[:, keep] @ (V[:, keep].T @ W[i])
                assert np.linalg.norm(out) <= allow
                worst[1] = max(worst[1], err / (allow / 8))
    print("D=%d: full rank eta_dev / eta_lapack <= %.2f; deficient forward error / allowance base <= %.2f" % (D, worst[0], worst[1]))


def _restated_run(h, classes, S, threshold, D):
    """the restatement's back-off and solves on the DEVICE-made statistics -> trees, plan"""
    trees, plan = [], []
    for s in range(S):
        ttl = {node: h.ttl_frames(s, node) for node in h.nodes()[0]}

        def solve(node, s=s):
            return np.stack([A.svd_solve(*h.stats(s, node, i))[0] for i in range(D)])
        t, p = A.estimate_tree(classes, ttl, solve, threshold, speaker=s)
        trees.append(t); plan += p
    return trees, plan


def _close(a, b):
    """values of two solves of well-conditioned systems: 1e-5 of the transform's largest entry"""
    return np.abs(a - b).max() <= 1e-5 * np.abs(b).max()


def test_back_off_transforms_and_files(dsr, cuda, tmp_path):
    D, leaves, sizes, S = 5, [4, 5, 3, 12], [30, 3, 40, 2], 3
    m, g, classes = _model(dsr, D, sizes, leaves, seed=11)
    c, sumO = _stats(m, S, seed=12, mmi=False)
    c[1] *= 0.05                                                                        # speaker 1: hardly any data anywhere
    c[2, classes == 12] = 1000.0                                                        # speaker 2: the small leaf 12 has enough, 5 has not
    h = Mllr(g, S)
    for s in range(S):
        h.set_stats(s, c=c[s], sumO=sumO[s])
    thr = 100.0
    h.tree(1).set(9, np.ones((D, D + 1)))                                               # estimate starts from a cleared tree
    h.estimate(thr)
    trees, plan = _restated_run(h, classes, S, thr, D)
    assert [tuple(r) for r in h.plan()] == plan
    copies = [p for p in plan if p[3]]; backoffs = [p for p in plan if not p[3] and p[1] != p[2]]
    assert copies and backoffs and any(p[1] == 1 for p in plan)                         # the case holds copies, back-offs and the root
    for s in range(S):
        dev = h.tree(s)
        assert dev.indices() == sorted(trees[s].map) and dev.type() == 3
        for rc in dev.indices():
            assert _close(dev.find(rc, False), trees[s].map[rc].W()), (s, rc)
        for _, node, leaf, copy in [p for p in plan if p[0] == s]:
            assert np.array_equal(dev.find(leaf, False), dev.find(node, False))         # stored twice / copied: the same bits
        out = str(tmp_path / ("spk%d.mllr" % s)); h.write(s, out); text = open(out).read()
        own = A.ParamTree()
        for rc in dev.indices():
            own.findMLLR(rc).assign(dev.find(rc, False))
        assert text == own.text()                                                       # the writer, byte for byte, on the device's own values
        if text != trees[s].text():                                                     # last-bit differences of the two solves may show in %g
            back = A.ParamTree(text)
            assert all(_close(back.map[rc].W(), trees[s].map[rc].W()) for rc in back.map)
        h2 = Mllr(g, 1); h2.read(0, out)
        assert h2.tree(0).indices() == dev.indices()
        assert all(np.allclose(h2.transform(0, rc), dev.find(rc, False), rtol=1e-5, atol=0) for rc in dev.indices())


def test_a_speaker_with_non_finite_statistics_keeps_its_tree(dsr, cuda):
    D = 3; m, g, classes = _model(dsr, D, [9, 9], [2, 3], seed=21)
    c, sumO = _stats(m, 2, seed=22, mmi=False); sumO[1, 4, 1] = np.inf
    h = Mllr(g, 2)
    for s in range(2):
        h.set_stats(s, c=c[s], sumO=sumO[s])
    mark = np.arange(12.0).reshape(3, 4); h.tree(1).set(5, mark)
    with pytest.raises(DsrError) as e:
        h.estimate(0.0)
    assert e.value.status == 4                                                          # jconsistency_error
    assert h.speaker_status(0) == 0 and h.speaker_status(1) == 4
    assert h.tree(1).indices() == [5] and np.array_equal(h.tree(1).find(5, False), mark)
    assert h.tree(0).indices() == [2, 3]


def test_apply_is_the_restatement_bit_for_bit(dsr, cuda):
    import torch
    D, leaves, sizes, S = 39, [4, 5, 3], [90, 5, 85], 2
    m, g, classes = _model(dsr, D, sizes, leaves, seed=31)
    c, sumO = _stats(m, S, seed=32, mmi=False)
    h = Mllr(g, S)
    for s in range(S):
        h.set_stats(s, c=c[s], sumO=sumO[s])
    h.estimate(150.0)
    assert any(p[3] for p in h.plan()) or any(p[1] != p[2] for p in h.plan())          # leaf 5 is backed off
    want = []
    for s in range(S):
        own = A.ParamTree()
        for rc in h.tree(s).indices():
            own.findMLLR(rc).assign(h.tree(s).find(rc, False))
        want.append(A.transform_tree(own, classes, m.mean))
    allm = h.adapt_all().cpu().numpy()
    for s in range(S):
        assert np.array_equal(allm[s].view(np.uint32), want[s].view(np.uint32))
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((70, D)).astype(f32)).to(cuda)
    before = [g.score(x, mode=k)[0].cpu().numpy() for k in (0, 1, 2)]
    h.adapt(1)
    assert np.array_equal(g.params()["mean"].view(np.uint32), want[1].view(np.uint32))
    kw = m.as_kwargs(); kw["mean"] = want[1]; fresh = dsr.Gmm(**kw)
    for k in (0, 1, 2):                                                                 # every scoring mode follows at once
        a = g.score(x, mode=k)[0].cpu().numpy(); b = fresh.score(x, mode=k)[0].cpu().numpy()
        assert np.array_equal(a, b) and not np.array_equal(a, before[k]), k
    h.adapt(0)                                                                          # from the ORIGINAL means, not from speaker 1's
    assert np.array_equal(g.params()["mean"].view(np.uint32), want[0].view(np.uint32))
    h.reset_mean()
    assert np.array_equal(g.params()["mean"].view(np.uint32), m.mean.view(np.uint32))
    for k in (0, 1, 2):
        assert np.array_equal(g.score(x, mode=k)[0].cpu().numpy(), before[k])
    # a class without a transform or an ancestor with one: jkey_error, the model as it was
    t = h.tree(0); W = t.find(4, False); t.clear(); t.set(4, W)
    with pytest.raises(DsrError) as e:
        h.adapt(0)
    assert e.value.status == 11
    with pytest.raises(DsrError) as e:
        h.adapt_all()
    assert e.value.status == 11
    assert np.array_equal(g.params()["mean"].view(np.uint32), m.mean.view(np.uint32))


def test_codebook_files_carry_the_regression_classes(dsr, cuda, tmp_path):
    """load, save and round trip byte for byte; a model without the table is written as before; split hands the class down"""
    m = T.random_model([2, 3, 1], 4, seed=8); m.count = np.arange(1, 7).astype(f32)
    classes = [4, 5, 3, 4, 4, 7]
    ds = tmp_path / "ds.bin"; ds.write_bytes(A.distrib_file(m))
    for name, cl in (("plain", None), ("table", classes)):
        cb = tmp_path / (name + ".cbk"); cb.write_bytes(A.codebook_file(m, cl))
        g = dsr.Gmm(files=(str(cb), str(ds)))
        got = g.reg_classes()
        assert (got is None) if cl is None else (list(got) == cl)
        o1, o2 = str(tmp_path / (name + ".out")), str(tmp_path / (name + ".dso")); g.save(o1, o2)
        assert open(o1, "rb").read() == cb.read_bytes() and open(o2, "rb").read() == ds.read_bytes()
    cb = tmp_path / "multi.cbk"; cb.write_bytes(A.codebook_file(m, [[4, 9], [5], [], [4], [4, 1, 2], [7]]))
    g = dsr.Gmm(files=(str(cb), str(ds)))
    assert list(g.reg_classes()) == [4, 5, 0, 4, 4, 7]                                  # the first class; 0 without one (codebookBasic.h:275-280)
    g.set_reg_classes(3); assert list(g.reg_classes()) == [3] * 6
    g.set_reg_classes(classes)
    t = Trainer(g); t.split(1, 0.0, 0.2)                                                # codebook 1: its Gaussian of the largest count is the last (class 4)
    assert list(g.reg_classes()) == [4, 5, 3, 4, 4, 4, 7]


def test_end_to_end_path_statistics_adapt_the_model(dsr, cuda):
    """frames drawn from means moved by a known (A | b); path -> Trainer.accumulate_path -> Mllr.set_stats -> estimate -> adapt lowers the path
    score of the same frames, and W is within twice the CPU restatement's own distance from (A | b) on the same accumulators"""
    import torch
    D, K, R = 6, 3, 8; rng = np.random.default_rng(77)
    m = T.random_model([R] * K, D, seed=70, spread=3.0)
    Wtrue = np.concatenate([np.eye(D) + 0.1 * rng.standard_normal((D, D)), 0.8 * rng.standard_normal((D, 1))], axis=1)
    moved = m.copy(); moved.mean = A.transform_means(Wtrue, m.mean)
    ids = np.repeat(np.arange(K), 400).astype(np.int32); rng.shuffle(ids)
    x = np.concatenate([T.sample(moved, int(k), 1, rng) for k in ids]).astype(f32)
    g = dsr.Gmm(**m.as_kwargs()); g.set_reg_classes(1)
    xd = torch.from_numpy(x).to(cuda)
    t = Trainer(g); before = t.accumulate_path(xd, ids)
    h = Mllr(g, 1); h.set_stats(0, t); h.estimate(1000.0)
    assert [tuple(r) for r in h.plan()] == [(0, 1, 1, 0)] and abs(h.ttl_frames(0, 1) - len(ids)) < 1e-6 * len(ids)
    acc = t.get()
    G, Z, _ = A.calc_stats(m.mean, m.cv, acc["count"] - acc["den"], acc["sumO"], range(m.G))
    Wnp = A.estimate_W(G, Z); Wdev = h.transform(0, 1)
    dnp, ddev = np.linalg.norm(Wnp - Wtrue), np.linalg.norm(Wdev - Wtrue)
    print("|W - (A|b)|: restatement %.4g, device %.4g" % (dnp, ddev))
    assert ddev <= 2 * dnp
    h.adapt(0)
    t2 = Trainer(g); after = t2.accumulate_path(xd, ids)
    assert after < before, (before, after)


def test_reference_names_two_pass_adaptation(dsr, cuda, tmp_path):
    """dsr.asr.adapt / dsr.asr.train under the reference's names: a codebook file that carries the classes, accumulate(path),
    EstimatorTreeMLLRPtr + estimateAdaptationParameters, writeParams, adaptCbk from the written file, resetMean"""
    import torch
    from dsr.btk.feature import (SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr, MelFeaturePtr, LogFeaturePtr,
                                 CepstralFeaturePtr, FeatureSetPtr)
    from dsr.asr.adapt import ParamTreePtr, adaptCbk
    from dsr.asr.train import CodebookSetTrainPtr, DistribSetTrainPtr, EstimatorTreeMLLRPtr, estimateAdaptationParameters
    K, R, D = 4, 6, 13; rng = np.random.default_rng(5)
    m = T.random_model([R] * K, D, seed=90, spread=3.0)
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
    assert list(dss.gmm.reg_classes()) == list(classes)
    ids = np.repeat(np.arange(K), 150); rng.shuffle(ids)
    shifted = m.copy(); shifted.mean = (m.mean + f32(0.6)).astype(f32)
    x = np.concatenate([T.sample(shifted, int(k), 1, rng) for k in ids]).astype(f32)
    dss.setFeatures(torch.from_numpy(x).to(cuda))
    before = dss.accumulate(["ds%d" % k for k in ids], 1.0)
    pt = ParamTreePtr()
    tree = EstimatorTreeMLLRPtr(cbs, pt, trace=1, threshold=250.0)
    estimateAdaptationParameters(tree)
    assert pt.indices() == [2, 3] and pt.type() == 3 and abs(tree.ttlFrames() - 2 * len(ids)) < 1e-6 * len(ids)      # nodes 1, 2, 3
    out = str(tmp_path / "spk.mllr"); tree.writeParams(out)
    own = A.ParamTree()
    for rc in (2, 3):
        own.findMLLR(rc).assign(pt.find(rc, False))
    assert open(out).read() == own.text()
    adaptCbk(cbs, pt)
    assert np.array_equal(dss.gmm.params()["mean"].view(np.uint32), A.transform_tree(own, classes, m.mean).view(np.uint32))
    cbs.zeroAccus(); dss.zeroAccus()
    after = dss.accumulate(["ds%d" % k for k in ids], 1.0)
    assert after < before
    cbs.resetMean()
    assert np.array_equal(dss.gmm.params()["mean"].view(np.uint32), m.mean.view(np.uint32))
    adaptCbk(cbs, ParamTreePtr(out))                                                    # second pass from the file: %g keeps six digits
    assert np.allclose(dss.gmm.params()["mean"], A.transform_tree(own, classes, m.mean), rtol=0, atol=1e-3)
    with pytest.raises(DsrError) as e:
        cbs.setRegClasses(1)                                                            # after the originals were taken
    assert e.value.status == 4
