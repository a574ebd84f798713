"""GMM training on the device (include/dsr.h section 9, csrc/k_train.hip, csrc/train.cpp) against tests/train_np.py, the numpy restatement
of asr/train's CodebookTrain / DistribTrain.

Tolerance of the accumulators -- derived, not tuned.  The device forms gamma per item in the reference's order; it may differ from the
restatement's by up to two fp32 ulps (last-bit differences of the device's exp and log carried through one float rounding and one division),
and the fp64 contraction skips the two float product roundings of x*gamma and (gamma*x)*x: 4 * 2^-24 relative to the sum of the terms'
magnitudes.  The sum over n items is reordered in fp64: n * 2^-53 of the same.  Scores are compared within 2 fp32 ulps.
The largest ratio |dev - ref| / bound seen per case is printed (-s); DESIGN 4.8c records the largest of a run."""
import math
import os

import numpy as np
import pytest

from dsr._capi import Trainer
from tests import synth
from tests import train_np as T

pytestmark = pytest.mark.gpu
f32 = np.float32
CHUNK = 256                                             # kChunk of csrc/k_train.hip
ITEMS = [0, 1, 3, 4, 5, 63, 64, 65, CHUNK + 1]          # items per codebook


def _case(refNs, D, counts, seed, nFrames=97):
    """model + unsorted items with repeated (frame, distribution) pairs, factors of both signs and zero, scales != 1 and -- for refN >= 2 --
    one Gaussian per codebook far enough away that its exponent is below -100"""
    rng = np.random.default_rng(seed); K = len(refNs)
    scale = rng.choice(np.array([0.7, 1.0, 1.3], f32), K)
    m = T.random_model(refNs, D, seed, scale=scale, spread=1.0)
    for k in range(K):
        if refNs[k] >= 2:
            m.mean[m.off[k] + refNs[k] // 2] += f32(60.0 / math.sqrt(D) + 30.0)
    x = rng.standard_normal((nFrames, D)).astype(f32)
    dist = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(counts)]) if sum(counts) else np.zeros(0, np.int32)
    frame = rng.integers(0, nFrames, len(dist)).astype(np.int32)
    factor = rng.choice(np.array([1.0, 0.37, -0.5, -1.25, 0.0, 2.0], f32), len(dist))
    p = rng.permutation(len(dist))
    return m, x, frame[p], dist[p], factor[p]


def _reference(m, x, frame, dist, factor):
    a = T.Accu(m, track=True); info = {}
    sc = a.accumulate_items(x, frame, dist, factor, info)
    # precondition: no exponent near the -100 cutoff (a last-bit difference in the distance could flip the branch); NaN scores raise above
    e = np.array(info.get("exps", [0.0]))
    assert np.abs(e + 100.0).min() > 1e-3
    return a, sc


def _bounds(a):
    n = a.n.astype(np.float64); rel = 4 * 2.0 ** -24 + n * 2.0 ** -53
    return dict(count=rel * a.count, den=rel * a.den, sumO=rel[:, None] * a.absO, sumOsq=rel[:, None] * a.absOsq, dcount=rel * a.dcount, dden=rel * a.dden)


def _check(dev, a, what=""):
    bnd = _bounds(a); worst = 0.0
    for name in Trainer.NAMES:
        err = np.abs(dev[name] - getattr(a, name)); b = bnd[name]
        assert np.all(err <= b), (what, name, float((err - b).max()))
        nz = b > 0
        if nz.any():
            worst = max(worst, float((err[nz] / b[nz]).max()))
    return worst


def _ulps(a, b):
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _gmm(dsr, m):
    return dsr.Gmm(**m.as_kwargs())


@pytest.mark.parametrize("refN", [1, 2, 16, 17, 256])
@pytest.mark.parametrize("D", [1, 13, 39, 40, 41])
def test_accumulators_match_the_restatement(dsr, cuda, D, refN):
    import torch
    m, x, frame, dist, factor = _case([refN] * len(ITEMS), D, ITEMS, seed=1000 * D + refN)
    a, sc = _reference(m, x, frame, dist, factor)
    far = np.array([m.off[k] + refN // 2 for k in range(m.K)])
    if refN >= 2:
        assert not a.n[far].any() and a.n.sum() > 0                          # the far Gaussian's exponent is below -100 for every item
    g = _gmm(dsr, m); t = Trainer(g)
    xd = torch.from_numpy(x).to(cuda)
    sd = t.accumulate(xd, frame, dist, factor)
    dev = t.get()
    if refN >= 2:
        assert not dev["count"][far].any() and not dev["den"][far].any() and not dev["sumO"][far].any() and not dev["sumOsq"][far].any()    # exactly zero there
    worst = _check(dev, a, "D=%d refN=%d" % (D, refN))
    u = _ulps(sd, sc).max() if len(sc) else 0.0
    print("D=%d refN=%d: accumulators at %.3f of the bound, scores within %.1f ulp" % (D, refN, worst, u))
    assert u <= 2.0
    assert (dev["den"] >= 0).all() and dev["den"].sum() > 0 and dev["count"].sum() > 0
    # the same call on a fresh handle: the same bits
    t2 = Trainer(g); sd2 = t2.accumulate(xd, frame, dist, factor); dev2 = t2.get()
    assert np.array_equal(sd, sd2)
    for name in Trainer.NAMES:
        assert np.array_equal(dev[name].view(np.int64), dev2[name].view(np.int64)), name


def test_three_codebooks_of_different_size(dsr, cuda):
    import torch
    m, x, frame, dist, factor = _case([1, 17, 256, 4], 39, [70, 300, 129, 0], seed=77)
    a, sc = _reference(m, x, frame, dist, factor)
    t = Trainer(_gmm(dsr, m)); xd = torch.from_numpy(x).to(cuda)
    # in two calls: the accumulators carry over
    h = len(frame) // 3
    s1 = t.accumulate(xd, frame[:h], dist[:h], factor[:h]); s2 = t.accumulate(xd, frame[h:], dist[h:], factor[h:])
    b = T.Accu(m, track=True); b.accumulate_items(x, frame[:h], dist[:h], factor[:h]); b.accumulate_items(x, frame[h:], dist[h:], factor[h:])
    worst = _check(t.get(), b, "mixed")
    print("mixed sizes: accumulators at %.3f of the bound" % worst)
    assert _ulps(np.concatenate([s1, s2]), sc).max() <= 2.0
    t.zero(2); d = t.get()
    assert not d["dcount"].any() and not d["dden"].any() and d["count"].any()
    t.zero(1, nParts=2, part=1); d = t.get()                               # the first two codebooks only
    assert not d["count"][:18].any() and d["count"][18:].any()


@pytest.mark.parametrize("Tn", [1, 257])
def test_accumulate_path(dsr, cuda, Tn):
    import torch
    m = T.random_model([4, 2, 8], 13, seed=5, scale=[1.0, 0.8, 1.0]); rng = np.random.default_rng(Tn)
    x = rng.standard_normal((Tn, 13)).astype(f32); ids = rng.integers(0, 3, Tn)
    a = T.Accu(m, track=True); so = a.accumulate_path(x, ids, 0.75)
    t = Trainer(_gmm(dsr, m)); sd = t.accumulate_path(torch.from_numpy(x).to(cuda), ids, 0.75)
    _check(t.get(), a, "path")
    assert abs(sd - so) <= 2 * Tn * np.spacing(f32(abs(so) / Tn))           # a double sum of floats that agree within 2 ulp each


def _lattice(dsr, cuda, m, x):
    """a small decode in lattice mode over the model's own scores; the first graph seed whose lattice is a DAG with both kinds of skipped links"""
    import torch
    xd = torch.from_numpy(x).to(cuda)
    sc = dsr.Gmm(**m.as_kwargs()).score(xd, mode=0, want_argmin=False)[0]
    for seed in (6, 8, 16, 26, 36):
        arcs, fin = synth.random_wfst(300, m.K, seed=seed, eps_frac=0.35, out_frac=0.3, nWords=200)
        gd = dsr.Wfst()
        for a in arcs:
            gd.add_arc(*a)
        for s, c in fin:
            gd.add_final(s, c)
        dec = dsr.Decoder(beam=60.0, lmScale=12.0, maxActive=8192, streams=1, latticeTokens=400000); dec.set(gd)
        out = dec.decode_batch(sc[None].contiguous())
        assert out[0]["status"] == 0
        L = dec.lattice(0, eosX=7)
        try:
            L.gammaProbs(acScale=0.3, lmScale=12.0)
        except dsr.DsrError as e:
            assert e.status == 4                                             # not a DAG (an epsilon collision): try the next graph
            continue
        st = L.state(); live = (st["edgeLive"] != 0) & (st["nodeLive"][L.data["from"]] != 0)
        if (live & (L.data["in"] == 0)).any() and (live & (L.data["in"] != 0) & (st["gamma"] > 10.0)).any() and (live & (L.data["in"] != 0) & (st["gamma"] <= 10.0)).any():
            return L, st, live
    raise AssertionError("no graph gave a lattice with an epsilon link, a link with gamma > 10 and a link to accumulate")


def test_accumulate_lattice(dsr, cuda):
    import torch
    m = T.random_model([4] * 8, 13, seed=15, spread=0.5); Tn = 40
    x = np.random.default_rng(16).standard_normal((Tn, 13)).astype(f32)
    L, st, live = _lattice(dsr, cuda, m, x)
    assert (live & (L.data["in"] == 0)).any() and (live & (st["gamma"] > 10.0)).any()        # both skips are exercised
    xd = torch.from_numpy(x).to(cuda)
    for factor in (1.0, -0.6):
        frame, dist, fac, cnt = T.Accu.lattice_items(L.data, st["gamma"], live, factor, m.K, Tn)
        assert cnt > 0 and len(frame) >= cnt
        a = T.Accu(m, track=True); a.accumulate_items(x, frame, dist, fac)
        t = Trainer(_gmm(dsr, m))
        assert t.accumulate_lattice(L, xd, factor) == cnt
        d = t.get(); _check(d, a, "lattice %g" % factor)
        if factor < 0:
            assert d["den"].sum() > 0 and not d["count"].any() and d["dden"].sum() > 0 and not d["dcount"].any()
        else:
            assert d["count"].sum() > 0 and not d["den"].any()
    with pytest.raises(dsr.DsrError) as e:
        Trainer(_gmm(dsr, m)).accumulate_lattice(L, xd[:Tn - 1].contiguous(), 1.0)            # a link ends beyond the frames
    assert e.value.status == dsr.E_INDEX


def _same_params(p, m):
    for k, v in (("mean", m.mean), ("cv", m.cv), ("det", m.det), ("val", m.val), ("count", m.count)):
        assert np.array_equal(p[k].view(np.int32), v.view(np.int32)), k
    assert list(p["refN"]) == m.refN


def _trained(dsr, cuda, seed=21, minCount=5.0):
    import torch
    m = T.random_model([4, 16, 2], 13, seed=seed); rng = np.random.default_rng(seed)
    ids = rng.integers(0, 3, 700); x = np.stack([T.sample(m, int(k), 1, rng)[0] for k in ids])
    g = _gmm(dsr, m); t = Trainer(g, minCount)
    t.accumulate_path(torch.from_numpy(x).to(cuda), ids, 1.0)
    a = T.Accu(m, minCount)
    d = t.get()
    for name in Trainer.NAMES:
        setattr(a, name, d[name].copy())                                     # the restatement runs on the device-made accumulators
    return m, a, g, t, x


def test_update_chain_is_bit_identical_and_every_scoring_mode_follows(dsr, cuda):
    import torch
    m, a, g, t, x = _trained(dsr, cuda)
    a.update(3); t.update(3); _same_params(g.params(), m)
    assert a.floor_variances() == t.floor_variances()                        # (variances below the floor: test_floor_fix_invert_bit_identical)
    a.fix_gconsts(); t.fix_gconsts(); _same_params(g.params(), m)
    a.invert_variances(); t.invert_variances()
    p = g.params(); _same_params(p, m)
    assert (m.count[:4] > 5.0).any() and not np.array_equal(m.mean, T.random_model([4, 16, 2], 13, seed=21).mean)
    # scoring with the trained model: every mode equals a model created from the same parameters
    fresh = dsr.Gmm(refN=p["refN"], mean=p["mean"], ivar=p["cv"], det=p["det"], val=p["val"])
    xd = torch.from_numpy(np.random.default_rng(3).standard_normal((256, 13)).astype(f32)).to(cuda)
    s0, a0 = g.score(xd, mode=0); f0, fa0 = fresh.score(xd, mode=0)
    assert torch.equal(s0, f0) and torch.equal(a0, fa0)
    assert torch.equal(g.score(xd, mode=1)[0], fresh.score(xd, mode=1)[0])
    s2, a2m = g.score(xd, mode=2)
    assert torch.equal(a2m, a0)                                              # the MFMA operand image was rebuilt
    assert torch.allclose(s2, s0, rtol=1e-3, atol=1e-3)
    old = dsr.Gmm(**T.random_model([4, 16, 2], 13, seed=21).as_kwargs()).score(xd, mode=0)[0]
    assert not torch.equal(old, s0)                                          # and the parameters did change


def test_floor_fix_invert_bit_identical(dsr, cuda):
    """variances below the floor, through both sides: the device handle's model starts from parameters that need flooring"""
    m = T.random_model([3, 5], 7, seed=4)
    T.Accu(m).invert_variances()                                             # cv = variances, as after update
    m.cv[0, 0] = 1e-6; m.cv[4, 3] = 5e-5
    g = _gmm(dsr, m); t = Trainer(g); a = T.Accu(m)
    assert t.floor_variances() == a.floor_variances() == (8 * 7, 2)
    t.fix_gconsts(); a.fix_gconsts(); t.invert_variances(); a.invert_variances()
    _same_params(g.params(), m)
    # parts: the second codebook only
    t.invert_variances(nParts=2, part=2); a.invert_variances(nParts=2, part=2)
    _same_params(g.params(), m)
    m.cv[1, 1] = -1.0; g2 = _gmm(dsr, m)
    with pytest.raises(dsr.DsrError) as e:
        Trainer(g2).fix_gconsts()
    assert e.value.status == dsr.E_CONSISTENCY                               # "Determinant is NaN"


@pytest.mark.parametrize("merialdo", [False, True])
def test_mmi_update_bit_identical(dsr, cuda, merialdo):
    import torch
    m, a, g, t, x = _trained(dsr, cuda, seed=23)
    rng = np.random.default_rng(5); ids = rng.integers(0, 3, 300)
    t.accumulate_path(torch.from_numpy(x[:300].copy()).to(cuda), ids, -0.5)
    d = t.get()
    for name in Trainer.NAMES:
        setattr(a, name, d[name].copy())
    assert d["den"].sum() > 0
    a.update_mmi(3, E=2.0, merialdo=merialdo); t.update_mmi(3, E=2.0, merialdo=merialdo)
    _same_params(g.params(), m)
    t.set(dcount=np.where(np.arange(22) == 3, -np.inf, d["dcount"]))
    with pytest.raises(dsr.DsrError) as e:
        t.update_mmi(2, merialdo=merialdo)
    assert e.value.status == dsr.E_CONSISTENCY
    _same_params(g.params(), m)                                              # the refused update left the model alone


def test_split_then_accumulate(dsr, cuda):
    import torch
    m, a, g, t, x = _trained(dsr, cuda, seed=29)
    a.update(3); a.floor_variances(); a.fix_gconsts(); a.invert_variances()
    t.update(3); t.floor_variances(); t.fix_gconsts(); t.invert_variances()
    before = t.get()
    r = t.split(0, 0.0, 0.2); assert r == a.split(0, 0.0, 0.2)
    assert t.G == 23 and m.refN == [5, 16, 2]
    _same_params(g.params(), m)
    d = t.get()
    assert d["sumO"].shape == (23, 13) and not d["count"][:5].any() and np.array_equal(d["count"][5:], before["count"][4:]) and np.array_equal(d["sumO"][5:], before["sumO"][4:])
    with pytest.raises(dsr.DsrError) as e:
        t.split(2, 1e9, 0.2)
    assert e.value.status == dsr.E_PARAMETER
    # accumulation follows the new shape: the codebooks behind the split one moved up by one row
    t.zero(); rng = np.random.default_rng(2)
    frame = rng.integers(0, 200, 400).astype(np.int32); dist = rng.integers(0, 3, 400).astype(np.int32); factor = rng.choice(np.array([1.0, -1.0], f32), 400)
    b = T.Accu(m, track=True); so = b.accumulate_items(x, frame, dist, factor)
    sd = t.accumulate(torch.from_numpy(x).to(cuda), frame, dist, factor)
    _check(t.get(), b, "after split"); assert _ulps(sd, so).max() <= 2.0
    big = T.random_model([256, 2], 3, seed=1)
    with pytest.raises(dsr.DsrError) as e:
        Trainer(_gmm(dsr, big)).split(0)
    assert e.value.status == dsr.E_DIMENSION


def test_accumulator_files(dsr, cuda, tmp_path):
    import torch
    m, a, g, t, x = _trained(dsr, cuda, seed=33)
    t.zero(3, nParts=3, part=2)                                              # the middle codebook is empty: skipped in the files
    d = t.get()
    for name in Trainer.NAMES:
        setattr(a, name, d[name].copy())
    cf, df = str(tmp_path / "cb.accu"), str(tmp_path / "ds.accu")
    t.save_codebook_accus(cf, 3.5, 700); t.save_distrib_accus(df)
    assert open(cf, "rb").read() == a.save_codebook_accus(3.5, 700) and open(df, "rb").read() == a.save_distrib_accus()      # the restatement's writer, byte for byte
    t2 = Trainer(g)
    assert t2.load_codebook_accus(cf) == (3.5, 700)
    t2.load_distrib_accus(df)
    b = T.Accu(m); b.load_codebook_accus(open(cf, "rb").read()); b.load_distrib_accus(open(df, "rb").read())
    d2 = t2.get()
    for name in Trainer.NAMES:
        assert np.array_equal(d2[name], d[name].astype(f32).astype(np.float64)) and np.array_equal(d2[name], getattr(b, name)), name
    t2.load_codebook_accus(cf, factor=-0.25); b.load_codebook_accus(open(cf, "rb").read(), factor=-0.25)
    for name in Trainer.NAMES:
        assert np.array_equal(t2.get()[name], getattr(b, name)), name
    t2.add(t, 2.0); b.add(a, 2.0)                                            # Accu::add: scaled codebook sums, unscaled distribution counts
    for name in Trainer.NAMES:
        assert np.array_equal(t2.get()[name], getattr(b, name)), name
    co = str(tmp_path / "cb.counts"); t.save_codebook_accus(co, 0.0, 0, countsOnly=True)
    assert open(co, "rb").read() == a.save_codebook_accus(0.0, 0, countsOnly=True)
    # a handle of another shape refuses the file and keeps its accumulators
    other = T.random_model([5, 16, 2], 13, seed=33)
    t3 = Trainer(_gmm(dsr, other)); t3.set(count=np.arange(23.0))
    with pytest.raises(dsr.DsrError) as e:
        t3.load_codebook_accus(cf)
    assert e.value.status == dsr.E_DIMENSION and np.array_equal(t3.get()["count"], np.arange(23.0))
    with pytest.raises(dsr.DsrError) as e:
        t3.load_distrib_accus(df)
    assert e.value.status == dsr.E_DIMENSION
    with pytest.raises(dsr.DsrError) as e:
        t3.load_codebook_accus(str(tmp_path / "missing"))
    assert e.value.status == dsr.E_IO


def test_error_paths_leave_the_accumulators_alone(dsr, cuda):
    import torch
    m, a, g, t, x = _trained(dsr, cuda, seed=37)
    before = t.get(); xd = torch.from_numpy(x).to(cuda)
    for frame, dist in (([0, 700], [0, 0]), ([0, -1], [0, 0]), ([0, 1], [0, 3]), ([0, 1], [-1, 0])):
        with pytest.raises(dsr.DsrError) as e:
            t.accumulate(xd, frame, dist, [1.0, 1.0])
        assert e.value.status == dsr.E_INDEX
    xn = x.copy(); xn[5, 3] = np.nan
    for k in (0, 1):                                                         # a 4-Gaussian and a 16-Gaussian codebook; then the refN == 1 branch
        with pytest.raises(dsr.DsrError) as e:
            t.accumulate(torch.from_numpy(xn).to(cuda), [1, 5, 9], [k, k, 2], [1.0, 1.0, 1.0])
        assert e.value.status == 12                                          # DSR_E_NUMERIC
    g1 = _gmm(dsr, T.random_model([1, 2], 13, seed=2)); t1 = Trainer(g1)
    with pytest.raises(dsr.DsrError) as e:
        t1.accumulate(torch.from_numpy(xn).to(cuda), [5], [0], [1.0])
    assert e.value.status == 12 and not t1.get()["count"].any()
    after = t.get()
    for name in Trainer.NAMES:
        assert np.array_equal(before[name].view(np.int64), after[name].view(np.int64)), name
    assert t.accumulate(xd, [], [], []).size == 0                            # an empty batch is not an error
