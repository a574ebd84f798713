"""Feature-space adaptation on the device (include/dsr.h section 11, csrc/k_fsa.hip, csrc/fsa.cpp) against tests/fsa_np.py, the numpy
restatement of asr/train/fsa.cc ("fsa").

Tolerances -- derived, not tuned.
  Statistics.  The operands c = gamma iv (gamma float(mu iv)) and xi_j xi_k are exact in fp64.  The reference rounds c xi_j and then (c xi_j) xi_k:
  two roundings a term of G_i, one a term of z_i, 2^-53 each relative to the term's magnitude; both sums over the n items of an accumulator are
  reordered in fp64: up to n 2^-53 sum |terms| each.  G within (2 n + 2) 2^-53 sum |terms|, z within (2 n + 1) 2^-53 sum |terms|.
  Estimate.  Against the restatement on the device-made statistics.  Yardstick: the larger of the restatement's own difference between its SVD
  variant and its numpy.linalg.inv / det variant, and iterN (D + 1) 2^-53 max_i cond(G_i) max |W|.  The device may differ by 8 x that (the
  margin of the MLLR solve test, for the same reason: two legitimate orders of the same fp64 arithmetic).
The largest ratios seen are printed (-s); DESIGN 4.8e records those of a run."""
import numpy as np
import pytest

from dsr._capi import DsrError, Fsa
from dsr.asr.train import FeatureSpaceAdaptationFeaturePtr
from tests import fsa_np as F

pytestmark = pytest.mark.gpu
f32 = np.float32
DIMS = [1, 3, 15, 16, 39, 40]
ITEMS = [1, 3, 63, 64, 65, 257]                         # items per accumulator: around the MFMA k-step (4) and the chunk (64), several chunks
REFN = [1, 4, 17]
GAMMAS = np.array([1.0, 0.37, -0.5, -1.25, 0.0, 2.0], f32)


def _gmm(dsr, m):
    return dsr.Gmm(**m)


def _np_state(m, nAccu=1, nTran=1, track=False):
    return F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"], nAccu, nTran, track)


def _items(rng, K, nFrames, counts):
    """unsorted items of len(counts) accumulators, interleaved, with repeated (frame, distribution) pairs and gammas of both signs and zero"""
    accu = np.concatenate([np.full(c, a, np.int32) for a, c in enumerate(counts)]); n = len(accu)
    frame = rng.integers(0, nFrames, n).astype(np.int32); frame[n // 2:] = frame[:n - n // 2]       # repeats
    dist = rng.integers(0, K, n).astype(np.int32); gamma = rng.choice(GAMMAS, n)
    p = rng.permutation(n)
    return frame[p], dist[p], gamma[p], accu[p]


def _check_stats(dev, ref, a):
    """-> (ratio of G, ratio of z) to the derived bounds"""
    n = float(ref.items[a]); low = np.tril(np.ones(ref.G.shape[2:], bool))[None]
    bG = (2 * n + 2) * 2.0 ** -53 * ref.Gabs[a]; bz = (2 * n + 1) * 2.0 ** -53 * ref.zabs[a]
    eG = np.abs(dev["G"] - ref.G[a]); ez = np.abs(dev["z"] - ref.z[a])
    assert not dev["G"][~np.broadcast_to(low, dev["G"].shape)].any()          # only the lower triangle is written
    assert np.all(eG <= bG), float((eG - bG).max())
    assert np.all(ez <= bz), float((ez - bz).max())
    rG = float((eG[bG > 0] / bG[bG > 0]).max()) if (bG > 0).any() else 0.0
    rz = float((ez[bz > 0] / bz[bz > 0]).max()) if (bz > 0).any() else 0.0
    return rG, rz


@pytest.mark.parametrize("ni", range(len(ITEMS)))
@pytest.mark.parametrize("di", range(len(DIMS)))
def test_items_and_statistics_match_the_restatement(dsr, cuda, di, ni):
    import torch
    D = DIMS[di]; R = REFN[(di + ni) % len(REFN)]; K = 5; nFrames = 41
    counts = [ITEMS[ni], ITEMS[(ni + 1 + di) % len(ITEMS)]]
    rng = np.random.default_rng(100 * di + ni)
    m = F.synth_model(K, R, D, seed=7 + 100 * di + ni)
    xScore = (rng.standard_normal((nFrames, D)) * 2.0).astype(f32); xSrc = (xScore * f32(0.9) + rng.standard_normal((nFrames, D)).astype(f32) * f32(0.3)).astype(f32)
    frame, dist, gamma, accu = _items(rng, K, nFrames, counts)
    g = _gmm(dsr, m); h = Fsa(g, nAccu=2, nTran=1)
    ref = _np_state(m, 2, 1, track=True)
    for k in range(K):
        if k != 2:                                                           # distribution 2 stays switched off
            h.add(k); ref.add(k)
    xs, xr = torch.from_numpy(xScore).to(cuda), torch.from_numpy(xSrc).to(cuda)
    accepted, near = h.accumulate(xs, frame, dist, gamma, accu, xSrc=xr, want_nearest=True)
    chosen = ref.accumulate_items(xScore, xSrc, frame, dist, gamma, accu)
    # item level: the nearest Gaussian is scoring mode 0's argmin
    am = g.score(xs, mode=0, want_argmin=True)[1].cpu().numpy()
    want = np.where(dist == 2, -1, am[frame, dist].astype(np.int32))
    assert np.array_equal(near, want)
    assert np.array_equal(near, np.array([-1 if c is None else c - ref.off[d] for c, d in zip(chosen, dist)], np.int32))
    worst = [0.0, 0.0]
    for a in range(2):
        dev = h.get_accu(a)
        assert accepted[a] == ref.items[a] == int(((accu == a) & (dist != 2)).sum())
        assert dev["count"] == ref.count[a] and dev["beta"].view(np.int32) == ref.beta[a].view(np.int32)       # bit for bit
        rG, rz = _check_stats(dev, ref, a); worst = [max(worst[0], rG), max(worst[1], rz)]
    print("D=%d items=%s refN=%d: G at %.3f, z at %.3f of the bound" % (D, counts, R, worst[0], worst[1]))
    # the same call on a fresh handle: the same bits
    h2 = Fsa(g, nAccu=2, nTran=1); h2.add_all(); h.zero(0); h.zero(1); h.add(2)
    h.accumulate(xs, frame, dist, gamma, accu, xSrc=xr); h2.accumulate(xs, frame, dist, gamma, accu, xSrc=xr)
    for a in range(2):
        d1, d2 = h.get_accu(a), h2.get_accu(a)
        assert np.array_equal(d1["G"].view(np.int64), d2["G"].view(np.int64)) and np.array_equal(d1["z"].view(np.int64), d2["z"].view(np.int64))


def _speakers(dsr, cuda, D, nSpk, T, seed, K=6, R=4):
    """device-made statistics of nSpk speakers (accumulator s) + the restatement carrying the same numbers"""
    import torch
    m = F.synth_model(K, R, D, seed); g = _gmm(dsr, m); h = Fsa(g, nAccu=nSpk, nTran=nSpk); h.add_all()
    ref = _np_state(m, nSpk, nSpk); ref.addAll(); truth = []
    for s in range(nSpk):
        x, dist, W0 = F.synth_speaker(m, T[s] if isinstance(T, (list, tuple)) else T, seed=seed + 10 * s + 1); truth.append(W0)
        xd = torch.from_numpy(x).to(cuda)
        h.accumulate(xd, np.arange(len(dist)), dist, np.ones(len(dist), f32), np.full(len(dist), s))
        dev = h.get_accu(s)
        ref.count[s], ref.beta[s], ref.z[s], ref.G[s] = dev["count"], dev["beta"], dev["z"], dev["G"]
    return m, g, h, ref, truth


@pytest.mark.parametrize("iterN", [1, 10])
@pytest.mark.parametrize("D", DIMS)
def test_estimate_matches_the_restatement(dsr, cuda, D, iterN, tmp_path):
    """four pairs in one call on the device-made statistics: two from the identity, two from a transform loaded from a file"""
    T = max(50 * D, 60)
    m, g, h, ref, truth = _speakers(dsr, cuda, D, 4, T, seed=300 + D)
    rng = np.random.default_rng(D)
    for t in (2, 3):
        W = np.eye(D, D + 1, 1) + 0.05 * rng.standard_normal((D, D + 1)); h.set_transform(W, t)
        fn = str(tmp_path / ("w%d.saw" % t)); h.save(fn, t); h.clear(t); h.load(fn, t)
        assert np.array_equal(h.transform(t), W.astype(f32).astype(np.float64))
    start = [h.transform(t) for t in range(4)]
    h.estimate(iterN, [0, 1, 2, 3], [0, 1, 2, 3])
    worst = 0.0
    for t in range(4):
        assert h.transform_status(t) == 0
        Wd = h.transform(t)
        Ws = ref.estimate(iterN, t, t, variant="svd", W0=start[t]); Wi = ref.estimate(iterN, t, t, variant="inv", W0=start[t])
        Gs = ref.sym(t); kappa = max(np.linalg.cond(Gs[i]) for i in range(D))
        yard = max(float(np.abs(Ws - Wi).max()), iterN * (D + 1) * 2.0 ** -53 * kappa * float(np.abs(Ws).max()))
        err = float(np.abs(Wd - Ws).max()); worst = max(worst, err / yard)
        assert err <= 8 * yard, (t, err, yard)
        Qd, Qs = ref.aux(Wd, t), ref.aux(Ws, t)
        assert Qd >= Qs - 8 * yard * abs(Qs), (t, Qd, Qs)
        assert ref.aux(Wd, t) > ref.aux(start[t], t)
    print("D=%d iterN=%d: W at %.3f of the yardstick (8 allowed)" % (D, iterN, worst))


@pytest.mark.parametrize("D", [3, 13, 39])
def test_deficient_pair_is_refused(dsr, cuda, D):
    """a pair with (D + 1) / 2 frames is flagged and keeps its transform; the other pairs of the call are done"""
    m, g, h, ref, truth = _speakers(dsr, cuda, D, 3, [50 * D, (D + 1) // 2, 50 * D], seed=500 + D)
    W1 = np.eye(D, D + 1, 1) + 0.01 * np.random.default_rng(D).standard_normal((D, D + 1)); h.set_transform(W1, 1)
    with pytest.raises(DsrError) as e:
        h.estimate(2, [0, 1, 2], [0, 1, 2])
    assert e.value.status == dsr.E_CONSISTENCY
    assert h.transform_status(1) == dsr.E_CONSISTENCY and np.array_equal(h.transform(1), W1)
    for t in (0, 2):
        assert h.transform_status(t) == 0
        Ws = ref.estimate(2, t, t, W0=np.eye(D, D + 1, 1))
        assert np.abs(h.transform(t) - Ws).max() <= 1e-6 * np.abs(Ws).max() and not np.array_equal(h.transform(t), np.eye(D, D + 1, 1))
    h.estimate(1, 0, 1)                                                      # good statistics: the flag is cleared
    assert h.transform_status(1) == 0


@pytest.mark.parametrize("D", DIMS)
def test_apply_is_bit_exact(dsr, cuda, D):
    import torch
    N = 1000 if D < 39 else 300                                              # not a multiple of the block size
    rng = np.random.default_rng(40 + D); m = F.synth_model(2, 2, D, seed=D)
    h = Fsa(_gmm(dsr, m), nAccu=1, nTran=3); ref = _np_state(m, 1, 3)
    for t in range(3):
        W = np.eye(D, D + 1, 1) + 0.3 * rng.standard_normal((D, D + 1)); h.set_transform(W, t); ref.W[t] = W
    x = (rng.standard_normal((N, D)) * 3.0).astype(f32); xd = torch.from_numpy(x).to(cuda)
    tr = rng.integers(0, 3, N).astype(np.int32); trd = torch.from_numpy(tr).to(cuda)
    for shift in (1.0, -1.0, 0.5):
        out = h.apply(xd, trd, shift).cpu().numpy()
        assert np.array_equal(out.view(np.int32), ref.apply(x, tr, shift).view(np.int32)), shift
        out0 = h.apply(xd, None, shift).cpu().numpy()
        assert np.array_equal(out0.view(np.int32), ref.apply(x, 0, shift).view(np.int32)), shift
    bad = tr.copy(); bad[5] = 3; bad[7] = -1
    out = h.apply(xd, torch.from_numpy(bad).to(cuda), 1.0).cpu().numpy()
    assert np.isnan(out[5]).all() and np.isnan(out[7]).all() and not np.isnan(out[6]).any()


class _Frames(object):
    def __init__(self, x):
        self.x = x

    def size(self):
        return self.x.shape[1]

    def reset(self):
        pass

    def __iter__(self):
        return iter(self.x)


def test_stream_operator(dsr, cuda):
    import torch
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    D, N = 13, 70; rng = np.random.default_rng(3); m = F.synth_model(3, 2, D, seed=9); g = _gmm(dsr, m)
    x = rng.standard_normal((N, D)).astype(f32)
    src = PyVectorFloatFeatureStreamPtr(_Frames(x), "Src"); fsa = FeatureSpaceAdaptationFeaturePtr(src, 2, 2, "FSA")
    assert fsa.size() == D and fsa.name() == "FSA"
    with pytest.raises(DsrError) as e:
        fsa.next()
    assert e.value.status == dsr.E_CONSISTENCY                               # next() before distribSet
    with pytest.raises(DsrError) as e:
        fsa.addAll()
    assert e.value.status == dsr.E_CONSISTENCY

    class _Dss(object):
        gmm = g
    fsa.distribSet(_Dss()); h = fsa.handle()
    assert h.nAccu == 2 and h.nTran == 2 and fsa.topN() == 1 and fsa.shift() == 1.0
    W = np.eye(D, D + 1, 1) + 0.2 * rng.standard_normal((D, D + 1)); h.set_transform(W, 0)
    for shift in (1.0, -1.0):
        fsa.setShift(shift); fsa.reset()
        batch = h.apply(torch.from_numpy(x).to(cuda), None, shift).cpu().numpy()
        rows = np.stack([np.array(fsa.next(t)) for t in range(N)])
        assert np.array_equal(rows.view(np.int32), batch.view(np.int32))
        with pytest.raises(StopIteration):
            fsa.next()
    fsa.reset(); fsa.next(0)
    with pytest.raises(DsrError) as e:
        fsa.next(2)
    assert e.value.status == dsr.E_INDEX                                      # out of order
    with pytest.raises(DsrError) as e:
        fsa.setTopN(3)                                                       # beyond refN = 2 of the largest codebook
    assert e.value.status == dsr.E_INDEX
    fsa.setTopN(2); assert fsa.topN() == 2


def test_accumulate_path_and_lattice_quirks(dsr, cuda, capsys):
    """a name the set does not know does not advance the frame; a lattice link gives every second frame"""
    import torch
    from tests import train_np as T
    from tests.test_gpu_train import _lattice
    tm = T.random_model([4] * 8, 13, seed=15, spread=0.5); Tn = 40
    x = np.random.default_rng(16).standard_normal((Tn, 13)).astype(f32); xd = torch.from_numpy(x).to(cuda)
    m = tm.as_kwargs(); g = dsr.Gmm(**m)
    h = Fsa(g, 2, 1); h.add_all(); ref = _np_state(m, 2, 1, track=True); ref.addAll()
    ids = [3, -1, 0, 7, -1, -1, 2, 2, 5]
    assert h.accumulate_path(xd, ids, 1, 0.75) == 6 == ref.accumulate(x, x, [None if i < 0 else i for i in ids], 1, 0.75)
    dev = h.get_accu(1)
    assert dev["count"] == 6.0 == ref.count[1] and dev["beta"] == ref.beta[1]
    _check_stats(dev, ref, 1)
    L, st, live = _lattice(dsr, cuda, tm, x)
    links = [(int(L.data["in"][e]), float(st["gamma"][e]), int(L.data["start"][e]), int(L.data["end"][e])) for e in range(len(live)) if live[e]]
    for factor in (1.0, -0.6):
        h.zero(0); ref.zeroAccu(0)
        cnt = ref.accumulate_lattice(x, x, links, 0, factor)
        assert cnt > 0 and h.accumulate_lattice(L, xd, 0, factor) == cnt
        dev = h.get_accu(0)
        assert dev["count"] == ref.count[0] and dev["beta"].view(np.int32) == ref.beta[0].view(np.int32)
        assert ref.count[0] == sum((e - s) // 2 + 1 for i, gm, s, e in links if i != 0 and gm <= 10.0)
        _check_stats(dev, ref, 0)
    with pytest.raises(DsrError) as e:
        h.accumulate_lattice(L, xd[:Tn - 1].contiguous(), 0, 1.0)
    assert e.value.status == dsr.E_INDEX


def test_files_accumulator_operations_and_error_codes(dsr, cuda, tmp_path):
    import torch
    D = 5; m, g, h, ref, truth = _speakers(dsr, cuda, D, 2, 40, seed=77)
    sas = str(tmp_path / "a.sas"); saw = str(tmp_path / "w.saw")
    # files written by the product equal the restatement's writer on the device's own arrays, byte for byte
    h.save_accu(sas, 1); assert open(sas, "rb").read() == ref.accu_bytes(1)
    h.estimate(3, 1, 1); ref.W[1] = h.transform(1)
    h.save(saw, 1); assert open(saw, "rb").read() == ref.tran_bytes(1)
    # loadAccu adds with its factor; the upper triangle the file brought is written again
    data = bytearray(ref.accu_bytes(1)); up = 7 + 4 * (2 + D * (D + 1) + 1); data[up:up + 4] = np.array([2.5], ">f4").tobytes()      # G_0[0][1]
    open(sas, "wb").write(bytes(data))
    h.load_accu(sas, 0, 0.5); ref.load_accu_bytes(bytes(data), 0, 0.5)
    dev = h.get_accu(0)
    assert dev["count"] == ref.count[0] and dev["beta"] == ref.beta[0] and np.array_equal(dev["z"], ref.z[0]) and np.array_equal(dev["G"], ref.G[0])
    assert dev["G"][0, 0, 1] == 1.25
    h.save_accu(sas, 0); assert open(sas, "rb").read() == ref.accu_bytes(0)
    # the estimate reads the lower triangle only (_makeSymmetric)
    h.estimate(1, 0, 0); Wa = h.transform(0); dev["G"][0, 0, 1] = 0.0; ref.G[0][0, 0, 1] = 0.0; h.set_accu(0, G=dev["G"]); h.clear(0); h.estimate(1, 0, 0)
    assert np.array_equal(Wa, h.transform(0))
    # scale, add, zero as written
    h.scale(0.3, 0); ref.scaleAccu(0.3, 0); h.add_accu(0, 1, -0.7); ref.addAccu(0, 1, -0.7)
    dev = h.get_accu(0)
    assert dev["count"] == ref.count[0] and dev["beta"] == ref.beta[0] and np.array_equal(dev["z"], ref.z[0]) and np.array_equal(dev["G"], ref.G[0])
    h.zero(0); dev = h.get_accu(0)
    assert dev["count"] == 0 and dev["beta"] == 0 and not dev["z"].any() and not dev["G"].any() and h.count(0) == 0
    # SAW round trip, clear, compareTransform's column range
    h.load(saw, 0); assert np.array_equal(h.transform(0), h.transform(1).astype(f32).astype(np.float64))
    ref.W[0] = h.transform(0)
    assert h.compare(0, 1) == ref.compareTransform(0, 1)
    W = h.transform(0); W[:, D] += 1.0; h.set_transform(W, 0)                # the last column does not count
    assert h.compare(0, 1) == ref.compareTransform(0, 1)
    h.clear(0); assert np.array_equal(h.transform(0), np.eye(D, D + 1, 1))
    # error codes
    def status(fn, *a):
        with pytest.raises(DsrError) as e:
            fn(*a)
        return e.value.status
    assert status(h.zero, 2) == dsr.E_INDEX and status(h.scale, 1.0, -1) == dsr.E_INDEX and status(h.save_accu, sas, 2) == dsr.E_INDEX
    assert status(h.load_accu, sas, 5) == dsr.E_INDEX and status(h.add_accu, 0, 2) == dsr.E_INDEX and status(h.get_accu, 2) == dsr.E_INDEX
    assert status(h.clear, 2) == dsr.E_INDEX and status(h.compare, 0, 2) == dsr.E_INDEX and status(h.save, saw, 2) == dsr.E_INDEX
    assert status(h.load, saw, -1) == dsr.E_INDEX and status(h.estimate, 1, 2, 0) == dsr.E_INDEX and status(h.estimate, 1, 0, 2) == dsr.E_INDEX
    assert status(h.add, 99) == dsr.E_INDEX and status(h.set_top_n, 5) == dsr.E_INDEX
    assert status(h.estimate, 1, [0, 1], [1, 1]) == dsr.E_PARAMETER           # the same transformation twice
    assert status(h.load_accu, saw, 0) == dsr.E_CONSISTENCY                   # no magic SAS
    assert status(h.load, sas, 0) == dsr.E_IO                                 # no magic SAW
    other = Fsa(_gmm(dsr, F.synth_model(2, 2, D + 1, seed=1)), 1, 1)
    assert status(other.load_accu, sas, 0) == dsr.E_DIMENSION and status(other.load, saw, 0) == dsr.E_DIMENSION
    assert status(h.load, str(tmp_path / "missing"), 0) == dsr.E_IO
    xd = torch.zeros((3, D), device=cuda)
    assert status(h.accumulate, xd, [3], [0], [1.0], [0]) == dsr.E_INDEX and status(h.accumulate, xd, [0], [0], [1.0], [2]) == dsr.E_INDEX


def test_two_passes(dsr, cuda, tmp_path, capsys):
    """decode, accumulate(bestPath()), estimate, decode again through dsr_decoder_decode_stream on the adapted stream"""
    import torch
    from dsr.btk.feature import FeatureSetPtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    from dsr.asr.dictionary import LexiconPtr
    from dsr.asr.gaussian import CodebookSetBasicPtr, DistribSetBasicPtr
    from dsr.asr.decoder import WFSTFlyWeightPtr, DecoderFlyWeightPtr
    from tests import synth
    K, R, D, T = 24, 4, 8, 400
    m = F.synth_model(K, R, D, seed=5); m["val"][:] = f32(np.log(R))          # uniform weights: the score is 0.5 min_g dist_g + a constant
    x, _, W0 = F.synth_speaker(m, T, seed=6)
    cbf, dsf = str(tmp_path / "cb.bin"), str(tmp_path / "ds.bin"); dsr.Gmm(**m).save(cbf, dsf)
    open(tmp_path / "cb.desc", "w").write("".join("%-25s%-20s%-10d%-3d%-10s\n" % ("cb%d" % k, "FSA", R, D, "DIAGONAL") for k in range(K)))
    open(tmp_path / "ds.desc", "w").write("".join("%-25s%-25s\n" % ("ds%d" % k, "cb%d" % k) for k in range(K)))
    inlex = ["eps"] + ["ds%d" % k for k in range(K)] + ["SIL-m"]              # the silence symbol is on no arc: every name of the path is known
    outlex = ["eps", "</s>"] + ["w%d" % i for i in range(50)]
    open(tmp_path / "in.lex", "w").write("\n".join(inlex) + "\n"); open(tmp_path / "out.lex", "w").write("\n".join(outlex) + "\n")
    arcs, fin = synth.random_wfst(400, K, seed=4, nWords=51, out_frac=0.2)
    with open(tmp_path / "g.fsm", "w") as f:
        for a in arcs:
            f.write("%d %d %d %d %.9g\n" % a)
        for s, c in fin:
            f.write("%d %.9g\n" % (s, c))
    src = PyVectorFloatFeatureStreamPtr(_Frames(x), "Src"); fsa = FeatureSpaceAdaptationFeaturePtr(src, 1, 1, "FSA")
    fs = FeatureSetPtr(); fs.add(fsa)
    cbs = CodebookSetBasicPtr(str(tmp_path / "cb.desc"), fs, cbf); dss = DistribSetBasicPtr(cbs, str(tmp_path / "ds.desc"), dsf)
    fsa.distribSet(dss); fsa.addAll()
    wfst = WFSTFlyWeightPtr(LexiconPtr("state"), LexiconPtr("in", str(tmp_path / "in.lex")), LexiconPtr("out", str(tmp_path / "out.lex")))
    wfst.read(str(tmp_path / "g.fsm"), binary=False)
    d = DecoderFlyWeightPtr(dss, beam=80.0, lmScale=12.0, silPenalty=0.5); d.set(wfst)
    d.decode(); path = list(d.bestPath())
    assert len(path) == T
    first = np.stack([np.array(v) for v in fsa])
    assert np.array_equal(first, x)                                          # the identity: float(0 + 1 x_d + 0 ...) = x_d
    ids = np.array([int(n[2:]) for n in path])
    assert fsa.accumulate(path) == T and "Accumulated %d frames." % T in capsys.readouterr().out
    assert fsa.count() == T
    fsa.estimate(10)
    h = fsa.handle(); W = h.transform(0)
    d.decode()                                                               # resets the stream: the new transform shows
    second = np.stack([np.array(v) for v in fsa])
    xd = torch.from_numpy(x).to(cuda)
    assert np.array_equal(second.view(np.int32), h.apply(xd).cpu().numpy().view(np.int32))
    # the first pass's path under the adapted frames, plus beta log|det A|, is better than before (costs are negative log-likelihoods)
    sc1 = dss.gmm.score(xd, mode=0, want_argmin=False)[0].cpu().numpy().astype(np.float64)
    sc2 = dss.gmm.score(torch.from_numpy(second).to(cuda), mode=0, want_argmin=False)[0].cpu().numpy().astype(np.float64)
    c1 = sc1[np.arange(T), ids].sum(); c2 = sc2[np.arange(T), ids].sum() - T * np.linalg.slogdet(W[:, 1:])[1]
    print("two passes: cost of the first pass's path %.2f -> %.2f" % (c1, c2))
    assert c2 < c1
