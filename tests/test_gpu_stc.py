"""STC and LDA estimation on the device (include/dsr.h section 12, csrc/k_stc.hip, csrc/stc.cpp) against tests/stc_np.py, the numpy
restatement of asr/train/estimateAdapt.cc:2203-3036 ("eA") and asr/adapt/transform.cc:1788-1984.

Tolerances -- derived, not tuned.  u = 2^-53.
  sumOsq, within, between, mixture.  The device's operands (float(iv c) and o_i o_j; c o_i and o_j) are exact in fp64.  The reference rounds the
  first product and then the second: two roundings a term, the device one, u each relative to the term's magnitude; both sums over the n items
  of an estimator are reordered in fp64: up to n u sum |terms| each.  Within (2 n + 2) u sum |terms|.
  regSq.  The reference forms P = sum_col (float(c / iv_col) a_i) a_j per item -- two roundings a term and D - 1 additions -- and adds iv_d P:
  one more rounding and the n additions of the items: (n + D + 2) u T with T the sum of the magnitudes of all terms iv_d w a_i a_j.  The device
  sums R[d][col] = sum_n iv_d w, exactly formed products, over the n items in chunks of 64 (n u, and ceil(n / 64) u for the chunks' sums),
  rounds a_i a_j and its product with R (2 u), sums D columns (D u) and adds to the accumulator (u): (n + ceil(n / 64) + D + 3) u T, less
  the first addition onto zero.  Together (2 n + 2 D + 4 + ceil(n / 64)) u T.
  STC estimate.  Against the restatement on the device-made statistics.  Yardstick: the larger of the restatement's own difference between its
  LU variant and its numpy.linalg.inv variant, and 10 D u max_d cond(G_d) max |A|.  The device may differ by 8 x that (the margin of
  test_gpu_fsa.py and the MLLR solve test: two legitimate orders of one fp64 computation).  With cascade (a mode beyond ML and MMI) the result
  is the product B A0 of the update B and the matrix A0 it started from: an error dB of the update shows as dB A0, at most max |dB| times the
  largest column sum of |A0|, so the yardstick is multiplied by that (and by no less than 1).
  Auxiliary function.  "Not lower than the restatement's" is asked of two numbers that are themselves rounded: Q is a sum of about D^3 products
  evaluated in fp64, and a matrix within 8 yardsticks of the restatement's moves Q, which is stationary there in every row, by no more than
  that relative amount.  Q(device) >= Q(restatement) - 8 yard |Q| is asserted; with cascade on the updates B = A A0^-1 (A0^-1 from numpy).
  _stcInv.  W(2) reads the columns of the inverse that set_transform formed.  That inverse is held against numpy.linalg.inv within
  20 D u cond(A) max |A^-1| (two inversions of order D, each with a forward error of about 10 D u cond(A)); the restatement then takes the
  library's inverse, so that the regSq bound compares sums of the same terms.
  LDA estimate.  A backward-stable eigen-decomposition returns V diag(l) V^T = W + dW with |dW| <= c D u |W|; under L = U^T diag(l)^-1/2 V^T
  that is c D u |W| |L|^2 = c D u cond(W) in L W L^T - I, and the same relative to the largest eigenvalue in L B L^T.  Ten Jacobi sweeps and
  four products of order D: c = 100.  Eigenvalues of W within 100 D u max(l), of the whitened B within 100 D u cond(W) max(m).  Rows, up to
  sign, within 8 x the difference between the restatement through numpy.linalg.eigh and the device's phases run on the host with one thread
  (inputs with neighbouring eigenvalues 25 % apart).
The largest ratios seen are printed (-s); DESIGN 4.8f records those of a run."""
import os

import numpy as np
import pytest

from dsr._capi import DsrError, Lda, Stc
from dsr.asr.adapt import LDATransformerPtr, STCTransformerPtr
from dsr.asr.train import LDAEstimatorPtr, STCEstimatorPtr
from tests import stc_np as S
from tests.conftest import PKG

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -53
DIMS = [1, 3, 15, 16, 17, 39, 40]                        # the 16-wide MFMA tile and either side of it; D (D + 1) / 2 on and off a multiple of 16
ITEMS = [1, 3, 63, 64, 65, 257]                          # items per estimator: around the MFMA k-step (4) and the chunk (64), several chunks
REFN = [1, 4, 17]
FACTORS = np.array([1.0, 0.37, -0.5, -1.25, 0.0, 2.0], f32)


def _items(rng, K, nFrames, counts):
    """unsorted items of len(counts) estimators, interleaved, with repeated (frame, distribution) pairs and factors of both signs and zero"""
    est = np.concatenate([np.full(c, a, np.int32) for a, c in enumerate(counts)]); n = len(est)
    frame = rng.integers(0, nFrames, n).astype(np.int32); dist = rng.integers(0, K, n).astype(np.int32)
    frame[n // 2:] = frame[:n - n // 2]; dist[n // 2:] = dist[:n - n // 2]                          # repeats
    fac = rng.choice(FACTORS, n); p = rng.permutation(n)
    return frame[p], dist[p], fac[p], est[p]


def _ratio(err, bound):
    assert np.all(err <= bound), float((err - bound).max())
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("ni", range(len(ITEMS)))
@pytest.mark.parametrize("di", range(len(DIMS)))
def test_items_and_statistics_match_the_restatement(dsr, cuda, di, ni):
    import torch
    D = DIMS[di]; R = REFN[(di + ni) % len(REFN)]; K = 5; nFrames = 41; cascade = bool((di + ni) % 2)
    counts = [ITEMS[ni], ITEMS[(ni + 1 + di) % len(ITEMS)]]
    rng = np.random.default_rng(100 * di + ni)
    m = S.synth_model(K, R, D, seed=7 + 100 * di + ni); gm = S.synth_model(1, R, D, seed=3 + di)
    xScore = (rng.standard_normal((nFrames, D)) * 2.0).astype(f32); xSrc = (xScore * f32(0.9) + rng.standard_normal((nFrames, D)).astype(f32) * f32(0.3)).astype(f32)
    frame, dist, fac, est = _items(rng, K, nFrames, counts)
    g = dsr.Gmm(**m); gg = dsr.Gmm(**gm); h = Stc(g, nEst=2, cascade=cascade, mmiEstimation=True); l = Lda(g, gg, nEst=2)
    refs = [S.Stc(m["refN"], m["mean"], m["ivar"], m["det"], cascade=cascade, mmi=True, track=True) for _ in range(2)]
    lrefs = [S.Lda(m["refN"], m["mean"], m["ivar"], m["det"], gm["mean"][0], R, track=True) for _ in range(2)]
    for e in range(2):                                                       # _stcInv is not the identity: W(2) sees its columns
        A = np.eye(D) + 0.2 * rng.standard_normal((D, D)) / np.sqrt(D); h.set_transform(A, e); refs[e].A = A; refs[e].Ainv = h.inverse(e)
        Ai = np.linalg.inv(A); assert np.abs(refs[e].Ainv - Ai).max() <= 20 * D * U * np.linalg.cond(A) * np.abs(Ai).max()
    xs, xr = torch.from_numpy(xScore).to(cuda), torch.from_numpy(xSrc).to(cuda)
    near, score = h.accumulate(xs, frame, dist, fac, est, xSrc=xr, want_nearest=True)
    lnear, lscore = l.accumulate(xs, frame, dist, fac, est, xSrc=xr, want_nearest=True)
    chosen = [refs[e].accu_one(int(d), xScore[f], xSrc[f], c) for f, d, c, e in zip(frame, dist, fac, est)]
    for f, d, c, e in zip(frame, dist, fac, est):
        lrefs[e].accu_one(int(d), xScore[f], xSrc[f], c)
    # item level: the nearest Gaussian is scoring mode 0's argmin, the score is mode 0's score
    sc, am = g.score(xs, mode=0, want_argmin=True); sc, am = sc.cpu().numpy(), am.cpu().numpy()
    assert np.array_equal(near, am[frame, dist].astype(np.int32)) and np.array_equal(near, lnear)
    assert np.array_equal(near, np.array([c - refs[0].off[d] for c, d in zip(chosen, dist)], np.int32))
    assert np.array_equal(score.view(np.int32), sc[frame, dist].view(np.int32)) and np.array_equal(score, lscore)
    low = np.tril(np.ones((D, D), bool)); worst = [0.0, 0.0, 0.0]
    for e in range(2):
        dev, ref = h.get_accu(e), refs[e]; n = ref.items
        assert n == counts[e] and dev["count"] == ref.count and dev["denCount"] == ref.denCount                # bit for bit
        assert not dev["sumOsq"][:, ~low].any() and not dev["regSq"][:, ~low].any()                          # only the lower triangle is written
        worst[0] = max(worst[0], _ratio(np.abs(dev["sumOsq"] - ref.sumOsq), (2 * n + 2) * U * ref.Sabs))
        worst[1] = max(worst[1], _ratio(np.abs(dev["regSq"] - ref.regSq), (2 * ref.denItems + 2 * D + 4 + -(-ref.denItems // 64)) * U * ref.Rabs))
        ldev, lref = l.get_accu(e), lrefs[e]
        assert ldev["count"] == lref.count
        for k, name in enumerate(("within", "between", "mixture")):
            assert not ldev[name][~low].any()
            worst[2] = max(worst[2], _ratio(np.abs(ldev[name] - getattr(lref, name)), (2 * n + 2) * U * lref.abs[k]))
    print("D=%d items=%s refN=%d cascade=%d: sumOsq at %.3f, regSq at %.3f, scatter at %.3f of the bound" % (D, counts, R, cascade, *worst))
    # the same call on fresh handles: the same bits
    h2 = Stc(g, nEst=2, cascade=cascade, mmiEstimation=True); l2 = Lda(g, gg, nEst=2)
    for e in range(2):
        h2.set_transform(refs[e].A, e)
    h2.accumulate(xs, frame, dist, fac, est, xSrc=xr); l2.accumulate(xs, frame, dist, fac, est, xSrc=xr)
    for e in range(2):
        d1, d2 = h.get_accu(e), h2.get_accu(e)
        assert np.array_equal(d1["sumOsq"].view(np.int64), d2["sumOsq"].view(np.int64)) and np.array_equal(d1["regSq"].view(np.int64), d2["regSq"].view(np.int64))
        d1, d2 = l.get_accu(e), l2.get_accu(e)
        assert all(np.array_equal(d1[k].view(np.int64), d2[k].view(np.int64)) for k in ("within", "between", "mixture"))


def _fed(dsr, cuda, D, nEst, T, seed, mmi=False, cascade=False, K=6, R=4):
    """device-made statistics of nEst estimators (T frames each, a quarter more as denominator frames with mmi) -> (model, gmm, handle)"""
    import torch
    T = T if isinstance(T, (list, tuple)) else [T] * nEst
    m, x, dist, Rot, lam = S.synth_stc(K, R, D, 2 * max(T), seed); g = dsr.Gmm(**m); h = Stc(g, nEst=nEst, cascade=cascade, mmiEstimation=mmi)
    xd = torch.from_numpy(x).to(cuda); rng = np.random.default_rng(seed)
    for e in range(nEst):
        fr = rng.permutation(len(x))[:T[e]]; n = len(fr)
        h.accumulate(xd, fr, dist[fr], np.ones(n, f32), np.full(n, e))
        if mmi:
            fr = rng.permutation(len(x))[:max(T[e] // 4, 1)]; n = len(fr)
            h.accumulate(xd, fr, dist[fr], np.full(n, -0.5, f32), np.full(n, e))
    return m, g, h


def _restate(m, h, e, A0, mmi, cascade):
    """the restatement carrying estimator e's numbers, started from A0"""
    s = S.Stc(m["refN"], m["mean"], m["ivar"], m["det"], cascade=cascade, mmi=mmi); dev = h.get_accu(e)
    s.count, s.denCount, s.sumOsq, s.regSq = dev["count"], dev["denCount"], dev["sumOsq"], dev["regSq"]; s.A = A0.copy()
    return s


@pytest.mark.parametrize("mode", ["ml", "mmi", "ml-cascade"])
@pytest.mark.parametrize("D", DIMS)
def test_stc_estimate_matches_the_restatement(dsr, cuda, D, mode, tmp_path):
    """four estimators in one call on the device-made statistics: two from the identity, two from a matrix loaded from a file"""
    mmi, cascade = mode == "mmi", mode == "ml-cascade"
    m, g, h = _fed(dsr, cuda, D, 4, max(50 * D, 60), seed=300 + D, mmi=mmi, cascade=cascade)
    rng = np.random.default_rng(D)
    for e in (2, 3):
        A = np.eye(D) + 0.05 * rng.standard_normal((D, D)); h.set_transform(A, e)
        fn = str(tmp_path / ("a%d.mat" % e)); h.save(fn, e); h.set_transform(np.eye(D), e); h.load(fn, e)
        assert np.array_equal(h.transform(e), A) and np.abs(h.inverse(e) @ A - np.eye(D)).max() < 1e-12
    start = [h.transform(e) for e in range(4)]
    before = [h.get_accu(e) for e in range(4)]
    h.estimate([0, 1, 2, 3], 1.0, 1.0)
    worst = 0.0
    for e in range(4):
        assert h.status(e) == 0
        Ad = h.transform(e)
        slu = _restate(m, h, e, start[e], mmi, cascade); Alu = slu.estimate(variant="lu")
        sin = _restate(m, h, e, start[e], mmi, cascade); Ain = sin.estimate(variant="inv")
        assert h.E(e) == slu.E
        yard = S.yardstick(slu, Alu, Ain) * (max(1.0, float(np.abs(start[e]).sum(0).max())) if cascade else 1.0)     # B A: the update's error times |A|_1
        err = float(np.abs(Ad - Alu).max()); worst = max(worst, err / yard)
        assert err <= 8 * yard, (e, err, yard)
        assert np.abs(h.inverse(e) @ Ad - np.eye(D)).max() <= 1e-9
        Si = np.linalg.inv(start[e]) if cascade else np.eye(D)                  # with cascade Q is the update's: B = A A0^-1, from A0
        Qd, Qs = slu.aux(Ad @ Si), slu.aux(Alu @ Si)
        assert Qd >= Qs - 8 * yard * abs(Qs), (e, Qd, Qs)
        assert Qd > slu.aux(start[e])
        if not cascade:
            assert abs(h.aux(e) - Qd) <= 1e-9 * abs(Qd)
        # the estimate read through sumOsq() / regSq(): the accumulators are symmetric now, their lower triangle is unchanged
        after = h.get_accu(e); assert np.array_equal(after["sumOsq"], S.sym(before[e]["sumOsq"])) and np.array_equal(after["regSq"], S.sym(before[e]["regSq"]))
    print("D=%d %s: A at %.3f of the yardstick (8 allowed)" % (D, mode, worst))


def test_make_pos_def_on_the_device(dsr, cuda):
    """statistics built so that minE is too small: E doubles to 8 (and is then multiplied); positive definite ones keep minE"""
    D = 4; m, g, h = _fed(dsr, cuda, D, 2, 200, seed=11, mmi=True)
    Sx = np.stack([np.tril(-5.0 * np.eye(D) + 0.01 * (k + 1) * np.ones((D, D))) for k in range(D)]); h.set_accu(1, sumOsq=Sx, regSq=np.stack([np.eye(D)] * D))
    h.estimate([0, 1], 1.0, 2.0)
    assert h.E(0) == 2.0 and h.E(1) == 16.0 and h.status(0) == 0 and h.status(1) == 0
    s = _restate(m, h, 1, np.eye(D), True, False); A = s.estimate(1.0, 2.0); assert s.E == 16.0
    assert np.abs(h.transform(1) - A).max() <= 1e-9 * np.abs(A).max()


@pytest.mark.parametrize("D", [3, 17, 39])
def test_deficient_estimator_is_refused(dsr, cuda, D):
    """an estimator with fewer frames than D, and one with a non-finite entry, are flagged and keep their matrices; the others are done"""
    m, g, h = _fed(dsr, cuda, D, 4, [50 * D, D - 1, 50 * D, 50 * D], seed=500 + D)
    A1 = np.eye(D) + 0.01 * np.random.default_rng(D).standard_normal((D, D)); h.set_transform(A1, 1)
    acc = h.get_accu(3); good = acc["sumOsq"][D - 1, D - 1, 0]; acc["sumOsq"][D - 1, D - 1, 0] = np.nan; h.set_accu(3, sumOsq=acc["sumOsq"])
    with pytest.raises(DsrError) as e:
        h.estimate([0, 1, 2, 3])
    assert e.value.status == dsr.E_CONSISTENCY
    assert h.E(1) == 0.0 and h.E(3) == 0.0 and h.E(0) == 1.0                # a flagged estimator keeps its E as well
    assert h.status(1) == dsr.E_CONSISTENCY and np.array_equal(h.transform(1), A1) and h.status(3) == dsr.E_CONSISTENCY and np.array_equal(h.transform(3), np.eye(D))
    for t in (0, 2):
        assert h.status(t) == 0
        A = _restate(m, h, t, np.eye(D), False, False).estimate()
        assert np.abs(h.transform(t) - A).max() <= 1e-6 * np.abs(A).max() and not np.array_equal(h.transform(t), np.eye(D))
    acc["sumOsq"][D - 1, D - 1, 0] = good; h.set_accu(3, sumOsq=acc["sumOsq"]); h.estimate(3)     # good statistics: the flag is cleared
    assert h.status(3) == 0


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stc_host")
    return S.build_host(tmp, os.path.join(PKG, "csrc")), tmp


@pytest.mark.parametrize("D", DIMS)
def test_lda_estimate(dsr, cuda, D, host):
    """four estimators a call on scatter matrices with a known spectrum, neighbouring eigenvalues 25 % apart; estimator 3 is not finite"""
    exe, tmp = host
    m = S.synth_model(2, 2, D, seed=D); g = dsr.Gmm(**m); h = Lda(g, g, nEst=4); ins = []
    for e in range(4):
        W, B, lam = S.synth_scatter(D, seed=20 * D + e); cnt = 100.0 + e; ins.append(lam)
        h.set_accu(e, count=cnt, within=np.tril(W * cnt), between=np.tril(B * cnt), mixture=np.tril((W + B) * cnt))
    bad = h.get_accu(3)["within"]; bad[0, 0] = np.inf; h.set_accu(3, within=bad)
    raw = [h.get_accu(e) for e in range(3)]
    with pytest.raises(DsrError) as err:
        h.estimate([0, 1, 2, 3])
    assert err.value.status == dsr.E_CONSISTENCY and h.status(3) == dsr.E_CONSISTENCY and np.array_equal(h.transform(3), np.eye(D))
    worst = [0.0, 0.0, 0.0, 0.0]
    for e in range(3):
        assert h.status(e) == 0
        acc = h.get_accu(e, through_accessor=True); W, B = acc["within"], acc["between"]
        assert np.array_equal(W, S.sym(raw[e]["within"] / raw[e]["count"])) and np.array_equal(acc["mixture"], S.sym(raw[e]["mixture"] / raw[e]["count"]))      # scaled in place
        L = h.transform(e); hw, hb = h.eigenvalues(e)
        ref = S.Lda([1], np.zeros((1, D)), np.ones((1, D)), [0.0], np.zeros(D), 1); Le, lw, lb = ref.solve(W, B)
        kappa = np.linalg.cond(W); tol = 100 * D * U * kappa
        worst[0] = max(worst[0], np.abs(L @ W @ L.T - np.eye(D)).max() / tol, np.abs(L @ B @ L.T - np.diag(hb)).max() / (tol * lb[0]))
        assert np.all(np.diff(hb) < 0) or D == 1
        worst[1] = max(worst[1], np.abs(np.sort(hw) - lw).max() / (100 * D * U * lw[-1]), np.abs(hb - lb).max() / (tol * lb[0]))
        assert np.allclose(hb, ins[e], rtol=1e-9)
        rc, Lh, _, _ = S.host_lda(exe, tmp, W, B); assert rc == 0
        flip = lambda X: np.sign((X * Le).sum(1))[:, None] * X                   # noqa: E731
        yard = float(np.abs(flip(Lh) - Le).max()); errL = float(np.abs(flip(L) - Le).max())
        worst[2] = max(worst[2], errL / yard if yard > 0 else 0.0); worst[3] = max(worst[3], float(np.abs(L - Lh).max()))
        assert errL <= 8 * yard, (e, errL, yard)
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    print("D=%d: invariants at %.3f, eigenvalues at %.3f of the bound; rows at %.3f of the eigh / Jacobi difference (8 allowed), |device - host phases| %.1e" % (D, *worst))
    h.estimate(0); again = h.get_accu(0, through_accessor=True)["within"]
    assert np.array_equal(again, S.sym(raw[0]["within"] / raw[0]["count"] / raw[0]["count"]))     # a second estimate divides again (eA:2754, 2921-2932)


def test_lda_refuses_another_codebook_size(dsr, cuda):
    import torch
    D = 3; m = S.synth_model(3, [2, 4, 2], D, seed=1); gm = S.synth_model(1, 2, D, seed=2); l = Lda(dsr.Gmm(**m), dsr.Gmm(**gm), 1)
    x = torch.zeros((4, D), device=cuda)
    l.accumulate(x, [0, 1], [0, 2], [1.0, 1.0], [0, 0]); assert l.get_accu(0)["count"] == 2.0
    with pytest.raises(DsrError) as e:
        l.accumulate(x, [0, 1], [0, 1], [1.0, 1.0], [0, 0])
    assert e.value.status == dsr.E_DIMENSION and l.get_accu(0)["count"] == 2.0       # eA:2995: refN 4 against the global codebook's 2


class _Frames(object):
    def __init__(self, x):
        self.x = x

    def size(self):
        return self.x.shape[1]

    def reset(self):
        pass

    def __iter__(self):
        return iter(self.x)


@pytest.mark.parametrize("D", DIMS)
def test_apply_and_streams_are_bit_exact(dsr, cuda, D, tmp_path):
    import torch
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    N = 300 if D < 39 else 131; rng = np.random.default_rng(40 + D); m = S.synth_model(2, 2, D, seed=D); g = dsr.Gmm(**m)
    x = (rng.standard_normal((N, D)) * 3.0).astype(f32); xd = torch.from_numpy(x).to(cuda)
    h = Stc(g, nEst=3); ref = S.Stc(m["refN"], m["mean"], m["ivar"], m["det"])
    for e in range(3):
        A = np.eye(D) + 0.3 * rng.standard_normal((D, D)); h.set_transform(A, e); ref.A = A
        assert np.array_equal(h.apply(xd, e).cpu().numpy().view(np.int32), ref.transform(x).view(np.int32))
    outDim = max(1, D - 2); l = Lda(g, g, nEst=2); lref = S.Lda(m["refN"], m["mean"], m["ivar"], m["det"], m["mean"][0], 2)
    Lm = rng.standard_normal((D, D)); l.set_transform(Lm, 1); lref.L = Lm
    for od in (outDim, D):
        out = l.apply(xd, od, 1).cpu().numpy(); assert out.shape == (N, od) and np.array_equal(out.view(np.int32), lref.apply(x, od).view(np.int32))
    # the stream operators: a bare transformer is the identity, then a loaded matrix
    src = PyVectorFloatFeatureStreamPtr(_Frames(x), "Src"); stc = STCTransformerPtr(src, D, 1, "STC")
    assert stc.size() == D and stc.name() == "STC" and np.array_equal(np.stack([np.array(v) for v in stc]), x)
    fn = str(tmp_path / "stc.mat"); h.save(fn, 2); assert open(fn, "rb").read() == ref.tran_bytes()
    stc.load(fn); stc.reset(); rows = np.stack([np.array(stc.next(t)) for t in range(N)])
    assert np.array_equal(rows.view(np.int32), ref.transform(x).view(np.int32))
    with pytest.raises(StopIteration):
        stc.next()
    with pytest.raises(DsrError) as e:
        stc.handle().estimate(0)
    assert e.value.status == dsr.E_CONSISTENCY                               # a transformer has no statistics
    with pytest.raises(DsrError) as e:
        stc.handle().accumulate(xd, [0], [0], [1.0], [0])
    assert e.value.status == dsr.E_CONSISTENCY
    src2 = PyVectorFloatFeatureStreamPtr(_Frames(x), "Src2"); lda = LDATransformerPtr(src2, outDim, 1, "LDA")
    assert lda.size() == outDim and lda.name() == "LDA"
    for fn_, args in ((lda.handle().estimate, (0,)), (lda.handle().accumulate, (xd, [0], [0], [1.0], [0])), (lda.handle().get_accu, (0,))):
        with pytest.raises(DsrError) as e:
            fn_(*args)
        assert e.value.status == dsr.E_CONSISTENCY
    fl = str(tmp_path / "lda.mat"); open(fl, "wb").write(Lm.astype("=f8").tobytes()); lda.load(fl)      # load reads float64
    rows = np.stack([np.array(v) for v in lda]); assert np.array_equal(rows.view(np.int32), lref.apply(x, outDim).view(np.int32))
    lda.save(fl); assert open(fl, "rb").read() == lref.tran_bytes()                                     # save writes float32
    if D > 1:
        with pytest.raises(DsrError) as e:
            lda.load(fl)
        assert e.value.status == dsr.E_IO                                    # half of what load wants (transform.cc:1961-1984)


def test_files_and_error_codes(dsr, cuda, tmp_path):
    import torch
    D = 5; m, g, h = _fed(dsr, cuda, D, 2, 40, seed=77, mmi=True); h.increment(-123.5, 40, 1)
    ref = _restate(m, h, 1, np.eye(D), True, False); ref.totalPr, ref.totalT = -123.5, 40
    fa = str(tmp_path / "a.stc"); h.save_accu(fa, 1); assert open(fa, "rb").read() == ref.accu_bytes()
    h.load_accu(fa, 0)                                                       # loading adds: estimator 0 now holds its own sums plus the file's
    a0 = h.get_accu(0); assert a0["totalT"] == 40 and a0["totalPr"] == float(f32(-123.5)) and a0["sumOsq"][0, 0, 1] == ref.sumOsq[0, 0, 1] != 0.0
    h.zero(0); h.load_accu(fa, 0); a0 = h.get_accu(0)
    assert a0["count"] == float(f32(ref.count)) and a0["denCount"] == float(f32(ref.denCount)) and np.array_equal(a0["sumOsq"], ref.sumOsq)
    assert np.array_equal(a0["regSq"], ref.regSq)
    h.estimate(1); ref.A = h.transform(1)
    ft = str(tmp_path / "t.mat"); h.save(ft, 1); assert open(ft, "rb").read() == ref.tran_bytes()
    assert np.array_equal(h.trans_matrix(1), ref.trans_matrix())
    ff = str(tmp_path / "f.mat"); h.save_float(ff, None, 1); assert open(ff, "rb").read() == ref.save_float_bytes()
    tr = np.random.default_rng(1).standard_normal((D, D)).astype(f32); h.save_float(ff, tr, 1); assert open(ff, "rb").read() == ref.save_float_bytes(tr)
    # LDA accumulator files
    l = Lda(g, g, 2); x = torch.from_numpy(np.random.default_rng(2).standard_normal((30, D)).astype(f32)).to(cuda)
    l.accumulate(x, np.arange(30), np.arange(30) % 6, np.full(30, 0.5, f32), np.zeros(30, np.int32))
    acc = l.get_accu(0); lref = S.Lda(m["refN"], m["mean"], m["ivar"], m["det"], m["mean"][0], 4)
    lref.count, lref.within, lref.between, lref.mixture = acc["count"], acc["within"], acc["between"], acc["mixture"]
    fl = str(tmp_path / "a.lda"); l.save_accu(fl, 0); assert open(fl, "rb").read() == lref.accu_bytes()
    l.load_accu(fl, 1); a1 = l.get_accu(1); assert a1["count"] == 15.0 and np.array_equal(a1["within"], lref.within) and a1["within"][0, 1] != 0.0
    l.zero(1); assert l.get_accu(1)["count"] == 0 and not l.get_accu(1)["mixture"].any()

    def status(fn, *a):
        with pytest.raises(DsrError) as e:
            fn(*a)
        return e.value.status
    assert status(h.zero, 2) == dsr.E_INDEX and status(h.save_accu, fa, 2) == dsr.E_INDEX and status(h.load_accu, fa, -1) == dsr.E_INDEX
    assert status(h.estimate, [0, 2]) == dsr.E_INDEX and status(h.estimate, [1, 1]) == dsr.E_PARAMETER and status(h.apply, x, 2) == dsr.E_INDEX
    assert status(h.load, str(tmp_path / "missing"), 0) == dsr.E_IO and status(h.load, ff, 0) == dsr.E_IO                   # the float file is too short
    assert status(h.set_transform, np.zeros((D, D)), 0) == dsr.E_CONSISTENCY
    other = Stc(dsr.Gmm(**S.synth_model(2, 2, D + 1, seed=1)), 1); assert status(other.load_accu, fa, 0) == dsr.E_DIMENSION
    assert status(l.estimate, [2]) == dsr.E_INDEX and status(l.apply, x, D + 1, 0) == dsr.E_DIMENSION
    assert status(h.accumulate, x, [30], [0], [1.0], [0]) == dsr.E_INDEX and status(h.accumulate, x, [0], [0], [1.0], [2]) == dsr.E_INDEX
    assert status(h.accumulate_path, x, [0, -1, 2]) == dsr.E_INDEX
    with pytest.raises(DsrError):
        Stc(dsr.Gmm(**S.synth_model(1, 1, 65, seed=1)), 1)                   # built for dimN <= 64


def test_two_passes(dsr, cuda, tmp_path, capsys):
    """decode, accumulate(bestPath()), estimate, decode again through dsr_decoder_decode_stream on the STC stream: the second decode sees the
    transformed frames; LDAEstimatorPtr takes the same path"""
    import torch
    from dsr.btk.feature import FeatureSetPtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    from dsr.asr.dictionary import LexiconPtr
    from dsr.asr.gaussian import CodebookSetBasicPtr, DistribSetBasicPtr
    from dsr.asr.decoder import WFSTFlyWeightPtr, DecoderFlyWeightPtr
    from tests import synth
    K, R, D, T = 24, 4, 8, 400
    m, x, _, Rot, lam = S.synth_stc(K, R, D, T, seed=5); m["val"][:] = f32(np.log(R))
    cbf, dsf = str(tmp_path / "cb.bin"), str(tmp_path / "ds.bin"); dsr.Gmm(**m).save(cbf, dsf)
    open(tmp_path / "cb.desc", "w").write("".join("%-25s%-20s%-10d%-3d%-10s\n" % ("cb%d" % k, "STC", R, D, "DIAGONAL") for k in range(K)))
    open(tmp_path / "ds.desc", "w").write("".join("%-25s%-25s\n" % ("ds%d" % k, "cb%d" % k) for k in range(K)))
    inlex = ["eps"] + ["ds%d" % k for k in range(K)] + ["SIL-m"]
    outlex = ["eps", "</s>"] + ["w%d" % i for i in range(50)]
    open(tmp_path / "in.lex", "w").write("\n".join(inlex) + "\n"); open(tmp_path / "out.lex", "w").write("\n".join(outlex) + "\n")
    arcs, fin = synth.random_wfst(400, K, seed=4, nWords=51, out_frac=0.2)
    with open(tmp_path / "g.fsm", "w") as f:
        for a in arcs:
            f.write("%d %d %d %d %.9g\n" % a)
        for s, c in fin:
            f.write("%d %.9g\n" % (s, c))
    src = PyVectorFloatFeatureStreamPtr(_Frames(x), "Src")
    # the distribution set scores the STC stream itself, so the estimator is built on a set that is built on it: a transformer first
    stc0 = STCTransformerPtr(src, D, 1, "STC"); fs0 = FeatureSetPtr(); fs0.add(stc0)
    cbs0 = CodebookSetBasicPtr(str(tmp_path / "cb.desc"), fs0, cbf); dss0 = DistribSetBasicPtr(cbs0, str(tmp_path / "ds.desc"), dsf)
    stc = STCEstimatorPtr(src, None, dss0, 0, None, False, False, 1, "STC"); fs = FeatureSetPtr(); fs.add(stc)
    cbs = CodebookSetBasicPtr(str(tmp_path / "cb.desc"), fs, cbf); dss = DistribSetBasicPtr(cbs, str(tmp_path / "ds.desc"), dsf)
    assert stc.size() == D and stc.name() == "STC"
    wfst = WFSTFlyWeightPtr(LexiconPtr("state"), LexiconPtr("in", str(tmp_path / "in.lex")), LexiconPtr("out", str(tmp_path / "out.lex")))
    wfst.read(str(tmp_path / "g.fsm"), binary=False)
    d = DecoderFlyWeightPtr(dss, beam=80.0, lmScale=12.0, silPenalty=0.5); d.set(wfst)
    d.decode(); path = list(d.bestPath())
    assert len(path) == T
    assert np.array_equal(np.stack([np.array(v) for v in stc]), x)           # the identity
    stc.accumulate(path); assert "STCEstimator: accumulated %d numerator frames." % T in capsys.readouterr().out
    assert stc.totalT() == T and stc.handle().get_accu(0)["count"] == T
    xd = torch.from_numpy(x).to(cuda); ids = np.array([int(n[2:]) for n in path])
    sc1 = dss.gmm.score(xd, mode=0, want_argmin=False)[0].cpu().numpy()
    assert stc.totalPr() == float(np.cumsum(sc1[np.arange(T), ids].astype(np.float64))[-1])       # eA:2273: the scores of the path, summed in fp64 in path order
    stc.estimate(); h = stc.handle(); A = h.transform(0)
    assert "Using E = 1" in capsys.readouterr().out and not np.array_equal(A, np.eye(D))
    d.decode()                                                               # resets the stream: the new matrix shows
    second = np.stack([np.array(v) for v in stc])
    assert np.array_equal(second.view(np.int32), h.apply(xd).cpu().numpy().view(np.int32)) and not np.array_equal(second, x)
    fn = str(tmp_path / "stc.f32"); stc.save(fn); assert np.array_equal(np.fromfile(fn, "=f4").reshape(D, D), stc.transMatrix())
    # LDA over the same path; the global codebook is codebook 0 of the set
    lda = LDAEstimatorPtr(src, None, dss0, dss0)
    score = lda.accumulate(path); assert score == stc.totalPr() and lda.handle().get_accu(0)["count"] == T
    lda.estimate(); L = lda.matrix(); acc = lda.handle().get_accu(0, through_accessor=True)
    assert np.abs(L @ acc["within"] @ L.T - np.eye(D)).max() <= 100 * D * U * np.linalg.cond(acc["within"])
    lda.zeroAccu(); assert lda.handle().get_accu(0)["count"] == 0
