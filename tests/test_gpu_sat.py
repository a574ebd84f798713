"""Speaker-adaptive training on the device (include/dsr.h section 14, csrc/sat_kernels.hip, csrc/sat.cpp) against tests/sat_np.py, the numpy
restatement of the ML slice of asr/sat/sat.cc ("sat").

Tolerances -- derived, not tuned.
  Mean accumulators, against the np.longdouble sums.  An entry sums n = (slots) bl terms.  sat:192-213 round, per term: T = a iv (1), the
  product of the dgemm (1), the scaling by c and the addition into the accumulator (2) for mat, n + 3 with the n - 1 additions; c b, the
  subtraction, T, the product (4) for vec, n + 4; one more (the division by c) for scalar, n + 5.  The device forms c iv exactly, rounds a a',
  iv v1 and every fused step once and adds a batch into the resident sums once: no more roundings than that, in another order.  So
  |mat - exact| <= (n + 3) 2^-53 sum |c iv a a'|, |vec - exact| <= (n + 4) 2^-53 sum |iv a| (|sumO| + |c b|), |scalar - exact| <=
  (n + 5) 2^-53 sum iv (|sumO| + |c b|)^2 / |c|; occ is the sequential double sum, bit for bit.
  Variance accumulators and transformed means.  Bit for bit: k_sat_var_acc does the restatement's operations in its order.
  Solve.  The criteria DESIGN 4.8d holds the MLLR solve to, on the device-made accumulators: full rank, the normwise backward error of the
  device's double solution is within 8x that of numpy.linalg.svd with the same 1e-7 rule; deficient, the kept rank is numpy's and the
  distance to numpy's truncated solution is within 8x the larger of numpy's own SVD / eigh difference and bl 2^-53 sigma_1 / sigma_r.
  Recovery.  On the full-rank recipe |double(mean) - mu*| <= 2^-23 |mu*| + 1e-10: one float ulp (a perturbed value may round across a
  boundary) plus a solve error LAPACK keeps four orders below.  Variances: 2^-23 sigma^2 (the float store) plus what the float transform
  leaves, sum c (trn - y)^2 / occ (computed by the restatement), plus 4 (slots) 2^-53 sum (|sumOsq| + 2 |trn sumO| + c trn^2) / occ.
The largest fraction of each accumulator bound seen is printed (-s); DESIGN 4.8h records those of a run."""
import numpy as np
import pytest

from dsr._capi import APT_RAPT, Apt, DsrError, ParamTree, Sat, SAT_MEAN, SAT_VARIANCE
from tests import apt_np as P
from tests import sat_cases as Cs
from tests import sat_np as N

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53
_cache = {}
_worst = dict(mat=0.0, vec=0.0, scalar=0.0)
needs_ld = pytest.mark.skipif(not N.HAVE_LD, reason="np.longdouble holds no more than a double here")
CASES = list(range(len(Cs.GPU_CASES)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _problem(ci):
    """the recipe for case ci with S + 2 speakers: the first batch takes S, the second two"""
    case = Cs.GPU_CASES[ci]; D, nB, S = case["D"], case["nB"], case["S"]; tf = None
    if case["path"] == "apt":
        L = D // nB
        def tf(s, rc):
            a = Cs.APT_ALPHAS[(3 * s + rc) % len(Cs.APT_ALPHAS)]; nb = (0, L, D)[(s + ci) % 3]
            bias = (0.3 * np.random.default_rng(1000 * s + rc).standard_normal(nb)).astype(f32)
            return N.apt_xform(P.matrix(APT_RAPT, [a], L), nB, bias)
    kind = N.APT if (nB > 1 and case["path"] == "raw") else N.MLLR
    return Cs.Problem(D, nB, case["leaves"], case["sizes"], S + 2, seed=300 + ci, kind=kind, transforms=tf)


def _fill(dsr, h, p, ci, slot, s, keep):
    """speaker s of the problem into a slot, by the case's path"""
    case = Cs.GPU_CASES[ci]; xf = p.xf[s]
    if case["path"] == "tree":
        t = ParamTree()
        for rc, x in xf.items():
            t.set(rc, np.concatenate([x.A[0], x.b[:, None]], axis=1))
        h.set_tree(slot, t)
    elif case["path"] == "apt":
        L = p.D // p.nB; apt = Apt(h.gmm, 1, APT_RAPT, L, p.nB, 0); keep.append(apt)
        for rc in xf:
            a = Cs.APT_ALPHAS[(3 * s + rc) % len(Cs.APT_ALPHAS)]; nb = (0, L, p.D)[(s + ci) % 3]
            apt.set_params(0, rc, [a], (0.3 * np.random.default_rng(1000 * s + rc).standard_normal(nb)).astype(f32))
        h.set_apt(slot, apt, 0)
    else:
        h.clear_slot(slot)
        for rc, x in xf.items():
            h.set_transform(slot, rc, x.kind, x.A, x.b if x.bSize else None)
    h.set_stats(slot, c=p.c[s], sumO=p.sumO[s], sumOsq=p.sumOsq[s])


def _make(dsr, p, S, massThreshold=1.0, nParts=1, part=1):
    g = dsr.Gmm(**p.m.as_kwargs()); g.set_reg_classes(p.classes)
    tr = dsr.Trainer(g); return Sat(tr, max(S, 2), massThreshold, nParts, part)


def _accumulated(dsr, ci, what, batches=2):
    """a fresh handle after one or two batches of `what`"""
    p = _problem(ci); S = Cs.GPU_CASES[ci]["S"]; h = _make(dsr, p, S); keep = []; h.keep_transformed(True); trn = []
    for first, n in ((0, S), (S, 2))[:batches]:
        for k in range(n):
            _fill(dsr, h, p, ci, k, first + k, keep)
        h.accumulate(what, n)
        if what == SAT_VARIANCE:
            trn += [h.transformed(k) for k in range(n)]
    return p, h, trn


def _case(dsr, ci):
    if ci not in _cache:
        p, h, _ = _accumulated(dsr, ci, SAT_MEAN); mat, vec, scalar, occ, has = h.mean_accus()
        _cache[ci] = dict(p=p, h=h, mat=mat, vec=vec, scalar=scalar, occ=occ, has=has, nsp=Cs.GPU_CASES[ci]["S"] + 2)
    return _cache[ci]


# ---- 1. the accumulators ------------------------------------------------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("ci", CASES)
def test_mean_accumulators_within_the_rounding_bound_of_the_exact_sums(dsr, cuda, ci):
    c = _case(dsr, ci); p = c["p"]; ld = p.mean_accus(N.LD); ref = p.mean_accus()
    n = c["nsp"] * (p.D // p.nB)
    assert dsr.load().dsr_sat_num_blocks(c["h"].h) == p.nB and c["mat"].shape == ld.mat.shape
    for name, got, want, mag, k in (("mat", c["mat"], ld.mat, ld.bmat, 3), ("vec", c["vec"], ld.vec, ld.bvec, 4), ("scalar", c["scalar"], ld.scalar, ld.bscalar, 5)):
        err = np.abs(got.astype(N.LD) - want).astype(f64); bound = (n + k) * U * mag
        frac = float((err / np.where(bound > 0, bound, 1.0)).max()); _worst[name] = max(_worst[name], frac)
        print("sat case %d %s: largest fraction of the bound %.4f (n = %d)" % (ci, name, frac, n))
        assert (err <= bound).all(), (name, frac)
    assert np.array_equal(_bits(c["occ"]), _bits(ref.occ)) and np.array_equal(c["has"].astype(bool), ref.has)
    assert np.array_equal(c["mat"], np.swapaxes(c["mat"], 2, 3))                                    # one value for both halves
    print("sat: largest fractions so far mat %.4f vec %.4f scalar %.4f" % (_worst["mat"], _worst["vec"], _worst["scalar"]))


@pytest.mark.parametrize("ci", CASES)
def test_variance_accumulators_and_transformed_means_bit_for_bit(dsr, cuda, ci):
    p, h, trn = _accumulated(dsr, ci, SAT_VARIANCE); va = N.VarAccus(p.G, p.D)
    for s in range(len(trn)):
        want = va.accumulate(p.classes, p.m.mean, p.c[s], p.sumO[s], p.sumOsq[s], p.xf[s])
        assert np.array_equal(_bits(trn[s]), _bits(want)), (s, np.abs(trn[s] - want).max())
    vec, occ = h.var_accus()
    assert np.array_equal(_bits(vec), _bits(va.vec)) and np.array_equal(_bits(occ), _bits(va.occ))
    v0, o0 = h.var_accu(p.G - 1)
    assert np.array_equal(v0, vec[-1]) and o0 == occ[-1]


@pytest.mark.parametrize("batches", [1, 2])
@pytest.mark.parametrize("ci", [2, 3, 6, 7])
def test_the_same_calls_twice_give_the_same_bits(dsr, cuda, ci, batches):
    a = _accumulated(dsr, ci, SAT_MEAN, batches)[1].mean_accus(); b = _accumulated(dsr, ci, SAT_MEAN, batches)[1].mean_accus()
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x) if x.dtype.kind == "f" else x, _bits(y) if y.dtype.kind == "f" else y)
    if batches == 2:                                                                                # the resident sums took the second batch in
        one = _accumulated(dsr, ci, SAT_MEAN, 1)[1].mean_accus()
        assert not np.array_equal(one[0], a[0]) and (a[3] > one[3]).all()


def test_zero_keeps_the_blocks_and_clears_the_sums(dsr, cuda):
    p, h, _ = _accumulated(dsr, 1, SAT_MEAN, 1); h.zero()
    mat, vec, scalar, occ, has = h.mean_accus()
    assert not mat.any() and not vec.any() and not scalar.any() and not occ.any() and has.all() and h.num_blocks() == 1
    h.accumulate(SAT_MEAN, Cs.GPU_CASES[1]["S"])
    again = _accumulated(dsr, 1, SAT_MEAN, 1)[1].mean_accus()
    assert np.array_equal(_bits(h.mean_accus()[0]), _bits(again[0]))


# ---- 2. the solve and the update ----------------------------------------------------------------------------------------------------------------
def _eta(G, w, z):
    return np.linalg.norm(G @ w - z) / (np.linalg.norm(G, 2) * np.linalg.norm(w) + np.linalg.norm(z))


@pytest.mark.parametrize("ci", CASES)
def test_update_decisions_counters_recovery_and_solve(dsr, cuda, ci):
    c = _case(dsr, ci); p, h = c["p"], c["h"]; before = h.gmm.params()["mean"].copy()
    want = N.update_means(c["mat"], c["vec"], c["scalar"], c["occ"], c["has"], before, 1.0)       # the restatement on the device's own accumulators
    r = h.update(SAT_MEAN); kept, dec, aO, aN = h.records(); x = h.solution(); after = h.gmm.params()["mean"]
    assert r["info"] == want["info"] and r["totals"] == want["totals"] == [p.G, p.G]
    assert np.array_equal(dec, want["decision"]) and np.array_equal(kept, want["kept"]) and (dec == N.UPDATED).all()
    aux = 0.0
    for g in range(p.G):
        for nb in range(p.nB):
            aux += aN[g, nb] if dec[g, nb] == N.UPDATED else aO[g, nb]
    assert _bits(np.array([r["aux"]]))[0] == _bits(np.array([aux]))[0]                            # the model-order sum of the device's values
    assert np.array_equal(_bits(after), _bits(x.astype(f32)))                                     # each component stored as float(q)
    bl = p.D // p.nB; worst = 0.0
    for g in range(p.G):
        for nb in range(p.nB):
            M, v = c["mat"][g, nb], c["vec"][g, nb]; xn, rank, sv = N.solve(M, v); xd = x[g, nb * bl:(nb + 1) * bl]
            assert rank == bl
            # the auxiliary values: the same bl^2 + 2 bl + 2 terms summed in another order, at the old mean and at the device's solution
            for got, at in ((aO[g, nb], before[g, nb * bl:(nb + 1) * bl].astype(f64)), (aN[g, nb], xd)):
                mag = 0.5 * (np.abs(at) @ np.abs(M) @ np.abs(at) + abs(c["scalar"][g, nb])) + np.abs(at) @ np.abs(v)
                assert abs(got - N.aux_func(M, v, float(c["scalar"][g, nb]), at)) <= 2 * (bl * bl + 2 * bl + 3) * U * mag, (g, nb)
            ed, en = _eta(M, xd, v), _eta(M, xn, v)
            assert ed <= 8 * max(en, U), (g, nb, ed, en)
            worst = max(worst, ed / max(en, U))
    print("sat case %d: largest backward error %.2f x LAPACK's" % (ci, worst))
    if Cs.GPU_CASES[ci]["path"] != "apt":                                                         # the full-rank recipe; a bilinear transform is not it
        assert (np.abs(after.astype(f64) - p.muStar) <= 2.0 ** -23 * np.abs(p.muStar) + 1e-10).all()


@pytest.mark.parametrize("D,k", Cs.DEFICIENT)
def test_deficient_solve_keeps_numpys_rank(dsr, cuda, D, k):
    p = Cs.Problem(D, 1, [1], [5], 1, seed=D, deficient=k); h = _make(dsr, p, 1)
    h.set_transform(0, 1, N.MLLR, p.xf[0][1].A, p.xf[0][1].b); h.set_stats(0, c=p.c[0], sumO=p.sumO[0], sumOsq=p.sumOsq[0]); h.accumulate(SAT_MEAN, 1)
    mat, vec, scalar, occ, has = h.mean_accus(); r = h.update(SAT_MEAN); kept, dec, aO, aN = h.records(); x = h.solution()
    assert r["info"] == [p.G, p.G, p.G * D, p.G * (D - k)] and (dec == N.UPDATED).all()
    for g in range(p.G):
        M, v = mat[g, 0], vec[g, 0]; xn, rank, sv = N.solve(M, v)
        assert kept[g, 0] == rank == D - k
        lam, V = np.linalg.eigh(M); keep = np.abs(lam) / np.abs(lam).max() >= 1e-7
        xe = V[:, keep] @ ((V[:, keep].T @ v) / lam[keep])
        allow = 8 * max(np.linalg.norm(xn - xe), D * U * sv[0] / sv[rank - 1] * np.linalg.norm(xn))
        assert np.linalg.norm(x[g] - xn) <= allow, (g, np.linalg.norm(x[g] - xn), allow)


def test_thresholds_zero_occupancy_keep_old_and_a_flagged_gaussian(dsr, cuda):
    D = 3; p = Cs.Problem(D, 1, [1], [6], 2, seed=5)
    # 0: below the threshold; 1: counts +5 and -5 (occ == 0 with blocks); 2: never a count; 3: indefinite at occ 15; 4: a NaN statistic; 5: plain
    p.c[0][:] = [4.0, 5.0, 0.0, 30.0, 20.0, 20.0]; p.c[1][:] = [3.0, -5.0, 0.0, -15.0, 9.0, 9.0]
    p.xf[0][1] = N.Xform(N.MLLR, 0.1 * np.eye(D), np.zeros(D)); p.xf[1][1] = N.Xform(N.MLLR, np.eye(D), np.zeros(D))
    p.sumO[1][4, 1] = np.nan
    for thr, left0 in ((-1.0, False), (0.0, True)):
        h = _make(dsr, p, 2, massThreshold=thr)
        for s in range(2):
            h.set_transform(s, 1, N.MLLR, p.xf[s][1].A, p.xf[s][1].b); h.set_stats(s, c=p.c[s], sumO=p.sumO[s], sumOsq=p.sumOsq[s])
        h.accumulate(SAT_MEAN, 2); mat, vec, scalar, occ, has = h.mean_accus()
        assert occ.tolist() == [7.0, 0.0, 0.0, 15.0, 29.0, 29.0] and has.tolist() == [1, 1, 0, 1, 1, 1]
        before = h.gmm.params()["mean"].copy()
        with pytest.raises(DsrError) as e:
            h.update(SAT_MEAN)
        assert e.value.status == 4 and h.gaussian_status(4) == 4 and [h.gaussian_status(g) for g in (0, 1, 2, 3, 5)] == [0] * 5
        after = h.gmm.params()["mean"]; kept, dec, aO, aN = h.records(); r = h.last
        ok = [0, 1, 2, 3, 5]
        want = N.update_means(mat[ok], vec[ok], scalar[ok], occ[ok], has[ok], before[ok], thr)
        assert np.array_equal(dec[ok], want["decision"]) and dec[4, 0] == 4
        assert dec[:, 0].tolist() == ([N.LEFT, N.LEFT, N.LEFT, N.KEPT_OLD, 4, N.UPDATED] if left0 else [N.UPDATED, N.ZEROED, N.LEFT, N.KEPT_OLD, 4, N.UPDATED])
        assert np.array_equal(_bits(after[4]), _bits(before[4])) and np.array_equal(_bits(after[2]), _bits(before[2]))
        assert np.array_equal(_bits(after[3]), _bits(before[3])) and aO[3, 0] < aN[3, 0] - 1.0
        assert np.array_equal(_bits(after[0]), _bits(before[0])) == left0 and (not after[1].any()) == (not left0)
        assert not np.array_equal(after[5], before[5])                                            # the others finish
        assert r["info"] == want["info"] and r["totals"] == [6, 3 if left0 else 6]                # the flagged Gaussian counts in the totals only


def test_variance_update_recovers_sigma2_and_leaves_variances(dsr, cuda):
    ci = 4; p = _problem(ci); S = Cs.GPU_CASES[ci]["S"]; p.m.mean = p.muStar.astype(f32); h = _make(dsr, p, S, massThreshold=0.0); keep = []
    p.c[1][3] = 0.0; p.c[0][3] = 2.0; p.c[2][3] = 3.0                                             # Gaussian 3 stays below the threshold of 10
    va = N.VarAccus(p.G, p.D); before = h.gmm.params()["cv"].copy()
    for s in range(S):
        _fill(dsr, h, p, ci, s, s, keep); va.accumulate(p.classes, p.m.mean, p.c[s], p.sumO[s], p.sumOsq[s], p.xf[s], exact=p.y[s])
    h.accumulate(SAT_VARIANCE, S); r = h.update(SAT_VARIANCE); cv = h.gmm.params()["cv"]
    want, tot = N.update_variances(va.vec, va.occ, before, 0.0)
    assert r["totals"] == tot == [p.G, p.G - 1] and np.array_equal(_bits(cv), _bits(want))
    assert np.array_equal(_bits(cv[3]), _bits((1.0 / before[3].astype(f64)).astype(f32)))         # fixup: the slot holds variances everywhere
    ok = np.arange(p.G) != 3
    tol = 2.0 ** -23 * p.sigma2 + (va.model + 4 * S * U * va.bound) / va.occ[:, None]
    assert (np.abs(cv.astype(f64) - p.sigma2) <= tol)[ok].all()


# ---- 3. through the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [SAT_MEAN, SAT_VARIANCE])
def test_updated_model_scores_and_saves_as_a_model_built_from_its_parameters(dsr, cuda, what, tmp_path):
    import torch
    ci = 2; p, h, _ = _accumulated(dsr, ci, what, 1); tr = h.trainer; q0 = h.gmm.params()
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((40, p.D)).astype(f32)).to(cuda)
    before = [h.gmm.score(x, mode)[0].cpu().numpy() for mode in (0, 1, 2)]                       # every mode has its device image built
    kw = p.m.as_kwargs()
    if what == SAT_MEAN:
        mat, vec, scalar, occ, has = h.mean_accus(); kw["mean"] = N.update_means(mat, vec, scalar, occ, has, q0["mean"], 1.0)["mean"]
    else:
        vec, occ = h.var_accus(); kw["ivar"] = N.update_variances(vec, occ, q0["cv"], 1.0)[0]
    h.update(what); other = dsr.Gmm(**kw)
    if what == SAT_VARIANCE:
        tr.invert_variances(); tr.fix_gconsts(); t2 = dsr.Trainer(other); t2.invert_variances(); t2.fix_gconsts()
    q = h.gmm.params()
    assert np.array_equal(_bits(q["mean"]), _bits(other.params()["mean"])) and np.array_equal(_bits(q["cv"]), _bits(other.params()["cv"]))
    for mode in (0, 1, 2):
        a = h.gmm.score(x, mode)[0].cpu().numpy(); b = other.score(x, mode)[0].cpu().numpy()
        assert np.array_equal(a, b) and not np.array_equal(a, before[mode]), mode
    cb, ds = str(tmp_path / "m.cb"), str(tmp_path / "m.ds"); h.gmm.save(cb, ds)
    back = dsr.Gmm(files=(cb, ds)).params()
    assert np.array_equal(_bits(back["mean"]), _bits(q["mean"])) and np.array_equal(_bits(back["cv"]), _bits(q["cv"]))


# ---- 4. slot tables and refusals ----------------------------------------------------------------------------------------------------------------
def test_slot_tables_from_a_tree_an_apt_handle_and_arrays(dsr, cuda):
    D = 6; p = Cs.Problem(D, 1, [2, 3], [3, 2], 1, seed=1); h = _make(dsr, p, 2)
    rng = np.random.default_rng(2); W = rng.standard_normal((D, D + 1)); t = ParamTree(); t.set(2, W); t.set(3, 2 * W)
    h.set_tree(0, t)
    assert h.slot_classes(0) == [2, 3]
    k, A_, b, bs = h.get_transform(0, 3)
    assert (k, bs) == (N.MLLR, D) and np.array_equal(A_[0], 2 * W[:, :D]) and np.array_equal(b, 2 * W[:, D])
    apt = Apt(h.gmm, 1, APT_RAPT, 3, 2, 0); bias = np.array([0.5, -0.25, 0.125], f32); apt.set_params(0, 2, [0.2], bias); apt.set_params(0, 3, [-0.1])
    h.set_apt(1, apt, 0)
    k, A_, b, bs = h.get_transform(1, 2); M = P.matrix(APT_RAPT, [0.2], 3)
    assert (k, bs, A_.shape) == (N.APT, 3, (2, 3, 3)) and np.array_equal(_bits(A_[0]), _bits(M)) and np.array_equal(A_[1], A_[0])
    assert b.tolist() == [0.5, -0.25, 0.125, 0.0, 0.0, 0.0] and h.get_transform(1, 3)[3] == 0
    h.set_transform(1, 7, N.APT, np.stack([np.eye(2)] * 3), None)
    assert h.slot_classes(1) == [2, 3, 7] and h.get_transform(1, 7)[1].shape == (3, 2, 2)
    h.clear_slot(1)
    assert h.slot_classes(1) == []
    bad = ParamTree(); bad.set(2, np.zeros((D - 1, D)))
    four = np.zeros(36)                                                                           # four blocks do not divide dimN = 6 (sat:63-65)
    for call, status in ((lambda: h.set_transform(0, 0, N.MLLR, np.eye(D)), dsr.E_INDEX),                  # class 0: _setNode(0)
                         (lambda: dsr.check(dsr.load().dsr_sat_set_transform(h.h, 0, 2, N.APT, 4, four.ctypes.data, None)), dsr.E_DIMENSION),
                         (lambda: h.set_transform(0, 2, 3, np.eye(D)), dsr.E_PARAMETER),
                         (lambda: h.set_tree(0, bad), dsr.E_DIMENSION), (lambda: h.set_stats(5, c=np.zeros(5), sumO=np.zeros((5, D)), sumOsq=np.zeros((5, D))), dsr.E_INDEX)):
        with pytest.raises(DsrError) as e:
            call()
        assert e.value.status == status
    assert h.slot_classes(0) == [2, 3]                                                            # a refused tree leaves the slot as it was


def test_accumulate_refusals(dsr, cuda):
    D = 4; p = Cs.Problem(D, 1, [2, 3], [3, 2], 2, seed=3); h = _make(dsr, p, 2); I = np.eye(D)
    def fill(s, classes, nB=1):
        h.clear_slot(s)
        for rc in classes:
            h.set_transform(s, rc, N.APT if nB > 1 else N.MLLR, np.stack([np.eye(D // nB)] * nB), np.zeros(D))
        h.set_stats(s, c=p.c[s], sumO=p.sumO[s], sumOsq=p.sumOsq[s])
    for what in (SAT_MEAN, SAT_VARIANCE):
        fill(0, [2])
        with pytest.raises(DsrError) as e:
            h.accumulate(what, 1)
        assert e.value.status == dsr.E_KEY and "Could not find node 3" in str(e.value)            # the exact node, no ancestor
        fill(0, [2, 3, 6])
        with pytest.raises(DsrError) as e:
            h.accumulate(what, 1)
        assert e.value.status == dsr.E_CONSISTENCY and "not a leaf" in str(e.value)
        fill(0, [2, 3]); fill(1, [2, 3], nB=2)
        with pytest.raises(DsrError) as e:
            h.accumulate(what, 2)
        assert e.value.status == dsr.E_DIMENSION
    with pytest.raises(DsrError) as e:
        h.accumulate(3, 1)
    assert e.value.status == dsr.E_PARAMETER
    with pytest.raises(DsrError) as e:
        h.mean_accus()
    assert e.value.status == dsr.E_CONSISTENCY and h.num_blocks() == 0                            # nothing was accumulated
    h.accumulate(SAT_MEAN, 1); fill(0, [2, 3], nB=2)
    with pytest.raises(DsrError) as e:
        h.accumulate(SAT_MEAN, 1)                                                                 # a second batch with another block count, sat:57-59
    assert e.value.status == dsr.E_DIMENSION and h.num_blocks() == 1
    g = dsr.Gmm(**p.m.as_kwargs()); h0 = Sat(dsr.Trainer(g), 1); h0.set_transform(0, 1, N.MLLR, I)
    with pytest.raises(DsrError) as e:
        h0.accumulate(SAT_MEAN, 1)                                                                # a model without classes: class 0
    assert e.value.status == dsr.E_INDEX


# ---- 5. files -------------------------------------------------------------------------------------------------------------------------------------
def _speaker_files(dsr, p, tmp_path, labels):
    """<tmp>/accu_<label>.cbs.accu by dsr_train_save_codebook_accus and <tmp>/par_<label> by dsr_mllr_write, for the problem's speakers"""
    g = dsr.Gmm(**p.m.as_kwargs()); g.set_reg_classes(p.classes); tr = dsr.Trainer(g); ml = dsr.Mllr(g, 1); pr, tt = [], []
    for s, lab in enumerate(labels):
        tr.zero(); tr.set(count=p.c[s], den=np.zeros(p.G), sumO=p.sumO[s], sumOsq=p.sumOsq[s])
        pr.append(f32(-1234.5 * (s + 1))); tt.append(100 + 7 * s)
        tr.save_codebook_accus(str(tmp_path / ("accu_%s.cbs.accu" % lab)), float(pr[-1]), tt[-1])
        t = ml.tree(0); t.clear()
        for rc, x in p.xf[s].items():
            t.set(rc, np.concatenate([x.A[0], x.b[:, None]], axis=1))
        ml.write(0, str(tmp_path / ("par_%s" % lab)))
    (tmp_path / "spk.txt").write_text("".join(l + "\n" for l in labels))
    return pr, tt


@pytest.mark.parametrize("what", [SAT_MEAN, SAT_VARIANCE])
def test_estimate_files_equals_the_in_memory_path(dsr, cuda, tmp_path, what):
    labels = ["spkA", "B02", "c"]; p = Cs.Problem(13, 1, [2, 3], [20, 13], 3, seed=77, refN=[10, 10, 13]); pr, tt = _speaker_files(dsr, p, tmp_path, labels)
    pre = str(tmp_path) + "/"
    for slots in (3, 2):                                                                          # one batch, and a batch of two then one
        # in memory: the same files, loaded by hand, in the batches the handle's slots make
        h = _make(dsr, p, slots); tr = h.trainer
        for s, lab in enumerate(labels):
            tr.zero(); tr.load_codebook_accus(pre + "accu_%s.cbs.accu" % lab); h.set_stats(s % slots, trainer=tr); h.set_tree(s % slots, ParamTree(pre + "par_" + lab))
            if s % slots == slots - 1 or s == 2:
                h.accumulate(what, s % slots + 1)
        tr.zero(); h.update(what); want = h.gmm.params()
        f = _make(dsr, p, slots)
        ret = f.estimate_files(what, pre + "spk.txt", pre + "par_", pre + "accu_"); got = f.gmm.params()
        assert ret == N.estimate_return(pr, tt)
        assert np.array_equal(_bits(got["mean"]), _bits(want["mean"])) and np.array_equal(_bits(got["cv"]), _bits(want["cv"]))
        assert not np.array_equal(got["mean" if what == SAT_MEAN else "cv"], p.m.mean if what == SAT_MEAN else p.m.cv)
        assert not f.trainer.get()["count"].any()                                                 # the model accumulators are zeroed (sat:1833)


def test_estimate_files_parts_errors_and_the_facade(dsr, cuda, tmp_path):
    labels = ["s1", "s2", "s3"]; p = Cs.Problem(5, 1, [2, 3], [6, 6], 3, seed=78, refN=[3, 3, 3, 3]); pr, tt = _speaker_files(dsr, p, tmp_path, labels)
    pre = str(tmp_path) + "/"
    h = _make(dsr, p, 3, nParts=2, part=1); before = h.gmm.params()["mean"].copy()
    h.estimate_files(SAT_MEAN, pre + "spk.txt", pre + "par_", pre + "accu_"); after = h.gmm.params()["mean"]
    assert np.array_equal(_bits(after[6:]), _bits(before[6:])) and (after[:6] != before[:6]).all()
    assert h.mean_accus()[3][6:].tolist() == [0.0] * 6 and (h.mean_accus()[3][:6] > 0).all()       # (nParts, part) = (2, 1) touches only its codebooks
    (tmp_path / "one.txt").write_text("s1\nnobody\n")
    with pytest.raises(DsrError) as e:
        _make(dsr, p, 3).estimate_files(SAT_MEAN, pre + "one.txt", pre + "par_", pre + "accu_")
    assert e.value.status == dsr.E_IO
    (tmp_path / "accu_nopar.cbs.accu").write_bytes((tmp_path / "accu_s1.cbs.accu").read_bytes()); (tmp_path / "np.txt").write_text("nopar\n")
    with pytest.raises(DsrError) as e:
        _make(dsr, p, 3).estimate_files(SAT_MEAN, pre + "np.txt", pre + "par_", pre + "accu_")
    assert e.value.status == dsr.E_IO and "par_nopar" in str(e.value)                             # a missing parameter file
    t = ParamTree(pre + "par_s2"); t.set(6, t.find(3, False)); t.write(pre + "par_s2")           # class 3 gains a child: not a leaf
    with pytest.raises(DsrError) as e:
        _make(dsr, p, 3).estimate_files(SAT_MEAN, pre + "spk.txt", pre + "par_", pre + "accu_")
    assert e.value.status == dsr.E_CONSISTENCY and "not a leaf" in str(e.value)


def test_facade_estimate_returns_the_same_number(dsr, cuda, tmp_path):
    from dsr.asr.sat import MeanSATPtr, SpeakerListPtr, VarianceSATPtr
    labels = ["s1", "s2", "s3"]; p = Cs.Problem(5, 1, [2, 3], [6, 6], 3, seed=79, refN=[3, 3, 3, 3]); pr, tt = _speaker_files(dsr, p, tmp_path, labels)
    pre = str(tmp_path) + "/"
    h = _make(dsr, p, 3); want = h.estimate_files(SAT_MEAN, pre + "spk.txt", pre + "par_", pre + "accu_"); wantMean = h.gmm.params()["mean"]

    class Cbs(object):                                                                            # what the façade asks of a CodebookSetTrainPtr
        def __init__(self, tr):
            self._trainer = tr; self._sub = None

        def _need(self):
            return self._trainer
    g = dsr.Gmm(**p.m.as_kwargs()); g.set_reg_classes(p.classes); cbs = Cbs(dsr.Trainer(g))
    sat = MeanSATPtr(cbs, 0, 0.0, 1.0, slots=3)
    assert sat.estimate(SpeakerListPtr(pre + "spk.txt"), pre + "par_", pre + "accu_") == want == N.estimate_return(pr, tt)
    assert np.array_equal(_bits(g.params()["mean"]), _bits(wantMean))
    assert isinstance(VarianceSATPtr(cbs, 5).estimate(SpeakerListPtr(pre + "spk.txt"), pre + "par_", pre + "accu_"), float)
    for args, status in (((cbs, 7), dsr.E_DIMENSION), ((cbs, 0, 0.5), dsr.E_PARAMETER), ((cbs, 0, 0.0, 0.0, 1, 1, 2.0), dsr.E_PARAMETER),
                         ((cbs, 0, 0.0, 0.0, 1, 1, 1.0, True), dsr.E_PARAMETER)):      # the MMI-SAT options are refused, not ignored
        with pytest.raises(DsrError) as e:
            MeanSATPtr(*args)
        assert e.value.status == status
