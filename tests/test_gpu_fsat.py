"""Fast speaker-adaptive training on the device (include/dsr.h section 14b, csrc/fsat_kernels.hip, csrc/fsat.cpp) against tests/fsat_np.py, the
numpy restatement of asr/sat/codebookFastSAT.cc ("cfs") and of MDLSATMean / FastSAT / FastAcc in asr/sat/sat.cc ("sat").

Tolerances -- derived, not tuned.
  k_fsat_norm.  Bit for bit: counts, fastMean, fastVar, scalar are the restatement's operations in its order.
  Matrix-only accumulate.  mat within (n + 3) 2^-53 sum |c iv a a'| of the np.longdouble sums, n = (slots) bl: the bound, and its derivation, of
  tests/test_gpu_sat.py for the same sum; occ bit for bit; mat also bit for bit what dsr_sat_accumulate(1) leaves for the same slots.
  Solve, on the device's own sums.  Decisions, kept sets' sizes, descLen, UpdateInfo, totals and the auxiliary sum equal the restatement's under
  the input conditions tests/test_fsat_np_cpu.py asserts for the same cases.  With thr = 0 (nothing dropped) the normwise backward error of the
  device's double solution is within 8x that of numpy.linalg.svd with the 1e-7 rule (as test_gpu_sat.py).  With directions dropped
  the solution is V_kept diag(1 / l) V_kept^T vec: the rounding of a Jacobi sweep perturbs M by E, |E| <= bl 2^-53 lmax; the kept subspace turns by
  at most |E| / gap (Davis-Kahan, gap = the smallest distance of a kept to a dropped eigenvalue) and the kept inverse moves by |E| / lmin_kept
  relative, so |x - x_numpy| <= 8 bl 2^-53 (lmax / gap + lmax / lmin_kept) |vec| / lmin_kept for both decompositions together.
  The variances are float(varVec / occ) bit for bit; each mean component is float(x).
  End to end.  From one starting model MeanSAT solves M x = vec with vec summed on the MFMA and VarianceSAT forms sum (sumOsq - 2 trn sumO + c
  trn^2) / occ with trn = transform(starting mean); the fast path has the same M (the same kernel, bit for bit), vec = sum_s (A o iv)^T (sumO -
  c b) summed sequentially, and fastVar is VarianceSAT's sum in its order.  With thr = 0 nothing is dropped and both accept: the means agree to
  one float ulp + 1e-10 (the bound test_gpu_sat.py gives a recovered mean), the variances bit for bit; through the file fastVar is rounded to
  float once more and the quotient stored as float: 2^-22 relative.  The statistics of this test are floats, so that the full files the two-pass
  path reads hold what the trainer held when the fast path folded it.
The largest fraction of the accumulator bound and the largest backward-error ratio seen are printed (-s); DESIGN 4.8i records those of a run."""
import numpy as np
import pytest

from dsr._capi import APT_RAPT, Apt, DsrError, FastSat, ParamTree, Sat, SAT_MEAN, SAT_VARIANCE
from tests import fsat_cases as Fc
from tests import fsat_np as F
from tests import sat_cases as Cs
from tests import sat_np as N

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53
needs_ld = pytest.mark.skipif(not N.HAVE_LD, reason="np.longdouble holds no more than a double here")
_worst = dict(mat=0.0, eta=0.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(np.asarray(a) + 0.0), _bits(np.asarray(b) + 0.0))                  # -0.0 + 0.0 = +0.0: a sum that starts at +0.0 never holds -0.0


def _make(dsr, p, S, thr=0.0, mass=Fc.MASS, nParts=1, part=1, meanOnly=False, classes=True, cls=FastSat):
    g = dsr.Gmm(**p.m.as_kwargs())
    if classes:
        g.set_reg_classes(p.classes)
    tr = dsr.Trainer(g)
    return cls(tr, max(S, 2), thr, mass, nParts, part, meanOnly) if cls is FastSat else cls(tr, max(S, 2), mass, nParts, part)


def _transforms(h, p, path, ci, slot, s, keep):
    xf = p.xf[s]
    if path == "tree":
        t = ParamTree()
        for rc, x in xf.items():
            t.set(rc, np.concatenate([x.A[0], x.b[:, None]], axis=1))
        h.set_tree(slot, t)
    elif path == "apt":
        L = p.D // p.nB; apt = Apt(h.gmm, 1, APT_RAPT, L, p.nB, 0); keep.append(apt)
        for rc in xf:
            a, bias = Fc.apt_params(ci, p, s, rc); apt.set_params(0, rc, [a], bias)
        h.set_apt(slot, apt, 0)
    else:
        h.clear_slot(slot)
        for rc, x in xf.items():
            h.set_transform(slot, rc, x.kind, x.A, x.b if x.bSize else None)


def _fill(h, p, path, ci, slot, s, keep, full=True):
    _transforms(h, p, path, ci, slot, s, keep)
    if full:
        h.set_stats(slot, count=p.num[s], den=p.den[s], sumO=p.sumO[s], sumOsq=p.sumOsq[s])
    else:
        h.set_counts(slot, count=p.num[s], den=p.den[s])


def _fast_equal(got, want):
    """the dict of get_fast against a restatement's FastAccus, or another such dict"""
    return all(_same(got[k], want[k] if isinstance(want, dict) else getattr(want, k)) for k in ("count", "den", "fastMean", "fastVar", "scalar"))


# ---- 1. k_fsat_norm ---------------------------------------------------------------------------------------------------------------------------------
def _normed(dsr, ci, batches=2):
    case = Fc.NORM_CASES[ci]; p = Fc.norm_problem(ci); S = case["S"]; keep = []
    h = _make(dsr, p, S, classes=case["leaves"] != [1])                                           # class 1 everywhere: left to setRegClassesToOne
    out = []
    for first, n in ((0, S), (S, 2))[:batches]:
        for k in range(n):
            _fill(h, p, case["path"], ci, k, first + k, keep)
        h.norm(n); out.append(h.get_fast())
    return p, h, out


@pytest.mark.parametrize("ci", range(len(Fc.NORM_CASES)))
def test_norm_bit_for_bit_over_two_batches(dsr, cuda, ci):
    p, h, got = _normed(dsr, ci); S = Fc.NORM_CASES[ci]["S"]
    one = Fc.fold(p, range(S)); two = Fc.fold(p, range(S, S + 2), one.copy())
    assert h.fast_blocks() == p.nB == h.desc_blocks() and got[0]["scalar"].shape == (p.G, p.nB)
    for name in ("count", "den", "fastMean", "fastVar", "scalar"):
        assert _same(got[0][name], getattr(one, name)), (name, np.abs(got[0][name] - getattr(one, name)).max())
        assert _same(got[1][name], getattr(two, name)), (name, np.abs(got[1][name] - getattr(two, name)).max())
    assert not np.array_equal(got[0]["fastMean"], got[1]["fastMean"])                              # the resident values took the second batch in
    if p.G > 2:                                                                                   # speaker 0: no count, |ck| < 1e-6, ck = -8
        first = Fc.fold(p, [0])
        assert first.count[-1] == 5.0 and not first.fastMean[-1].any() and first.scalar[p.G // 2].min() < 0
    assert h.gmm.reg_classes().tolist() == p.classes.tolist() and h.desc_length() == p.G * p.nB


@pytest.mark.parametrize("ci", [2, 4])
def test_norm_twice_gives_the_same_bits(dsr, cuda, ci):
    a = _normed(dsr, ci)[2]; b = _normed(dsr, ci)[2]
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(_bits(x[k]), _bits(y[k])), k


def test_zero_fast_set_fast_and_the_file(dsr, cuda, tmp_path):
    ci = 2; p, h, got = _normed(dsr, ci, 1); S = Fc.NORM_CASES[ci]["S"]; want = Fc.fold(p, range(S)); path = str(tmp_path / "fast.accu")
    refN = [int(r) for r in p.m.refN]; names = list(p.m.cbNames)
    h.save_fast(path); data = open(path, "rb").read()
    assert data == F.save_fast(want, refN, names)                                                 # byte for byte the restatement's file
    fresh = _make(dsr, p, 1); assert fresh.fast_blocks() == 0
    with pytest.raises(DsrError) as e:
        fresh.get_fast()
    assert e.value.status == dsr.E_CONSISTENCY
    fresh.load_fast(path); one = F.load_fast(data, None, refN, names, p.D)
    assert fresh.fast_blocks() == p.nB and _fast_equal(fresh.get_fast(), one)
    fresh.load_fast(path); assert _fast_equal(fresh.get_fast(), F.load_fast(data, one, refN, names, p.D))      # load ADDS
    part = _make(dsr, p, 1); part.load_fast(path, 2, 2); k0 = len(refN) // 2
    assert _fast_equal(part.get_fast(), F.load_fast(data, None, refN, names, p.D, ks=range(k0, len(refN))))
    h.zero_fast(); assert h.fast_blocks() == 0
    h.norm(S); assert _fast_equal(h.get_fast(), want)                                             # allocated and zeroed again, not added to
    h.set_fast(one.count, one.den, one.fastMean, one.fastVar, one.scalar); assert _fast_equal(h.get_fast(), one)
    # refusals of the file
    (tmp_path / "cut.accu").write_bytes(data[:-7])
    with pytest.raises(DsrError) as e:
        _make(dsr, p, 1).load_fast(str(tmp_path / "cut.accu"))
    assert e.value.status == dsr.E_IO
    before = h.get_fast()
    with pytest.raises(DsrError) as e:
        h.load_fast(str(tmp_path / "cut.accu"))
    assert e.value.status == dsr.E_IO and _fast_equal(h.get_fast(), before)        # a refused file leaves the accumulators as they were
    three = F.FastAccus(p.G, p.D, 3); three.count[:] = 1.0; (tmp_path / "three.accu").write_bytes(F.save_fast(three, refN, names))
    with pytest.raises(DsrError) as e:
        h.load_fast(str(tmp_path / "three.accu"))                                                 # another nblks
    assert e.value.status == dsr.E_DIMENSION and "nblks" in str(e.value)
    other = F.FastAccus(p.G, p.D + 1, 1); other.count[:] = 1.0
    (tmp_path / "org.accu").write_bytes(F.save_fast(other, refN, names))
    with pytest.raises(DsrError) as e:
        _make(dsr, p, 1).load_fast(str(tmp_path / "org.accu"))                                    # another dimN / orgDimN
    assert e.value.status == dsr.E_DIMENSION
    with pytest.raises(DsrError) as e:
        _make(dsr, p, 1).load_fast(str(tmp_path / "missing.accu"))
    assert e.value.status == dsr.E_IO


# ---- 2. the matrix-only accumulate ------------------------------------------------------------------------------------------------------------------
MAT_CASES = [(1, None), (2, None), (4, None), (None, dict(D=81, nB=1, leaves=[1], sizes=[3], S=1, path="raw"))]


def _mat_problem(mi):
    ci, case = MAT_CASES[mi]
    if ci is not None:
        return ci, Fc.NORM_CASES[ci], Fc.norm_problem(ci)
    return 9, case, Fc.with_counts(Cs.Problem(case["D"], 1, case["leaves"], case["sizes"], case["S"] + 2, seed=581), 681)


@needs_ld
@pytest.mark.parametrize("mi", range(len(MAT_CASES)))
def test_matrix_only_accumulate(dsr, cuda, mi):
    ci, case, p = _mat_problem(mi); S = case["S"]; keep = []; h = _make(dsr, p, S); fast = Fc.fold(p)
    h.set_fast(fast.count, fast.den, fast.fastMean, fast.fastVar, fast.scalar); h.add_fast()
    two = _make(dsr, p, S, cls=Sat)                                                               # dsr_sat_accumulate(1) on the same slots
    for first, n in ((0, S), (S, 2)):
        for k in range(n):
            _fill(h, p, case["path"], ci, k, first + k, keep, full=False)                          # counts only
            _transforms(two, p, case["path"], ci, k, first + k, keep); two.set_stats(k, c=p.num[first + k] - p.den[first + k], sumO=p.sumO[first + k], sumOsq=p.sumOsq[first + k])
        if first == 0:
            with pytest.raises(DsrError) as e:
                h.norm(n)                                                                         # the fold needs sumO and sumOsq
            assert e.value.status == dsr.E_CONSISTENCY and "counts only" in str(e.value)
        h.accumulate(n); two.accumulate(SAT_MEAN, n)
    mat, vec, scalar, occ, has = h.sat.mean_accus(); varVec = h.sat.var_accus()[0]
    ld = Fc.sums(p, fast, N.LD); ref = Fc.sums(p, fast)
    n = (S + 2) * (p.D // p.nB); err = np.abs(mat.astype(N.LD) - ld.a.mat).astype(f64); bound = (n + 3) * U * ld.a.bmat
    frac = float((err / np.where(bound > 0, bound, 1.0)).max()); _worst["mat"] = max(_worst["mat"], frac)
    print("fsat mat case %d: largest fraction of the bound %.4f (n = %d); so far %.4f" % (mi, frac, n, _worst["mat"]))
    assert (err <= bound).all(), frac
    assert np.array_equal(_bits(occ), _bits(ref.a.occ)) and has.all() and np.array_equal(mat, np.swapaxes(mat, 2, 3))
    m2, v2, s2, o2, h2 = two.mean_accus()
    assert np.array_equal(_bits(mat), _bits(m2)) and np.array_equal(_bits(occ), _bits(o2))         # the same kernel without its vec columns
    assert _same(vec.reshape(p.G, p.D), fast.fastMean) and _same(scalar, fast.scalar) and _same(varVec, fast.fastVar)   # what add_fast put there
    assert np.abs(v2).max() > 0 and not np.array_equal(v2, vec)


# ---- 3. the solve and the update --------------------------------------------------------------------------------------------------------------------
def _eta(G, w, z):
    return np.linalg.norm(G @ w - z) / (np.linalg.norm(G, 2) * np.linalg.norm(w) + np.linalg.norm(z))


def _device_sums(h):
    mat, vec, scalar, occ, has = h.sat.mean_accus()
    return dict(mat=mat, vec=vec, scalar=scalar, occ=occ, has=has, varVec=h.sat.var_accus()[0])


def _prepared(dsr, q, mass=Fc.MASS, meanOnly=False):
    """a handle whose sums were made on the device from the problem's speakers: norm, add_fast, matrix-only accumulate"""
    p = q["p"]; h = _make(dsr, p, p.S, q["thr"], mass, meanOnly=meanOnly); keep = []
    for s in range(p.S):
        _fill(h, p, "raw", 0, s, s, keep)
    h.norm(p.S); h.add_fast(); h.accumulate(p.S); h.set_desc_len(q["descLen"])
    return h


def _check_update(h, d, want, r, before, cvBefore, thr, bl):
    """records, counters, auxiliary values, variances and means of an update against the restatement on the device's sums"""
    kept, dec, aO, aN, dl = h.records(); x = h.solution(); after = h.gmm.params()
    assert np.array_equal(dec, want["decision"]) and np.array_equal(kept, want["kept"]), (dec.tolist(), want["decision"].tolist())
    assert np.array_equal(h.get_desc_len(), want["descLen"]) and np.array_equal(dl, want["descLen"]) and h.desc_length() == F.desc_length(want["descLen"])
    assert r["info"] == want["info"] and r["totals"] == want["totals"]
    G, nB = dec.shape; aux = 0.0
    for g in range(G):
        for nb in range(nB):
            if dec[g, nb] in (F.UPDATED, F.KEPT_OLD):
                aux += aN[g, nb] if dec[g, nb] == F.UPDATED else aO[g, nb]
                M, v, sc = d["mat"][g, nb], d["vec"][g, nb], float(d["scalar"][g, nb]); xd = x[g, nb * bl:(nb + 1) * bl]
                for got, at, pen in ((aO[g, nb], before[g, nb * bl:(nb + 1) * bl].astype(f64), thr * want["descLenBefore"][g, nb]), (aN[g, nb], xd, thr * kept[g, nb])):
                    mag = 0.5 * (np.abs(at) @ np.abs(M) @ np.abs(at) + abs(sc)) + np.abs(at) @ np.abs(v) + abs(pen)
                    assert abs(got - (N.aux_func(M, v, sc, at) + pen)) <= 2 * (bl * bl + 2 * bl + 4) * U * mag, (g, nb)
                if dec[g, nb] == F.UPDATED:
                    assert np.array_equal(_bits(after["mean"][g, nb * bl:(nb + 1) * bl]), _bits(xd.astype(f32)))          # each component stored as float(q)
                else:
                    assert np.array_equal(_bits(after["mean"][g, nb * bl:(nb + 1) * bl]), _bits(before[g, nb * bl:(nb + 1) * bl]))
    assert _bits(np.array([r["aux"]]))[0] == _bits(np.array([aux]))[0]                            # the model-order sum of the device's values
    assert np.array_equal(_bits(after["cv"]), _bits(want["cv"]))
    return kept, dec, x


@pytest.mark.parametrize("si", range(len(Fc.SOLVE_CASES)))
def test_update_decisions_description_lengths_variances_and_solve(dsr, cuda, si):
    case = Fc.SOLVE_CASES[si]; q = Fc.solve_problem(si); p = q["p"]; thr = q["thr"]; bl = p.D // p.nB; h = _prepared(dsr, q)
    d = _device_sums(h); before = h.gmm.params()["mean"].copy(); cvBefore = h.gmm.params()["cv"].copy()
    want = F.update(d["mat"], d["vec"], d["scalar"], d["occ"], d["has"], d["varVec"], before, cvBefore, q["descLen"], thr, Fc.MASS)
    want["descLenBefore"] = q["descLen"]
    r = h.update(); kept, dec, x = _check_update(h, d, want, r, before, cvBefore, thr, bl)
    assert np.array_equal(_bits(h.gmm.params()["cv"]), _bits((d["varVec"] / d["occ"][:, None]).astype(f32)))               # float(varVec / occ)
    worst = 0.0
    for g in range(p.G):
        for nb in range(p.nB):
            M, v = d["mat"][g, nb], d["vec"][g, nb]; xd = x[g, nb * bl:(nb + 1) * bl]; s = want["solves"][(g, nb)]
            if kept[g, nb] == bl:
                xn = N.solve(M, v)[0]; ed, en = _eta(M, xd, v), _eta(M, xn, v)
                assert ed <= 8 * max(en, U), (g, nb, ed, en)
                worst = max(worst, ed / max(en, U))
            elif kept[g, nb] == 0:
                assert not xd.any()
            else:
                lam, keep = s["lam"], s["keep"]; gap = min(abs(a - b) for a in lam[keep] for b in lam[~keep]); lmin = np.abs(lam[keep]).min(); lmax = np.abs(lam).max()
                allow = 8 * bl * U * (lmax / gap + lmax / lmin) * np.linalg.norm(v) / lmin
                assert np.linalg.norm(xd - s["x"]) <= allow, (g, nb, np.linalg.norm(xd - s["x"]), allow)
    _worst["eta"] = max(_worst["eta"], worst)
    print("fsat solve case %s: largest backward error %.2f x LAPACK's; so far %.2f" % (case["name"], worst, _worst["eta"]))
    if case["thr"] == 0.0:
        assert (dec == F.UPDATED).all() and (kept == bl).all()
    if case["thr"] == "all":
        assert (kept == 0).all()
    if case["thr"] == "some":
        assert (kept < bl).any() and (kept > 0).any()
    if case["name"] == "second1":
        assert (dec == F.KEPT_OLD).all() and (h.get_desc_len() == 1).all()
    if case["name"] == "secondbl":
        assert (dec == F.UPDATED).all()                                                           # the same sums as second1: the penalty changed the decision


@pytest.mark.parametrize("meanOnly", [False, True])
def test_thresholds_zero_occupancy_keep_old_mean_only_and_a_flagged_gaussian(dsr, cuda, meanOnly):
    q = Fc.branch_problem(); p = q["p"]
    for mass, left0 in ((-1.0, False), (0.0, True)):
        h = _prepared(dsr, q, mass, meanOnly)
        fa = h.get_fast(); h.zero(); fa["fastMean"][4, 1] = np.inf                                # Gaussian 4: a statistic that is not finite
        h.set_fast(fa["count"], fa["den"], fa["fastMean"], fa["fastVar"], fa["scalar"]); h.add_fast(); h.accumulate(p.S)
        d = _device_sums(h); before = h.gmm.params()["mean"].copy(); cvBefore = h.gmm.params()["cv"].copy()
        assert d["occ"].tolist() == [7.0, 0.0, 0.0, 15.0, 29.0, 29.0] and d["has"].all()
        want = F.update(d["mat"], d["vec"], d["scalar"], d["occ"], d["has"], d["varVec"], before, cvBefore, q["descLen"], 0.0, mass, meanOnly, skip={4})
        want["descLenBefore"] = q["descLen"]
        with pytest.raises(DsrError) as e:
            h.update()
        assert e.value.status == dsr.E_CONSISTENCY and h.gaussian_status(4) == dsr.E_CONSISTENCY and [h.gaussian_status(g) for g in (0, 1, 2, 3, 5)] == [0] * 5
        kept, dec, x = _check_update(h, d, want, h.last, before, cvBefore, 0.0, p.D)
        assert dec[:, 0].tolist() == ([F.LEFT, F.LEFT, F.LEFT, F.KEPT_OLD, F.FLAGGED, F.UPDATED] if left0 else [F.UPDATED, F.ZEROED, F.ZEROED, F.KEPT_OLD, F.FLAGGED, F.UPDATED])
        after = h.gmm.params(); inv = (1.0 / cvBefore.astype(f64)).astype(f32)
        assert np.array_equal(_bits(after["mean"][4]), _bits(before[4])) and np.array_equal(_bits(after["cv"][4]), _bits(inv[4]))      # flagged: 1 / var
        assert h.last["totals"] == [6, 3 if left0 else 6] and h.get_desc_len()[:, 0].tolist() == ([1, 1, 1, 1, 1, 3] if left0 else [3, 1, 1, 1, 1, 3])
        if left0:
            assert np.array_equal(_bits(after["cv"][:3]), _bits(inv[:3])) and np.array_equal(_bits(after["mean"][:3]), _bits(before[:3]))   # below the mass threshold
        else:
            assert not after["mean"][1].any() and not after["mean"][2].any()                      # occ == 0: the mean zeroed
            assert np.array_equal(_bits(after["cv"][2]), _bits(inv[2]))                           # varVec / occ = 0 / 0: a NaN keeps 1 / var
        if meanOnly:
            assert np.array_equal(_bits(after["cv"]), _bits(inv))
        else:
            assert np.array_equal(_bits(after["cv"][5]), _bits((d["varVec"][5] / 29.0).astype(f32)))


# ---- 4. end to end: the fast path against the two-pass path ---------------------------------------------------------------------------------------
def _speaker_files(dsr, p, tmp_path, labels, fastHandle=None):
    """<tmp>/accu_<label>.cbs.accu (full), <tmp>/cnt_<label>.cbs.accu (counts only) and <tmp>/par_<label>; with fastHandle the training pass of the
    fast path as well: the trainer's accumulators of each speaker folded into its fast accumulators (set_stats, set_tree, norm), then zeroed"""
    g = dsr.Gmm(**p.m.as_kwargs()); g.set_reg_classes(p.classes); tr = dsr.Trainer(g) if fastHandle is None else fastHandle.trainer
    ml = dsr.Mllr(g, 1); pr, tt = [], []
    for s, lab in enumerate(labels):
        tr.zero(); tr.set(count=p.c[s], den=np.zeros(p.G), sumO=p.sumO[s], sumOsq=p.sumOsq[s])
        pr.append(f32(-1234.5 * (s + 1))); tt.append(100 + 7 * s)
        tr.save_codebook_accus(str(tmp_path / ("accu_%s.cbs.accu" % lab)), float(pr[-1]), tt[-1])
        tr.save_codebook_accus(str(tmp_path / ("cnt_%s.cbs.accu" % lab)), float(pr[-1]), tt[-1], True)
        t = ml.tree(0); t.clear()
        for rc, x in p.xf[s].items():
            t.set(rc, np.concatenate([x.A[0], x.b[:, None]], axis=1))
        ml.write(0, str(tmp_path / ("par_%s" % lab)))
        if fastHandle is not None:
            fastHandle.set_stats(0, trainer=tr); fastHandle.set_tree(0, ParamTree(str(tmp_path / ("par_%s" % lab)))); fastHandle.norm(1)
        tr.zero()
    (tmp_path / "spk.txt").write_text("".join(l + "\n" for l in labels))
    return pr, tt


def _e2e_problem():
    """the statistics are floats, as an accumulator file holds them: the two-pass path reads them from the full files, the fast path folds them
    from the trainer, and both see the same numbers"""
    p = Cs.Problem(13, 1, [2, 3], [20, 13], 3, seed=77, refN=[10, 10, 13])
    p.sumO = [a.astype(f32).astype(f64) for a in p.sumO]; p.sumOsq = [a.astype(f32).astype(f64) for a in p.sumOsq]
    return p


def test_fast_path_against_the_two_pass_path(dsr, cuda, tmp_path):
    """see the module docstring, End to end, for the algebra"""
    labels = ["spkA", "B02", "c"]; p = _e2e_problem(); pre = str(tmp_path) + "/"
    train = _make(dsr, p, 1); pr, tt = _speaker_files(dsr, p, tmp_path, labels, train); train.save_fast(pre + "fast.accu")
    assert not train.trainer.get()["count"].any() and train.fast_blocks() == 1
    # the two passes, each from the starting model on the full files
    a = _make(dsr, p, 3, cls=Sat); ret2 = a.estimate_files(SAT_MEAN, pre + "spk.txt", pre + "par_", pre + "accu_"); mean2 = a.gmm.params()["mean"]
    b = _make(dsr, p, 3, cls=Sat); b.estimate_files(SAT_VARIANCE, pre + "spk.txt", pre + "par_", pre + "accu_"); cv2 = b.gmm.params()["cv"]
    # in memory: the accumulators handed over in double
    mem = _make(dsr, p, 2); fa = train.get_fast(); mem.set_fast(fa["count"], fa["den"], fa["fastMean"], fa["fastVar"], fa["scalar"])
    retM = mem.estimate_files(pre + "spk.txt", pre + "par_", pre + "cnt_"); qm = mem.gmm.params()
    want = F.estimate_return(0.0, p.G, pr, tt)
    assert retM == want == ret2 == N.estimate_return(pr, tt)                                      # thr = 0: the description length adds nothing
    assert (np.abs(qm["mean"].astype(f64) - mean2.astype(f64)) <= 2.0 ** -23 * np.abs(mean2.astype(f64)) + 1e-10).all()
    assert np.array_equal(_bits(qm["cv"]), _bits(cv2))
    assert (mem.records()[1] == F.UPDATED).all() and not mem.trainer.get()["count"].any()         # the model accumulators are zeroed (sat:1833)
    # through the file, on a fresh handle, with counts-only speaker files: equal to in memory with the accumulators rounded to float
    fil = _make(dsr, p, 3); fil.load_fast(pre + "fast.accu"); retF = fil.estimate_files(pre + "spk.txt", pre + "par_", pre + "cnt_"); qf = fil.gmm.params()
    rnd = _make(dsr, p, 3); rnd.set_fast(*[fa[k].astype(f32).astype(f64) for k in ("count", "den", "fastMean", "fastVar", "scalar")])
    rnd.estimate_files(pre + "spk.txt", pre + "par_", pre + "accu_"); qr = rnd.gmm.params()       # full speaker files serve as well: only the counts are read
    assert retF == want and np.array_equal(_bits(qf["mean"]), _bits(qr["mean"])) and np.array_equal(_bits(qf["cv"]), _bits(qr["cv"]))
    # the file rounds vec to float: |dx| <= cond(M) 2^-24 sqrt(D) |x| per Gaussian, cond(M) <= 25 on the recipe (test_fsat_np_cpu.py), and the float store
    dx = np.linalg.norm(qf["mean"].astype(f64) - mean2.astype(f64), axis=1); nx = np.linalg.norm(mean2.astype(f64), axis=1)
    assert (dx <= (25 * 2.0 ** -24 * np.sqrt(p.D) + 2.0 ** -23) * nx + 1e-10).all()
    assert (np.abs(qf["cv"].astype(f64) - cv2.astype(f64)) <= 2.0 ** -22 * np.abs(cv2.astype(f64))).all()
    assert not np.array_equal(qf["mean"], p.m.mean) and not np.array_equal(qf["cv"], p.m.cv)


def test_estimate_return_adds_the_description_length_and_the_facade_returns_it(dsr, cuda, tmp_path):
    from dsr.asr.sat import CodebookSetFastSATPtr, FastMeanVarianceSATPtr, SpeakerListPtr
    labels = ["s1", "s2", "s3"]; p = Cs.Problem(5, 1, [2, 3], [6, 6], 3, seed=79, refN=[3, 3, 3, 3]); pre = str(tmp_path) + "/"; thr = 0.25
    train = _make(dsr, p, 1); pr, tt = _speaker_files(dsr, p, tmp_path, labels, train); train.save_fast(pre + "fast.accu")
    h = _make(dsr, p, 3, thr); h.load_fast(pre + "fast.accu")
    assert h.desc_length() == p.G
    ret = h.estimate_files(pre + "spk.txt", pre + "par_", pre + "cnt_"); wantMean = h.gmm.params()["mean"]; dl = h.get_desc_len()
    assert ret == F.estimate_return(thr, p.G, pr, tt) != N.estimate_return(pr, tt) and h.desc_length() == int(dl.sum())

    class Cbs(CodebookSetFastSATPtr):                                                             # a codebook set over a trainer made by hand
        def __init__(self, tr):
            CodebookSetFastSATPtr.__init__(self); self._trainer = tr; self._gmm = tr.gmm
    g = dsr.Gmm(**p.m.as_kwargs()); g.set_reg_classes(p.classes); cbs = Cbs(dsr.Trainer(g))
    cbs.loadFastAccus(pre + "fast.accu"); assert cbs.descLength() == p.G
    sat = FastMeanVarianceSATPtr(cbs, 0, thr, 1.0, slots=2)
    assert sat.estimate(SpeakerListPtr(pre + "spk.txt"), pre + "par_", pre + "cnt_") == ret
    assert np.array_equal(_bits(g.params()["mean"]), _bits(wantMean)) and cbs.descLength() == int(dl.sum())      # the lengths go back to the set
    with pytest.raises(DsrError) as e:
        cbs.normFastAccus(ParamTree(pre + "par_s1"), olen=7)
    assert e.value.status == dsr.E_DIMENSION
    cbs.zeroFastAccus(); tr = cbs._need(); tr.set(count=p.c[0], den=np.zeros(p.G), sumO=p.sumO[0], sumOsq=p.sumOsq[0])
    cbs.normFastAccus(ParamTree(pre + "par_s1")); got = cbs._fast().get_fast()                      # zeroed, then one speaker folded
    for args, status in (((cbs, 7), dsr.E_DIMENSION), ((cbs, 0, 0.1, 10.0, 1, 1, 2.0), dsr.E_PARAMETER), ((cbs, 0, 0.1, 10.0, 1, 1, 1.0, False, 2), dsr.E_PARAMETER)):
        with pytest.raises(DsrError) as e:
            FastMeanVarianceSATPtr(*args)
        assert e.value.status == status
    assert got["count"].tolist() == p.c[0].tolist()


def test_updated_model_scores_and_saves_as_a_model_built_from_its_parameters(dsr, cuda, tmp_path):
    import torch
    q = Fc.solve_problem(3); p = q["p"]; h = _prepared(dsr, q); tr = h.trainer; q0 = h.gmm.params(); d = _device_sums(h)
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((40, p.D)).astype(f32)).to(cuda)
    before = [h.gmm.score(x, mode)[0].cpu().numpy() for mode in (0, 1, 2)]                       # every mode has its device image built
    want = F.update(d["mat"], d["vec"], d["scalar"], d["occ"], d["has"], d["varVec"], q0["mean"], q0["cv"], q["descLen"], q["thr"], Fc.MASS)
    h.update(); kw = p.m.as_kwargs(); kw["mean"] = want["mean"]; kw["ivar"] = want["cv"]; other = dsr.Gmm(**kw)
    tr.invert_variances(); tr.fix_gconsts(); t2 = dsr.Trainer(other); t2.invert_variances(); t2.fix_gconsts()
    got = h.gmm.params()
    assert np.array_equal(_bits(got["mean"]), _bits(other.params()["mean"])) and np.array_equal(_bits(got["cv"]), _bits(other.params()["cv"]))
    for mode in (0, 1, 2):
        a = h.gmm.score(x, mode)[0].cpu().numpy(); b = other.score(x, mode)[0].cpu().numpy()
        assert np.array_equal(a, b) and not np.array_equal(a, before[mode]), mode
    cb, ds = str(tmp_path / "m.cb"), str(tmp_path / "m.ds"); h.gmm.save(cb, ds)
    back = dsr.Gmm(files=(cb, ds)).params()
    assert np.array_equal(_bits(back["mean"]), _bits(got["mean"])) and np.array_equal(_bits(back["cv"]), _bits(got["cv"]))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dsr, cuda):
    D = 4; p = Fc.with_counts(Cs.Problem(D, 1, [2, 3], [3, 2], 2, seed=3), 4, special=False); h = _make(dsr, p, 2)

    def fill(s, classes, nB=1, full=True):
        h.clear_slot(s)
        for rc in classes:
            h.set_transform(s, rc, N.APT if nB > 1 else N.MLLR, np.stack([np.eye(D // nB)] * nB), np.zeros(D))
        if full:
            h.set_stats(s, count=p.num[s], den=p.den[s], sumO=p.sumO[s], sumOsq=p.sumOsq[s])
        else:
            h.set_counts(s, count=p.num[s], den=p.den[s])
    for call in (lambda: h.norm(1), lambda: h.accumulate(1)):
        fill(0, [2])
        with pytest.raises(DsrError) as e:
            call()
        assert e.value.status == dsr.E_KEY and "Could not find node 3" in str(e.value)            # a missing class
        fill(0, [2, 3, 6])
        with pytest.raises(DsrError) as e:
            call()
        assert e.value.status == dsr.E_CONSISTENCY and "not a leaf" in str(e.value)               # class 3 has a child: subN > 1 is RegClassAcc's
    assert h.fast_blocks() == 0 and h.sat.num_blocks() == 0                                       # nothing was accumulated
    for call, status in ((lambda: h.get_fast(), dsr.E_CONSISTENCY), (lambda: h.add_fast(), dsr.E_CONSISTENCY), (lambda: h.save_fast("/nonexistent/x"), dsr.E_CONSISTENCY),
                         (lambda: h.norm(3), dsr.E_INDEX), (lambda: h.set_counts(2, count=np.zeros(p.G)), dsr.E_INDEX)):
        with pytest.raises(DsrError) as e:
            call()
        assert e.value.status == status
    fill(0, [2, 3]); fill(1, [2, 3], nB=2)
    with pytest.raises(DsrError) as e:
        h.norm(2)
    assert e.value.status == dsr.E_DIMENSION                                                      # transforms of different block counts
    h.norm(1); assert h.fast_blocks() == 1
    fill(0, [2, 3], nB=2)
    with pytest.raises(DsrError) as e:
        h.norm(1)                                                                                 # another block count than the accumulators'
    assert e.value.status == dsr.E_DIMENSION and h.fast_blocks() == 1
    with pytest.raises(DsrError) as e:
        h.save_fast("/nonexistent/dir/fast.accu")
    assert e.value.status == dsr.E_IO
    big = Cs.Problem(82, 1, [1], [2], 1, seed=1); hb = _make(dsr, big, 1)
    with pytest.raises(DsrError) as e:
        hb.set_transform(0, 1, N.MLLR, np.eye(82))
    assert e.value.status == dsr.E_DIMENSION and "at most 81" in str(e.value)                     # bl > 81
    with pytest.raises(DsrError) as e:
        hb.set_fast(np.zeros(2), np.zeros(2), np.zeros((2, 82)), np.zeros((2, 82)), np.zeros((2, 1)))
    assert e.value.status == dsr.E_DIMENSION
    with pytest.raises(DsrError) as e:
        FastSat(h.trainer, 1, float("nan"))
    assert e.value.status == dsr.E_PARAMETER
    with pytest.raises(DsrError) as e:
        dsr.sat_check(39, 39, 0.5, 0)                                                             # section 14 keeps refusing a likelihood threshold
    assert e.value.status == dsr.E_PARAMETER
