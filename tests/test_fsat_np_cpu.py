"""CPU tests of fast speaker-adaptive training: the numpy restatement (tests/fsat_np.py) against planted models and against tests/sat_np.py,
the fast-accumulator file, the refusals of include/dsr.h section 14b that need no device, the façade names, and the input conditions under
which tests/test_gpu_fsat.py compares decisions.  A dsr_fsat is created over a trainer, which needs a device: the rest is in test_gpu_fsat.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import fsat_cases as Fc
from tests import fsat_np as F
from tests import sat_cases as Cs
from tests import sat_np as N
from tests.conftest import PKG

f32, f64 = np.float32, np.float64
U = 2.0 ** -53


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _plain(D, nB, S, seed, kind=N.MLLR):
    p = Cs.Problem(D, nB, [2, 3], [4, 3], S, seed=seed, kind=kind); p.num = [c.copy() for c in p.c]; p.den = [np.zeros(p.G) for _ in p.c]
    return p


@pytest.mark.parametrize("D,nB,S", [(1, 1, 1), (3, 1, 3), (13, 1, 3), (39, 3, 3), (40, 2, 1)])
def test_restatement_recovers_planted_means_and_variances(D, nB, S):
    """The full-rank recipe: sumO = c (A mu* + b), sumOsq = c (sigma^2 + (A mu* + b)^2).  With thr = 0 the MDL solve is the plain one, so the mean
    is mu* to a float ulp + 1e-10; with the model AT mu*, fastVar / occ = sigma^2 up to the float store, what the float transform leaves
    (sum c (trn - y)^2 / occ) and the roundings of 4 S terms -- the bound tests/test_gpu_sat.py allows the two-pass variance"""
    kind = N.APT if nB > 1 else N.MLLR
    p = _plain(D, nB, S, 40 + D, kind); a = Fc.sums(p, Fc.fold(p))
    r = F.update(a.a.mat, a.a.vec, a.a.scalar, a.a.occ, a.a.has, a.varVec, p.m.mean, p.m.cv, np.ones((p.G, nB)), 0.0, 1.0)
    assert (r["decision"] == F.UPDATED).all() and (r["kept"] == D // nB).all() and r["totals"] == [p.G, p.G]
    assert r["info"] == [p.G * nB, p.G * nB, p.G * D, p.G * D] and F.desc_length(r["descLen"]) == p.G * D
    assert (np.abs(r["mean"].astype(f64) - p.muStar) <= 2.0 ** -23 * np.abs(p.muStar) + 1e-10).all()
    p = _plain(D, nB, S, 40 + D, kind); p.m.mean = p.muStar.astype(f32); fast = Fc.fold(p); a = Fc.sums(p, fast); va = N.VarAccus(p.G, p.D)
    for s in range(S):
        va.accumulate(p.classes, p.m.mean, p.c[s], p.sumO[s], p.sumOsq[s], p.xf[s], exact=p.y[s])
    assert np.array_equal(_bits(fast.fastVar), _bits(va.vec)) and np.array_equal(_bits(a.a.occ), _bits(va.occ))     # float counts: ck is c_k
    r = F.update(a.a.mat, a.a.vec, a.a.scalar, a.a.occ, a.a.has, a.varVec, p.m.mean, p.m.cv, np.ones((p.G, nB)), 0.0, 1.0)
    assert np.array_equal(_bits(r["cv"]), _bits((a.varVec / a.a.occ[:, None]).astype(f32)))
    tol = 2.0 ** -23 * p.sigma2 + (va.model + 4 * S * U * va.bound) / va.occ[:, None]
    assert (np.abs(r["cv"].astype(f64) - p.sigma2) <= tol).all()
    m = F.update(a.a.mat, a.a.vec, a.a.scalar, a.a.occ, a.a.has, a.varVec, p.m.mean, p.m.cv, np.ones((p.G, nB)), 0.0, 1.0, meanOnly=True)
    assert np.array_equal(_bits(m["cv"]), _bits((1.0 / p.m.cv.astype(f64)).astype(f32))) and np.array_equal(_bits(m["mean"]), _bits(r["mean"]))


def test_mdl_solve_at_threshold_zero_is_the_pseudo_inverse_solve():
    """a positive-definite matrix has l_k > 0 and 0.5 t_k^2 / l_k > 0 for every t_k != 0: with thr = 0 every direction whose ratio passes is
    kept, which is SATMean::_solve.  Both are backward stable at cond <= 25: they agree to 1e-10 (1 + |x|)"""
    for D, S in ((3, 1), (13, 3), (39, 3)):
        p = _plain(D, 1, S, 60 + D); a = Fc.sums(p, Fc.fold(p))
        for g in range(p.G):
            M, v = a.a.mat[g, 0], a.a.vec[g, 0]; s = F.mdl_solve(M, v, 0.0); x, k, sv = N.solve(M, v)
            assert s["kept"] == k == D and (s["lam"] > 0).all() and sv[-1] / sv[0] >= 0.04
            assert np.linalg.norm(s["x"] - x) <= 1e-10 * (1 + np.linalg.norm(x))
    s = F.mdl_solve(np.diag([4.0, 1.0, -1.0]), np.array([2.0, 1.0, 1.0]), 0.4)                     # contrib 0.5, 0.5, -0.5; ratio 1, 0.25, -0.25
    assert s["keep"].tolist() == [False, True, True] and np.allclose(s["x"], [0.5, 1.0, 0.0])     # eigh sorts ascending: the negative direction is dropped
    assert F.mdl_solve(np.diag([4.0, 1.0]), np.array([2.0, 1.0]), 0.5)["kept"] == 0               # contrib == thr is not kept (sat:483)
    assert F.mdl_solve(-np.eye(2), np.ones(2), 0.0)["kept"] == 0                                  # largestValue stays 0.0: every ratio fails


def test_fast_accumulator_file_round_trip_and_addition():
    p = Fc.norm_problem(1); fast = Fc.fold(p); refN = [10, 10, 11]; names = ["cbB", "cbA", "cbC"]; assert sum(refN) == p.G
    fast.count[10:20] = 0.0; fast.den[10:20] = 0.0                                                # codebook cbA has no occupancy: not in the file
    data = F.save_fast(fast, refN, names)
    dirLen = sum(2 + len(n) + 1 + 4 for n in ("cbB", "cbC")) + 2 + len(F.END_OF_ACCS) + 1
    assert len(data) == dirLen + F.record_size("cbB", 10, p.D, 1) + F.record_size("cbC", 11, p.D, 1)
    assert data[:7] == b"\x00\x03cbB\x00\x00" and data[dirLen - 20:dirLen] == b"\x00\x11EndOfAccumulators\x00"
    one = F.load_fast(data, None, refN, names, p.D)
    live = np.r_[0:10, 20:31]
    for k in ("count", "den", "fastMean", "fastVar", "scalar"):
        want = getattr(fast, k).astype(f32).astype(f64)                                           # the file holds floats
        assert np.array_equal(getattr(one, k)[live], want[live]) and not getattr(one, k)[10:20].any(), k
    two = F.load_fast(data, one, refN, names, p.D)
    for k in ("count", "den", "fastMean", "fastVar", "scalar"):
        assert np.array_equal(getattr(two, k), 2.0 * getattr(one, k)), k                          # load ADDS
    part = F.load_fast(data, None, refN, names, p.D, ks=[2])
    assert not part.count[:20].any() and np.array_equal(part.fastMean[20:], one.fastMean[20:])
    with pytest.raises(F.IOError_):
        F.load_fast(data[:-3], None, refN, names, p.D)
    with pytest.raises(F.DimensionError):
        F.load_fast(data, None, refN, names, p.D + 1)
    with pytest.raises(F.DimensionError):
        F.load_fast(data, F.FastAccus(p.G, p.D, 3), refN, names, p.D)                             # another nblks
    bad = bytearray(data); bad[-1] ^= 1
    with pytest.raises(F.IOError_):
        F.load_fast(bytes(bad), None, refN, names, p.D)                                           # the marker
    assert F.estimate_return(0.5, 7, [f32(-10.5), f32(-20.25)], [100, 200]) == (3.5 - 30.75) / 300


def test_norm_restatement_special_counts():
    p = Fc.norm_problem(1); fast = Fc.fold(p, [0]); G = p.G
    assert fast.count[0] == 0.0 and not fast.fastMean[0].any() and not fast.fastVar[0].any()                     # no count at all
    assert fast.count[-1] == 5.0 and fast.den[-1] == 5.0 - 2.0 ** -22 and not fast.fastMean[-1].any() and not fast.scalar[-1].any()   # |ck| < 1e-6
    assert fast.count[G // 2] == 1.0 and fast.den[G // 2] == 9.0 and fast.fastMean[G // 2].any() and fast.scalar[G // 2, 0] < 0   # ck = -8
    both = Fc.fold(p, [1], Fc.fold(p, [0])); assert np.array_equal(_bits(both.fastMean), _bits(Fc.fold(p, [0, 1]).fastMean))


def test_refusals_that_need_no_device(dsr):
    L = dsr.load()
    dsr.fsat_check(0, 39); dsr.fsat_check(39, 39, 0.0, 1.0, True, 1)
    for args, status in (((42, 39), dsr.E_DIMENSION), ((39, 39, 10.0, 2.0), dsr.E_PARAMETER), ((39, 39, 10.0, 1.0, False, 2), dsr.E_PARAMETER),
                         ((39, 39, 10.0, 1.0, False, 0), dsr.E_PARAMETER)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.fsat_check(*args)
        assert e.value.status == status, args
    h = C.c_void_p()
    assert L.dsr_fsat_create(None, 1, 0.0, 0.0, 1, 1, 0, C.byref(h)) == dsr.E_PARAMETER and not h.value
    for call in (lambda: L.dsr_fsat_norm(None, 1, None), lambda: L.dsr_fsat_accumulate(None, 1, None), lambda: L.dsr_fsat_update(None, None, None, None),
                 lambda: L.dsr_fsat_add_fast(None), lambda: L.dsr_fsat_zero(None), lambda: L.dsr_fsat_zero_fast(None), lambda: L.dsr_fsat_save_fast(None, b"x"),
                 lambda: L.dsr_fsat_load_fast(None, b"x", 1, 1), lambda: L.dsr_fsat_desc_length(None, None), lambda: L.dsr_fsat_set_counts(None, 0, None),
                 lambda: L.dsr_fsat_estimate_files(None, b"a", b"b", b"c", None), lambda: L.dsr_fsat_get_fast(None, None, None, None, None, None)):
        assert call() == dsr.E_PARAMETER
    assert L.dsr_fsat_fast_blocks(None) == 0 and L.dsr_fsat_desc_blocks(None) == 0 and not L.dsr_fsat_sat(None)
    L.dsr_fsat_destroy(None)
    import dsr._capi as K
    assert K.FastSat.__module__ == "dsr._fsat"
    dsr.sat_check(39, 39)                                                                         # section 14 keeps its own refusals
    with pytest.raises(dsr.DsrError) as e:
        dsr.sat_check(39, 39, 0.5, 0)
    assert e.value.status == dsr.E_PARAMETER


def test_stubs_raise_and_facade_names(dsr):
    from dsr.asr import sat as S
    for name in ("FastRegClassSATPtr", "FastMaxMutualInfoSATPtr", "FastMMIRegClassSATPtr"):
        with pytest.raises(dsr.DsrError) as e:
            getattr(S, name)(None)
        assert e.value.status == dsr.E_PARAMETER and "not built" in str(e.value) and name in str(e.value)
    import inspect
    sig = inspect.signature(S.FastMeanVarianceSATPtr.__init__); d = {k: v.default for k, v in sig.parameters.items()}
    assert list(sig.parameters)[1:10] == ["cbs", "meanLen", "lhoodThreshhold", "massThreshhold", "nParts", "part", "mmiMultiplier", "meanOnly", "maxNoRegClass"]
    assert (d["meanLen"], d["lhoodThreshhold"], d["massThreshhold"], d["nParts"], d["part"], d["mmiMultiplier"], d["meanOnly"], d["maxNoRegClass"]) == (0, 0.1, 10.0, 1, 1, 1.0, False, 1)
    for m in ("normFastAccus", "saveFastAccus", "loadFastAccus", "zeroFastAccus", "descLength", "setRegClassesToOne", "saveAccus", "zeroAccus"):
        assert callable(getattr(S.CodebookSetFastSATPtr, m))
    from dsr.asr.train import CodebookSetTrainPtr
    assert issubclass(S.CodebookSetFastSATPtr, CodebookSetTrainPtr)
    cbs = S.CodebookSetFastSATPtr()
    with pytest.raises(dsr.DsrError) as e:
        cbs.descLength()                                                                          # no accumulators allocated yet
    assert e.value.status == dsr.E_CONSISTENCY


def test_cpp_facade_names_compile(tmp_path):
    src = tmp_path / "f.cpp"
    src.write_text('#include "dsr_streams.hpp"\n#include <cstdio>\nint main() {\n'
                   '  CodebookSetFastSATPtr cbs(new CodebookSetFastSAT()); CodebookSetTrainPtr asTrain = cbs; FastMeanVarianceSATPtr f;\n'
                   '  try { cbs->descLength(); } catch (jconsistency_error& e) { printf("cons %d\\n", (int) e.getCode()); }\n'
                   '  try { FastMeanVarianceSAT s(cbs); } catch (jconsistency_error& e) { printf("cons %d\\n", (int) e.getCode()); }\n'
                   '  try { FastRegClassSAT r(cbs, 0, 0.1); } catch (jparameter_error& e) { printf("par %d\\n", (int) e.getCode()); }\n'
                   '  try { FastMaxMutualInfoSAT r(cbs); } catch (jparameter_error& e) { printf("par %d\\n", (int) e.getCode()); }\n'
                   '  try { FastMMIRegClassSAT r(cbs); } catch (jparameter_error& e) { printf("par %d\\n", (int) e.getCode()); }\n'
                   '  FastRegClassSATPtr a; FastMaxMutualInfoSATPtr b; FastMMIRegClassSATPtr c; return (f || a || b || c || !asTrain) ? 1 : 0; }\n')
    exe = tmp_path / "f"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split("\n")[:5] == ["cons 3", "cons 3", "par 12", "par 12", "par 12"], out.stdout + out.stderr


@pytest.mark.parametrize("si", range(len(Fc.SOLVE_CASES)))
def test_input_conditions_of_the_solve_cases(si):
    """what tests/test_gpu_fsat.py relies on when it compares the device's decisions with the restatement's: every 0.5 t^2 / l at least a
    relative 1e-6 from thr, every l / lmax a factor of 10 from 1e-7, eigenvalues across a kept / dropped boundary at least 1e-3 apart
    (relative), |auxOld - auxNew| at least 1e-9 of their magnitude"""
    q = Fc.solve_problem(si); case = Fc.SOLVE_CASES[si]; r = Fc.restated_update(q); c = F.conditions(r, q["thr"]); bl = case["D"] // case["nB"]
    print("fsat solve case %s: thr %.6g margins %s" % (case["name"], q["thr"], c))
    assert c["contrib"] >= 1e-6 and c["ratio"] >= 10.0 and c["gap"] >= 1e-3 and c["aux"] >= 1e-9
    kept = r["kept"]
    if case["thr"] == 0.0:
        assert (kept == bl).all() and (r["decision"] == F.UPDATED).all()
    elif case["thr"] == "all":
        assert (kept == 0).all()
    else:
        assert (kept < bl).any() and (kept > 0).any() and kept.min() < bl and 0 < kept.sum() < kept.size * bl       # some, not all
    if case["name"] == "second1":
        assert (r["decision"] == F.KEPT_OLD).all() and (r["descLen"] == 1).all()
    if case["name"] == "secondbl":
        assert (r["decision"] == F.UPDATED).all() and np.array_equal(r["descLen"], kept)          # the same sums: the penalty changed the decision


def test_input_conditions_of_the_branch_case():
    q = Fc.branch_problem(); a = q["sums"]
    assert a.a.occ.tolist() == [7.0, 0.0, 0.0, 15.0, 29.0, 29.0] and a.a.has.all()
    for mass, want in ((-1.0, [F.UPDATED, F.ZEROED, F.ZEROED, F.KEPT_OLD, F.FLAGGED, F.UPDATED]), (0.0, [F.LEFT, F.LEFT, F.LEFT, F.KEPT_OLD, F.FLAGGED, F.UPDATED])):
        r = Fc.restated_update(q, massThreshold=mass, skip={4}); c = F.conditions(r, 0.0)
        assert r["decision"][:, 0].tolist() == want and c["contrib"] >= 1e-6 and c["ratio"] >= 10.0 and c["aux"] >= 1e-9, (mass, c)
