"""CPU tests of STC and LDA estimation: the numpy restatement of asr/train/estimateAdapt.cc:2203-3036 and asr/adapt/transform.cc:1788-1984
(tests/stc_np.py) has the properties the two estimators must have and keeps the reference's file layouts and quirks, and the device's
estimation code (csrc/stc_rows.h), run on the host with one thread, agrees with it.  The Python faces are imported so that the module stands
and falls with them."""
import os
import struct

import numpy as np
import pytest

from dsr._capi import Lda, Stc                                              # noqa: F401  the bindings this restatement is the yardstick of
from dsr.asr.adapt import LDATransformerPtr, STCTransformerPtr              # noqa: F401
from dsr.asr.train import LDAEstimatorPtr, STCEstimatorPtr                  # noqa: F401
from tests import stc_np as S
from tests.conftest import PKG

f32 = np.float32


def _stc(D, T, seed, K=4, R=3, mmi=False, cascade=False, den=0):
    """a restatement fed with T numerator frames (and `den` denominator frames, factor -0.5)"""
    m, x, dist, Rot, lam = S.synth_stc(K, R, D, T + den, seed)
    s = S.Stc(m["refN"], m["mean"], m["ivar"], m["det"], cascade=cascade, mmi=mmi)
    s.accumulate(x[:T], x[:T], dist[:T], 1.0)
    if den:
        s.accumulate(x[T:], x[T:], dist[T:], -0.5)
    return s, m, x, dist, Rot, lam


@pytest.mark.parametrize("D,T,mmi", [(3, 150, False), (8, 400, False), (8, 400, True), (17, 850, False)])
def test_auxiliary_function_never_decreases(D, T, mmi):
    """Q(A) = 2 gamma log |det A| - sum_d a_d G_d a_d^T over every single row update, and from the identity to the end.  A row update
    maximises Q over that row, so a step is >= 0 up to the rounding of Q's own evaluation, allowed as 1e-11 |Q|."""
    s, *_ = _stc(D, T, seed=20 + D, mmi=mmi, den=T // 4 if mmi else 0)
    s.make_pos_def(); q = [s.aux(np.eye(D))]; steps = []

    def after_row(it, d, A):
        q.append(s.aux(A)); steps.append(q[-1] - q[-2])
    A = s.update(np.eye(D), after_row=after_row)
    assert len(steps) == S.MAX_ITNS * D and min(steps) >= -1e-11 * abs(q[-1]), min(steps)
    assert q[-1] > q[0] and np.isfinite(A).all()


@pytest.mark.parametrize("D", [3, 8, 17])
def test_estimate_decorrelates(D):
    """frames from Gaussians that share the rotated diagonal covariance Rot^T Lambda Rot, 50 a dimension: under the ML estimate A Sigma A^T is
    nearer to diagonal than Sigma itself (the off-diagonal share of the energy)"""
    s, m, x, dist, Rot, lam = _stc(D, 50 * D, seed=40 + D)
    A = s.estimate(); Sigma = Rot.T @ np.diag(lam) @ Rot
    before, after = S.offdiag_ratio(Sigma), S.offdiag_ratio(A @ Sigma @ A.T)
    print("D=%d: off-diagonal share %.4f -> %.4f" % (D, before, after))
    assert after < before
    assert np.allclose(s.Ainv @ s.A, np.eye(D), atol=1e-9)                    # _stcInv is refreshed (eA:2450-2453)


def test_make_pos_def_doubles_E_only_when_needed():
    D = 4; s, *_ = _stc(D, 200, seed=3, mmi=True, den=60)
    assert s.make_pos_def(1.0, 1.0) == 1.0                                  # numerator statistics alone are positive definite
    assert s.make_pos_def(0.25, 3.0) == 0.75                                # multE multiplies the E that was found
    # statistics built so that minE is too small: sumOsq[d] = -5 I + a small p.d. part, regSq[d] = I -> E must exceed 5: 1, 2, 4, 8
    t = S.Stc(s.refN, s.mean, s.ivar, s.det, mmi=True)
    t.sumOsq = np.stack([np.tril(-5.0 * np.eye(D) + 0.01 * (k + 1) * np.ones((D, D))) for k in range(D)]); t.regSq = np.stack([np.eye(D)] * D)
    assert t.make_pos_def(1.0, 1.0) == 8.0 and t.make_pos_def(1.0, 0.5) == 4.0
    t.regSq[:] = 0.0
    with pytest.raises(S.NumericError):
        t.make_pos_def(1.0, 1.0, cap=20)


def test_accumulation_places_the_roundings():
    """one frame by hand: wgt = float(iv float(1 x factor)), o = float(x - mu), (wgt o_i) o_j into the lower triangle; W(2) only for factor <= 0"""
    m = S.synth_model(2, 2, 3, 5); s = S.Stc(m["refN"], m["mean"], m["ivar"], m["det"])
    x = np.array([0.3, -1.7, 2.2], f32); g = s.accu_one(1, x, x, 0.37)
    o = (x - m["mean"][g]).astype(f32).astype(np.float64); w = (m["ivar"][g] * f32(0.37)).astype(f32).astype(np.float64)
    assert s.count == float(f32(0.37)) and s.denCount == 0.0 and not s.regSq.any()
    assert s.sumOsq[2, 1, 0] == (w[2] * o[1]) * o[0] and s.sumOsq[2, 0, 1] == 0.0
    s.Ainv = np.array([[1.0, 0.5, 0.0], [0.0, 2.0, 0.25], [0.0, 0.0, 1.0]])
    g = s.accu_one(0, x, x, -0.5)
    assert s.denCount == 0.5 and s.count == float(f32(0.37))
    iv = m["ivar"][g]; P = 0.0
    for col in range(3):
        P += (float(f32(f32(0.5) / iv[col])) * s.Ainv[1, col]) * s.Ainv[0, col]
    assert s.regSq[2, 1, 0] == float(iv[2]) * P and s.regSq[2, 0, 1] == 0.0
    s.accu_one(0, x, x, 0.0)                                                 # factor 0 goes through W(2) with a zero count (eA:2612)
    assert s.denItems == 2 and s.regSq[2, 1, 0] == float(iv[2]) * P
    # cascade: the statistics' frame is the transformed frame, the scoring frame is not
    c = S.Stc(m["refN"], m["mean"], m["ivar"], m["det"], cascade=True); c.A = np.diag([2.0, 1.0, 1.0]); g = c.accu_one(1, x, x, 1.0)
    o0 = float(f32(f32(2.0 * float(x[0])) - m["mean"][g, 0])); assert c.sumOsq[0, 0, 0] == (float(m["ivar"][g, 0]) * o0) * o0


@pytest.mark.parametrize("D", [3, 8, 17, 40])
def test_lda_invariants(D):
    """L within L^T = I and L between L^T = diag(lambda), lambda descending and the spectrum the input was built with.  Bound: the two
    eigen-decompositions and four products of order D leave about D 2^-53 cond(within) of relative error; 100 x that is allowed."""
    W, B, lam = S.synth_scatter(D, seed=D); l = S.Lda([1], np.zeros((1, D)), np.ones((1, D)), [0.0], np.zeros(D), 1)
    L, lw, lb = l.solve(W, B); tol = 100 * D * 2.0 ** -53 * np.linalg.cond(W)
    assert np.abs(L @ W @ L.T - np.eye(D)).max() <= tol
    assert np.abs(L @ B @ L.T - np.diag(lb)).max() <= tol * lam[0]
    assert np.all(np.diff(lb) < 0) and np.allclose(lb, lam, rtol=1e-9)
    # eigenvalues <= 0 of within give zero columns of the whitening: a rank-deficient within loses those directions, nothing is infinite
    W2 = W.copy(); v = np.linalg.eigh(W)[1][:, 0]; W2 = S.sym(W2 - np.linalg.eigvalsh(W)[0] * 1.5 * np.outer(v, v))
    L2, _, _ = l.solve(W2, B); assert np.isfinite(L2).all() and np.linalg.matrix_rank(L2) == D - 1


def test_lda_accumulation_and_the_second_estimate():
    m = S.synth_model(3, 2, 4, 9); mu0 = m["mean"][0]; rng = np.random.default_rng(1); x = rng.standard_normal((40, 4)).astype(f32)
    l = S.Lda(m["refN"], m["mean"], m["ivar"], m["det"], mu0, 2)
    g = l.accu_one(1, x[0], x[1], 0.5)
    oW = (x[1] - m["mean"][g]).astype(f32).astype(np.float64); oB = (m["mean"][g] - mu0).astype(f32).astype(np.float64); oM = (x[1] - mu0).astype(f32).astype(np.float64)
    assert l.count == 0.5 and l.within[2, 1] == (0.5 * oW[2]) * oW[1] and l.between[3, 0] == (0.5 * oB[3]) * oB[0] and l.mixture[1, 1] == (0.5 * oM[1]) * oM[1]
    assert l.within[1, 2] == 0.0
    for t in range(2, 40):
        l.accu_one(int(t % 3), x[t], x[t], 1.0)
    w0 = l.within.copy(); l.estimate(); assert np.array_equal(l.within, w0 / l.count)
    l.estimate(); assert np.array_equal(l.within, w0 / l.count / l.count)     # scaleScatterMatrices divides in place, every time
    with pytest.raises(S.DimensionError):
        S.Lda(m["refN"], m["mean"], m["ivar"], m["det"], mu0, 3).accu_one(0, x[0], x[0], 1.0)


def test_files_built_by_hand():
    D = 2; s, *_ = _stc(D, 30, seed=5, den=6)
    assert not np.triu(s.sumOsq, 1).any() and np.tril(s.regSq).any()
    Sm = np.arange(D ** 3, dtype=np.float64).reshape(D, D, D) * 0.5 - 1.0; Rm = np.arange(D ** 3, dtype=np.float64).reshape(D, D, D) * 0.25 + 3.0
    data = struct.pack(">ii", D, 1) + struct.pack(">fff", 7.0, 1.5, -20.25) + struct.pack(">i", 9) + Sm.tobytes() + Rm.tobytes()
    before = (s.count, s.denCount, s.totalPr, s.totalT, s.sumOsq.copy(), s.regSq.copy())
    s.load_accu_bytes(data)                                                  # loading ADDS
    assert (s.count, s.denCount, s.totalPr, s.totalT) == (before[0] + 7.0, before[1] + 1.5, before[2] - 20.25, before[3] + 9)
    assert np.array_equal(s.sumOsq, before[4] + Sm) and np.array_equal(s.regSq, before[5] + Rm)
    again = s.accu_bytes()                                                   # save reads through sumOsq(): the lower triangle is copied up
    assert len(again) == len(data) and again[:8] == data[:8]
    assert struct.unpack(">fff", again[8:20]) == (f32(s.count), f32(s.denCount), f32(s.totalPr)) and struct.unpack(">i", again[20:24]) == (s.totalT,)
    w = np.frombuffer(again[24:], "=f8").reshape(2, D, D, D)
    assert np.array_equal(w[0], S.sym(before[4] + Sm)) and w[0][0, 0, 1] == (before[4] + Sm)[0, 1, 0] and np.array_equal(s.sumOsq, w[0])
    with pytest.raises(S.DimensionError):
        s.load_accu_bytes(struct.pack(">ii", D + 1, 1) + data[8:])
    with pytest.raises(S.DimensionError):
        s.load_accu_bytes(struct.pack(">ii", D, 2) + data[8:])
    # matrices: raw doubles; load refreshes the inverse; the float file holds the product with an earlier transform
    A = np.array([[0.1, 1.0 / 3.0], [5.0, 1e-3]]); s.A = A.copy()
    assert s.tran_bytes() == struct.pack("=4d", *A.ravel())
    s.A = np.eye(D); s.load_tran_bytes(struct.pack("=4d", *A.ravel())); assert np.array_equal(s.A, A) and np.allclose(s.Ainv @ A, np.eye(D))
    assert s.save_float_bytes() == struct.pack("=4f", *A.astype(f32).ravel())
    tr = np.array([[2.0, 0.5], [-1.0, 0.25]], f32); T = A.astype(f32)
    want = [f32(f32(T[i, 0] * tr[0, j]) + f32(T[i, 1] * tr[1, j])) for i in range(2) for j in range(2)]
    assert s.save_float_bytes(tr) == struct.pack("=4f", *want)
    # LDA: the count comes last, as a float; save writes float32 and load reads float64
    l = S.Lda([1], np.zeros((1, D)), np.ones((1, D)), [0.0], np.zeros(D), 1)
    l.within = np.array([[1.0, 0.0], [0.5, 2.0]]); l.between = np.array([[3.0, 0.0], [0.25, 4.0]]); l.mixture = np.array([[5.0, 0.0], [0.125, 6.0]]); l.count = 10.5
    b = l.accu_bytes()
    assert b == struct.pack(">ii", D, 1) + struct.pack("=12d", 1.0, 0.5, 0.5, 2.0, 3.0, 0.25, 0.25, 4.0, 5.0, 0.125, 0.125, 6.0) + struct.pack(">f", 10.5)
    l.load_accu_bytes(b); assert l.count == 21.0 and l.within[0, 1] == 1.0
    l.L = A.copy(); saved = l.tran_bytes(); assert saved == struct.pack("=4f", *A.astype(f32).ravel()) and len(saved) == 4 * D * D
    l.load_tran_bytes(struct.pack("=4d", *A.ravel())); assert np.array_equal(l.L, A)
    with pytest.raises(ValueError):
        l.load_tran_bytes(saved)                                             # what save wrote is half of what load wants (tr:1961-1984)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stc_host")
    return S.build_host(tmp, os.path.join(PKG, "csrc")), tmp


def test_device_estimation_code_on_the_host(host):
    """csrc/stc_rows.h is written per (thread, thread count) with the barrier passed in: a host program runs the code of k_stc_eig, k_stc_rows
    and k_lda_solve with one thread.  STC agrees with the restatement within 8 x the estimate yardstick; deficient statistics are refused."""
    exe, tmp = host
    for D, T, mmi in ((1, 60, False), (3, 150, False), (8, 400, True), (13, 650, False)):
        s, *_ = _stc(D, T, seed=80 + D, mmi=mmi, den=T // 4 if mmi else 0)
        Alu = s.update(np.eye(D), variant="lu"); Ainv = s.update(np.eye(D), variant="inv")
        rc, A = S.host_stc(exe, tmp, s.G(s.E), np.eye(D), s.gamma(s.E))
        yard = S.yardstick(s, Alu, Ainv); err = float(np.abs(A - Alu).max())
        print("D=%d: host phases at %.3f of the yardstick (8 allowed)" % (D, err / yard))
        assert rc == 0 and err <= 8 * yard, (D, err, yard)
        assert s.aux(A) >= s.aux(Alu) - 8 * yard * abs(s.aux(Alu))
    for D in (3, 13):                                                        # fewer items than D: no G_d has an inverse
        s, *_ = _stc(D, D - 1, seed=90 + D)
        rc, A = S.host_stc(exe, tmp, s.G(1.0), np.eye(D), s.count)
        assert rc == 3 and np.array_equal(A, np.eye(D))
    s, *_ = _stc(3, 150, seed=7); G = s.G(1.0); G[1, 2, 0] = np.inf             # a non-finite entry
    rc, A = S.host_stc(exe, tmp, G, np.eye(3), s.count)
    assert rc == 1 and np.array_equal(A, np.eye(3))
    G = s.G(1.0); rc, A = S.host_stc(exe, tmp, G, np.eye(3), -1.0)              # gamma <= 0: no row can be scaled
    assert rc == 2 and np.array_equal(A, np.eye(3))


@pytest.mark.parametrize("D", [1, 3, 8, 17, 40])
def test_lda_phases_on_the_host(host, D):
    """k_lda_solve's code with one thread against the restatement through numpy.linalg.eigh: the same eigenvalues, the same rows up to sign"""
    exe, tmp = host
    W, B, lam = S.synth_scatter(D, seed=50 + D); l = S.Lda([1], np.zeros((1, D)), np.ones((1, D)), [0.0], np.zeros(D), 1)
    L, lw, lb = l.solve(W, B); rc, Lh, hw, hb = S.host_lda(exe, tmp, W, B)
    tol = 100 * D * 2.0 ** -53 * np.linalg.cond(W)
    assert rc == 0 and np.allclose(np.sort(hw), lw, rtol=tol, atol=0) and np.allclose(hb, lb, rtol=tol, atol=0)
    sign = np.sign((Lh * L).sum(1))[:, None]
    assert np.abs(sign * Lh - L).max() <= 1e4 * tol * np.abs(L).max()           # eigenvectors: the error grows with 1 / gap (gaps >= 10 %)
    assert np.abs(Lh @ W @ Lh.T - np.eye(D)).max() <= tol and np.abs(Lh @ B @ Lh.T - np.diag(hb)).max() <= tol * lam[0]
    rc, *_ = S.host_lda(exe, tmp, np.full((D, D), np.nan), B); assert rc == 1


def test_cpp_facade_has_the_classes(tmp_path):
    """host/dsr_streams.hpp: STCTransformer, LDATransformer, STCEstimator and LDAEstimator with the methods of adapt.i:228-304 and
    train.i:390-500, plain g++; a bare transformer is made without a device and keeps the matrix a file brought"""
    import subprocess
    src = tmp_path / "f.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
#include <cstdio>
int main(int argc, char** argv) {
  VectorFloatFeatureStreamPtr s(new SampleFeature("", 4, 2));
  STCTransformerPtr t(new STCTransformer(s, 4, 1, "STC")); LDATransformerPtr l(new LDATransformer(s, 3, 1, "LDA"));
  printf("%u %s %u %s\n", t->size(), t->name().c_str(), l->size(), l->name().c_str());
  t->load(argv[1]); std::vector<double> A = t->matrix(); printf("%g %g\n", A[1], A[15]);
  l->load(argv[1]); l->save(argv[2]); printf("%g\n", l->matrix()[4]);
  try { STCTransformer bad(s, 3, 1); } catch (jdimension_error& e) { printf("dim %d\n", (int) e.getCode()); }
  try { l->load(argv[2]); } catch (jio_error& e) { printf("io %d\n", (int) e.getCode()); }
  if (s->size() == 0) {                                       // never run: every method of the interface compiles
    ParamTreePtr pt; DistribSetTrainPtr d; DistribSetBasicPtr g; DistribPath p;
    STCEstimatorPtr e(new STCEstimator(s, pt, d, 0, CepstralFeat, true, true, 1, "E")); e->accumulate(p, -1.0f); e->estimate(1, 1.0, 2.0); e->transMatrix();
    e->save("x", (const float*) 0); e->save("x"); e->load("x"); e->zeroAccu(); e->saveAccu("x"); e->loadAccu("x"); e->totalPr(); e->totalT();
    LDAEstimatorPtr f(new LDAEstimator(s, pt, d, g, 0, CepstralFeat, 1)); f->accumulate(p, 1.0f); f->estimate(); f->zeroAccu(); f->saveAccu("x"); f->loadAccu("x");
    f->save("x"); f->load("x");
  }
  return 0;
}
""")
    exe = tmp_path / "f"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    A = np.arange(16, dtype=np.float64).reshape(4, 4) + np.eye(4); m64, m32 = str(tmp_path / "a.f64"), str(tmp_path / "a.f32")
    A.tofile(m64)
    out = subprocess.run([str(exe), m64, m32], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[:5] == ["4 STC 3 LDA", "1 16", "4", "dim 4", "io 7"], out.stdout
    assert open(m32, "rb").read() == A.astype(f32).tobytes()


def test_bare_transformer_has_no_statistics(tmp_path):
    """a handle made without a model (what every STCTransformerPtr / LDATransformerPtr stream owns) keeps a matrix, needs no device for that,
    and answers every accumulator entry with a consistency error"""
    from dsr._capi import DsrError, E_CONSISTENCY
    D = 3; s = Stc(dimN=D); l = Lda(dimN=D); fn = str(tmp_path / "a.bin"); Z3, Z2 = np.zeros((D, D, D)), np.zeros((D, D))
    assert s.D == D and s.nEst == 1 and l.D == D and l.nEst == 1
    calls = [(s.get_accu, 0), (s.get_accu, 0, True), (s.zero, 0), (s.increment, 1.0, 1, 0), (s.save_accu, fn, 0), (s.load_accu, fn, 0), (s.aux, 0),
             (s.aux, 0, np.eye(D), 1.0), (l.get_accu, 0), (l.get_accu, 0, True), (l.zero, 0), (l.save_accu, fn, 0), (l.load_accu, fn, 0)]
    # (accumulate and estimate take the device's stream: tests/test_gpu_stc.py asks them)
    for fn_, *a in calls:
        with pytest.raises(DsrError) as e:
            fn_(*a)
        assert e.value.status == E_CONSISTENCY, (fn_.__name__, e.value.status)
    for fn_, kw in ((s.set_accu, dict(count=1.0)), (s.set_accu, dict(sumOsq=Z3, regSq=Z3)), (l.set_accu, dict(count=1.0)), (l.set_accu, dict(within=Z2))):
        with pytest.raises(DsrError) as e:
            fn_(0, **kw)
        assert e.value.status == E_CONSISTENCY
    assert not os.path.exists(fn)                                            # nothing was written
    # the matrix itself works: set, save, load, the inverse, the float copy
    A = np.array([[2.0, 0.5, 0.0], [0.0, 1.0, 0.25], [1.0, 0.0, 4.0]]); s.set_transform(A); s.save(fn); s.set_transform(np.eye(D)); s.load(fn)
    assert np.array_equal(s.transform(), A) and np.abs(s.inverse() @ A - np.eye(D)).max() < 1e-15 and np.array_equal(s.trans_matrix(), A.astype(f32))
    assert s.status(0) == 0 and s.E(0) == 0.0
    l.set_transform(A); assert np.array_equal(l.transform(), A); l.save(fn); assert open(fn, "rb").read() == A.astype(f32).tobytes()
