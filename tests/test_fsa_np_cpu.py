"""CPU tests of feature-space adaptation: the numpy restatement of asr/train/fsa.cc (tests/fsa_np.py) has the properties constrained MLLR
must have, and keeps the reference's file layout and quirks.  The Python face is imported so that the module stands and falls with it."""
import os
import struct
import subprocess

import numpy as np
import pytest

from dsr._capi import Fsa                                                   # noqa: F401  the binding this restatement is the yardstick of
from dsr.asr.train import FeatureSpaceAdaptationFeaturePtr                  # noqa: F401
from tests import fsa_np as F
from tests.conftest import PKG

f32 = np.float32


def _state(D, T, seed, K=6, R=4, fast=True):
    m = F.synth_model(K, R, D, seed); x, dist, W0 = F.synth_speaker(m, T, seed + 1)
    f = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); f.addAll()
    if fast:
        f.accumulate_fast(x, dist)
    else:
        f.accumulate(x, x, list(dist))
    return f, x, dist, W0


@pytest.mark.parametrize("D,T,iterN", [(3, 150, 10), (13, 650, 5), (39, 2000, 2), (40, 2000, 2)])
def test_auxiliary_function_never_decreases(D, T, iterN):
    """Q(W) = beta log|det A| - 1/2 sum w_i G_i w_i^T + sum w_i . z_i over every single row update, and from the identity to the end.
    A row update maximises Q over that row, so a step is >= 0 up to the rounding of Q's own evaluation: a few hundred fp64 operations on terms
    of the size of |Q|, allowed as 1e-11 |Q|."""
    f, x, dist, W0 = _state(D, T, seed=20 + D)
    I = np.eye(D, D + 1, 1); q = [f.aux(I, 0)]; steps = []

    def after_row(it, i, W):
        q.append(f.aux(W, 0)); steps.append(q[-1] - q[-2])
    W = f.estimate(iterN, after_row=after_row)
    assert len(steps) == iterN * D and min(steps) >= -1e-11 * abs(q[-1]), min(steps)
    assert q[-1] > q[0] and np.isfinite(W).all()


@pytest.mark.parametrize("D,T", [(3, 150), (13, 650), (39, 2000)])
def test_result_is_nearer_to_the_truth_than_the_identity(D, T):
    """about 50 frames a dimension (with 30 the ratio comes close to 1)"""
    f, x, dist, W0 = _state(D, T, seed=40 + D)
    W = f.estimate(10); I = np.eye(D, D + 1, 1)
    ratio = np.linalg.norm(W - W0) / np.linalg.norm(I - W0)
    print("D=%d T=%d: distance to the truth %.3f of the identity's" % (D, T, ratio))
    assert ratio < 1.0


@pytest.mark.parametrize("D,T", [(3, 60), (13, 650)])
def test_the_sign_of_p_cancels(D, T):
    f, x, dist, W0 = _state(D, T, seed=60 + D, fast=(D > 3))
    Wa = f.estimate(3).copy(); f.clear(); Wb = f.estimate(3, flip=True)
    assert np.array_equal(Wa.view(np.int64), Wb.view(np.int64))
    f.clear(); Wc = f.estimate(3, variant="inv")
    assert np.abs(Wa - Wc).max() <= 1e-9 * np.abs(Wa).max()


def _bytes(magic, D, values):
    out = magic + struct.pack(">i", D)
    for v in values:
        out += struct.pack(">f", float(v))
    return out


def test_files_built_by_hand():
    D = 2; f, x, dist, W0 = _state(D, 30, seed=5, fast=False)
    z = np.arange(D * (D + 1), dtype=np.float64) * 0.5 - 1.0; G = np.arange(D * (D + 1) * (D + 1), dtype=np.float64) * 0.25 + 3.0      # a full matrix
    data = _bytes(b"SAS", D, [7.0, 6.5] + list(z) + list(G))
    before = dict(count=f.count[0], beta=f.beta[0], z=f.z[0].copy(), G=f.G[0].copy())
    assert not np.triu(before["G"], 1).any()                                # accumulation writes the lower triangle and column 0 only
    f.load_accu_bytes(data, 0, factor=0.5)                                  # loadAccu ADDS factor x the file
    assert f.count[0] == before["count"] + 3.5 and f.beta[0] == f32(float(before["beta"]) + 3.25)
    assert np.array_equal(f.z[0], before["z"] + 0.5 * z.reshape(D, D + 1)) and np.array_equal(f.G[0], before["G"] + 0.5 * G.reshape(D, D + 1, D + 1))
    again = f.accu_bytes(0)                                                 # a second saveAccu writes the upper triangle the file brought
    assert again[:7] == b"SAS" + struct.pack(">i", D) and len(again) == len(data)
    v = np.frombuffer(again[7:], ">f4")
    assert v[0] == f32(f.count[0]) and v[1] == f.beta[0]
    Gw = v[2 + D * (D + 1):].reshape(D, D + 1, D + 1)
    assert np.array_equal(Gw, f.G[0].astype(f32)) and Gw[0, 0, 1] == f32(0.5 * G[1]) and Gw[:, np.triu_indices(D + 1, 1)[0], np.triu_indices(D + 1, 1)[1]].all()
    # the estimate reads the lower triangle only
    Wa = f.estimate(2).copy(); f.G[0] = np.tril(f.G[0]); f.clear(); assert np.array_equal(Wa, f.estimate(2))
    with pytest.raises(F.ConsistencyError):
        f.load_accu_bytes(b"SAW" + data[3:], 0)
    with pytest.raises(F.DimensionError):
        f.load_accu_bytes(_bytes(b"SAS", D + 1, [0.0] * 40), 0)
    # transforms: float on writing, double again on reading
    W = np.array([[0.1, 1.0 / 3.0, -2.0], [5.0, 1e-3, 0.7]]); f.W[0] = W
    saw = f.tran_bytes(0); assert saw == _bytes(b"SAW", D, W.astype(f32).ravel())
    f.clear(0); f.load_tran_bytes(saw, 0); assert np.array_equal(f.W[0], W.astype(f32).astype(np.float64))
    with pytest.raises(F.IOError_):
        f.load_tran_bytes(b"SAS" + saw[3:], 0)
    with pytest.raises(F.DimensionError):
        f.load_tran_bytes(_bytes(b"SAW", 3, [0.0] * 12), 0)
    with pytest.raises(F.IndexError_):
        f.tran_bytes(1)
    with pytest.raises(F.IndexError_):
        f.accu_bytes(1)


def test_accumulator_operations():
    m = F.synth_model(3, 2, 2, 1); f = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"], nAccu=2); f.addAll()
    x = np.random.default_rng(0).standard_normal((9, 2)).astype(f32)
    f.accumulate(x, x, [0, 1, 2, 0, 1], 0, 0.5); f.accumulate(x, x, [2, 2, 1], 1, 2.0)
    c0, b0, z0, G0 = f.count[0], f.beta[0], f.z[0].copy(), f.G[0].copy()
    f.scaleAccu(0.3, 0)
    assert f.count[0] == c0 * float(f32(0.3)) and f.beta[0] == f32(b0 * f32(0.3)) and np.array_equal(f.G[0], G0 * float(f32(0.3)))
    f.addAccu(0, 1, -0.7)
    assert f.count[0] == c0 * float(f32(0.3)) + float(f32(-0.7)) * 3.0 and np.array_equal(f.z[0], z0 * float(f32(0.3)) + float(f32(-0.7)) * f.z[1])
    f.zeroAccu(0)
    assert f.count[0] == 0 and f.beta[0] == 0 and not f.z[0].any() and not f.G[0].any() and f.G[1].any()


def test_compare_transform_leaves_the_last_column_out():
    m = F.synth_model(2, 2, 3, 1); f = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"], nTran=2)
    f.W[1][:, 0] += 0.5                                                      # the bias counts
    assert f.compareTransform(0, 1) == f32(0.75)
    f.W[1][:, 3] += 9.0                                                      # the last column of A does not (fsa:495-496)
    assert f.compareTransform(0, 1) == f32(0.75)
    f.W[1][0, 2] += 2.0
    assert f.compareTransform(0, 1) == f32(4.75)
    with pytest.raises(F.IndexError_):
        f.compareTransform(0, 2)


def test_accumulate_does_not_advance_on_an_unknown_name():
    m = F.synth_model(3, 2, 4, 2); x = np.random.default_rng(1).standard_normal((6, 4)).astype(f32)
    a = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); a.addAll(); b = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); b.addAll()
    assert a.accumulate(x, x, [1, None, 0, None, None, 2], 0, 1.0) == 3       # "Accumulated 3 frames."
    assert b.accumulate(x, x, [1, 0, 2], 0, 1.0) == 3                        # the same frames 0, 1, 2
    assert np.array_equal(a.G, b.G) and np.array_equal(a.z, b.z) and a.count[0] == 3
    # a distribution that is not switched on is ignored before anything is counted, but its frame is used up
    c = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); c.add(1); c.add(2)
    assert c.accumulate(x, x, [1, 0, 2], 0, 1.0) == 3 and c.count[0] == 2 and c.beta[0] == 2
    d = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); d.addAll(); d.accu_one(1, x[0], x[0], 0, 1.0); d.accu_one(2, x[2], x[2], 0, 1.0)
    assert np.array_equal(c.G, d.G)
    # the scoring frame chooses the Gaussian, the source frame makes the statistics
    e = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); e.addAll(); g = e.accu_one(0, x[0], x[3], 0, 1.0)
    assert g == F.nearest(m["refN"], m["mean"], m["ivar"], m["det"], x[0], 0) and e.z[0][0, 1] == float(f32(m["mean"][g, 0] * m["ivar"][g, 0])) * float(x[3, 0])


def test_lattice_takes_every_second_frame():
    m = F.synth_model(3, 2, 4, 3); x = np.random.default_rng(2).standard_normal((12, 4)).astype(f32)
    a = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); a.addAll()
    links = [(2, 0.5, 0, 4), (0, 0.1, 0, 3), (1, 10.5, 2, 6), (3, 0.0, 5, 8)]   # input 0 and gamma > 10 are skipped
    assert a.accumulate_lattice(x, x, links, 0, 2.0) == 2
    b = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); b.addAll()
    p1 = f32(2.0 * np.exp(-0.5)); p2 = f32(2.0)
    for t in (0, 2, 4):
        b.accu_one(1, x[t], x[t], 0, p1)
    for t in (5, 7):
        b.accu_one(2, x[t], x[t], 0, p2)
    assert a.count[0] == 5 and np.array_equal(a.G, b.G) and np.array_equal(a.z, b.z) and a.beta[0] == b.beta[0]


@pytest.mark.parametrize("D,seed", [(3, 0), (13, 2), (39, 2)])
def test_deficient_data_is_not_finite(D, seed):
    """(D + 1) / 2 frames: G_i has no inverse and the quadratic's discriminant can be negative -- the reference then stores NaN (other draws
    give finite numbers without meaning).  The product refuses such statistics (tests/test_gpu_fsa.py)."""
    m = F.synth_model(6, 4, D, 1); x, dist, W0 = F.synth_speaker(m, (D + 1) // 2, seed)
    f = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); f.addAll(); f.accumulate(x, x, list(dist))
    assert not np.isfinite(f.estimate(1)).all()


def test_cpp_facade_has_the_class(tmp_path):
    """host/dsr_streams.hpp: FeatureSpaceAdaptationFeature with the methods of train.i:534-573, plain g++; before distribSet every use is a
    jconsistency_error"""
    src = tmp_path / "f.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
#include <cstdio>
int main() {
  VectorFloatFeatureStreamPtr s(new SampleFeature("", 320, 160));
  FeatureSpaceAdaptationFeaturePtr f(new FeatureSpaceAdaptationFeature(s, 2, 2, "FSA"));
  printf("%u %s\n", f->size(), f->name().c_str());
  try { f->addAll(); } catch (jconsistency_error& e) { printf("cons %d\n", (int) e.getCode()); }
  DistribPath p; p.push_back("x");
  try { f->accumulate(p); } catch (jconsistency_error& e) { printf("cons %d\n", (int) e.getCode()); }
  if (s->size() == 0) {                                       // never run: every method of the interface compiles
    LatticePtr l; DistribSetBasicPtr d; f->distribSet(d); f->accumulateLattice(l, 0, 1.0f); f->estimate(10, 0, 0); f->save("x", 0); f->load("x", 0);
    f->saveAccu("x", 0); f->loadAccu("x", 0, 1.0f); f->clear(0); f->compareTransform(0, 1); f->zeroAccu(0); f->scaleAccu(0.5f, 0); f->addAccu(0, 1, 1.0f);
    f->add(0); f->setTopN(1); f->topN(); f->count(0); f->shift(); f->setShift(-1.0f);
  }
  return 0;
}
""")
    exe = tmp_path / "f"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[:3] == ["320 FSA", "cons 3", "cons 3"]


def test_device_estimation_code_on_the_host(tmp_path):
    """csrc/fsa_rows.h is written per (thread, thread count) with the barrier passed in: a host program runs the code of k_fsa_eig and k_fsa_rows
    with one thread.  Its result agrees with the restatement, and deficient statistics are refused."""
    src = tmp_path / "e.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "fsa_rows.h"
using namespace dsr;
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); double hd[3]; if (!f || fread(hd, 8, 3, f) != 3) return 9;
  const int D = (int) hd[0], iterN = (int) hd[1], n = D + 1, m = (n + 1) & ~1; const double beta = hd[2];
  std::vector<double> G((size_t) D * n * n), z((size_t) D * n), W((size_t) D * n), Ginv(G.size());
  if (fread(G.data(), 8, G.size(), f) != G.size() || fread(z.data(), 8, z.size(), f) != z.size() || fread(W.data(), 8, W.size(), f) != W.size()) return 9;
  fclose(f);
  auto sync = [] {};
  int rc = 0;
  for (int i = 0; i < D && !rc; i++) {
    std::vector<double> a(G.begin() + (size_t) i * n * n, G.begin() + (size_t) (i + 1) * n * n), v(n * n), t(n), cs(m), sq(2);
    if (!fsa_eig_run(a.data(), v.data(), t.data(), cs.data(), sq.data(), n, Ginv.data() + (size_t) i * n * n, 0, 1, sync)) rc = 1;
  }
  if (!rc) {
    std::vector<double> mem(FsaWork::doubles(D, 1) + D); FsaWork w; w.carve(mem.data(), D, 1);
    for (int e = 0; e < D * n; e++) w.W[e] = W[e];
    if (!fsa_rows_run(w, D, iterN, Ginv.data(), z.data(), beta, 0, 1, sync)) rc = 2;
    else for (int e = 0; e < D * n; e++) W[e] = w.W[e];
  }
  f = fopen(argv[2], "wb"); double r = rc; fwrite(&r, 8, 1, f); fwrite(W.data(), 8, W.size(), f); fclose(f);
  return 0;
}
""")
    exe = tmp_path / "e"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)])

    def run(f, iterN):
        D = f.D; inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        np.concatenate([[D, iterN, float(f.beta[0])], f.sym(0).ravel(), f.z[0].ravel(), np.eye(D, D + 1, 1).ravel()]).astype(np.float64).tofile(inp)
        subprocess.check_call([str(exe), inp, outp]); r = np.fromfile(outp)
        return int(r[0]), r[1:].reshape(D, D + 1)
    for D, T, iterN in ((1, 60, 3), (3, 150, 10), (13, 650, 3)):
        f, x, dist, W0 = _state(D, T, seed=80 + D)
        rc, W = run(f, iterN)
        Ws = f.estimate(iterN); f.clear(); Wi = f.estimate(iterN, variant="inv")
        kappa = max(np.linalg.cond(g) for g in f.sym(0))
        yard = max(float(np.abs(Ws - Wi).max()), iterN * (D + 1) * 2.0 ** -53 * kappa * float(np.abs(Ws).max()))
        assert rc == 0 and np.abs(W - Ws).max() <= 8 * yard, (D, float(np.abs(W - Ws).max()), yard)
    for D, seed in ((3, 0), (3, 1), (13, 2), (13, 0)):                        # (D + 1) / 2 frames, whether the restatement is finite or not
        m = F.synth_model(6, 4, D, 1); x, dist, W0 = F.synth_speaker(m, (D + 1) // 2, seed)
        f = F.Fsa(m["refN"], m["mean"], m["ivar"], m["det"]); f.addAll(); f.accumulate(x, x, list(dist))
        rc, W = run(f, 1)
        assert rc != 0 and np.array_equal(W, np.eye(D, D + 1, 1))
