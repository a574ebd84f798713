"""CPU checks of tests/train_np.py, the numpy restatement of asr/train (codebookTrain.cc, distribTrain.cc) that the GPU tests of
dsr._capi.Trainer compare against: the accumulator file format against bytes built by hand, the ML update chain on data from a known model,
the MMI updates with numerator = denominator, and Gaussian splitting."""
import math
import struct

import numpy as np
import pytest

import dsr.asr.train as asr_train                      # noqa: F401  (the public face these tests belong to)
from dsr._capi import Trainer                           # noqa: F401
from tests import train_np as T

f32 = np.float32


def _s(name):
    b = name.encode(); return struct.pack(">h", len(b)) + b + b"\0"


def _two_codebook_set():
    """list order zeta, mid, alpha: 'mid' stays empty; the map must come out as alpha, zeta"""
    m = T.random_model([2, 3, 1], 3, seed=5)
    m.cbNames = ["zeta", "mid", "alpha"]; m.dsNames = ["d-zeta", "d-mid", "d-alpha"]
    a = T.Accu(m)
    rng = np.random.default_rng(9)
    a.count[:2] = [1.5, 0.0]; a.den[:2] = [0.0, 0.25]; a.sumO[:2] = rng.standard_normal((2, 3)); a.sumOsq[:2] = rng.uniform(0, 2, (2, 3))
    a.count[5] = 7.0; a.sumO[5] = [1.0, -2.0, 3.0]; a.sumOsq[5] = [4.0, 5.0, 6.0]
    a.dcount[:2] = [1.5, 0.0]; a.dden[:2] = [0.0, 0.25]; a.dcount[5] = 7.0
    return m, a


def test_codebook_accumulator_file_format():
    m, a = _two_codebook_set()
    size = lambda name, refN: 2 * refN * 4 + 2 * refN * 4 * 3 + 2 + len(name) + 1 + 5 * 4 + 4         # Accu::size, cT:542-563
    body = b""
    for k, name in ((0, "zeta"), (2, "alpha")):                                                        # list order, the empty codebook skipped
        body += _s(name) + struct.pack(">5i", m.refN[k], 3, 1, 2, 0)
        for g in range(m.off[k], m.off[k + 1]):
            body += struct.pack(">2f", a.count[g], a.den[g]) + struct.pack(">3f", *a.sumO[g]) + struct.pack(">3f", *a.sumOsq[g])
        body += struct.pack(">i", 123456789)
    head = struct.pack(">fi", 12.5, 77) + _s("alpha") + struct.pack(">i", size("zeta", 2)) + _s("zeta") + struct.pack(">i", 0) + _s("EndOfAccumulators")
    data = a.save_codebook_accus(12.5, 77)
    assert data == head + body
    assert len(body) == size("zeta", 2) + size("alpha", 1)                                             # offsets equal size()
    # loading adds: twice doubles, a factor scales, the header comes back
    b = T.Accu(m)
    assert b.load_codebook_accus(data) == (12.5, 77)
    for x, y in zip(b.arrays()[:4], a.arrays()[:4]):
        assert np.array_equal(x, y.astype(f32).astype(np.float64))
    b.load_codebook_accus(data)
    assert np.array_equal(b.sumO, 2 * a.sumO.astype(f32).astype(np.float64)) and b.count[5] == 14.0
    c = T.Accu(m); c.load_codebook_accus(data, factor=-0.5)
    assert np.array_equal(c.sumOsq, (f32(-0.5) * a.sumOsq.astype(f32)).astype(np.float64)) and c.den[1] == -0.125
    # counts only: no sums in the file, the sizes shrink
    co = a.save_codebook_accus(0.0, 0, countsOnly=True)
    d = T.Accu(m); d.load_codebook_accus(co)
    assert np.array_equal(d.count, a.count) and not d.sumO.any() and len(co) < len(data)
    # parts: 3 codebooks in 3 parts, part 3 = the last one only
    e = T.Accu(m); e.load_codebook_accus(data, nParts=3, part=3)
    assert e.count[5] == 7.0 and not e.count[:5].any()
    # a wrong refN and a broken marker raise and leave the accumulators alone
    m2 = T.random_model([3, 3, 1], 3, seed=5); m2.cbNames = m.cbNames
    w = T.Accu(m2)
    with pytest.raises(T.DimensionError):
        w.load_codebook_accus(data)
    assert not w.count.any()
    bad = bytearray(data); bad[-1] ^= 1
    with pytest.raises(IOError):
        T.Accu(m).load_codebook_accus(bytes(bad))


def test_distrib_accumulator_file_format():
    m, a = _two_codebook_set()
    body = struct.pack(">2i", 2, 1) + struct.pack(">4f", 1.5, 0.0, 0.0, 0.25) + struct.pack(">i", 987654321)
    body += struct.pack(">2i", 1, 1) + struct.pack(">2f", 7.0, 0.0) + struct.pack(">i", 987654321)
    head = _s("d-alpha") + struct.pack(">i", 2 * 2 * 4 + 12) + _s("d-zeta") + struct.pack(">i", 0) + _s("EndOfAccumulators")
    data = a.save_distrib_accus()
    assert data == head + body
    b = T.Accu(m); b.load_distrib_accus(data); b.load_distrib_accus(data)
    assert np.array_equal(b.dcount, 2 * a.dcount) and np.array_equal(b.dden, 2 * a.dden) and not b.count.any()
    m2 = T.random_model([2, 3, 2], 3, seed=5); m2.dsNames = m.dsNames
    with pytest.raises(T.DimensionError):
        T.Accu(m2).load_distrib_accus(data)


def test_add_scales_the_codebook_sums_and_not_the_distribution_counts():
    m, a = _two_codebook_set()
    b = T.Accu(m); b.add(a, 0.5)
    assert np.array_equal(b.sumO, 0.5 * a.sumO) and np.array_equal(b.count, 0.5 * a.count) and np.array_equal(b.dcount, a.dcount)      # dT:254-262


def _em_setup(seed=31):
    truth = T.random_model([4, 4, 4], 13, seed=seed, spread=3.0)
    rng = np.random.default_rng(seed + 1)
    ids = np.repeat(np.arange(3), 1000)
    x = np.concatenate([T.sample(truth, k, 1000, rng) for k in range(3)])
    p = rng.permutation(3000); ids, x = ids[p], x[p]
    start = truth.copy()
    start.mean = (start.mean + 0.4 * rng.standard_normal(start.mean.shape)).astype(f32)
    start.cv = (start.cv / f32(1.5)).astype(f32)                                     # variances 1.5 x the truth's
    start.val = np.full(12, -math.log(0.25), f32)
    T.Accu(start).invert_variances(); T.Accu(start).fix_gconsts(); T.Accu(start).invert_variances()
    return truth, start, x, ids


def test_ml_rounds_do_not_increase_the_path_score():
    truth, m, x, ids = _em_setup()
    d0 = np.abs(m.mean - truth.mean).mean()
    scores = []
    for _ in range(5):
        a = T.Accu(m)
        scores.append(a.accumulate_path(x, ids, 1.0))
        assert np.allclose(a.count.sum(), 3000.0, rtol=1e-5) and np.array_equal(a.count, a.dcount) and not a.den.any()
        a.update(); total, floored = a.floor_variances(); a.fix_gconsts(); a.invert_variances()
        assert total == 12 * 13 and floored == 0
    print("path scores per round:", scores)
    assert all(scores[i + 1] <= scores[i] for i in range(4)), scores               # costs: -log likelihood must not go up
    assert scores[-1] < scores[0] - 100.0
    d1 = np.abs(m.mean - truth.mean).mean()
    assert d1 < 0.5 * d0, (d0, d1)                                                   # the means moved toward the truth
    for k in range(3):
        assert abs(np.exp(-m.val[m.off[k]:m.off[k + 1]].astype(np.float64)).sum() - 1.0) < 1e-5


@pytest.mark.parametrize("merialdo", [False, True])
def test_mmi_with_equal_numerator_and_denominator_keeps_the_means(merialdo):
    truth, m, x, ids = _em_setup(seed=41)
    a = T.Accu(m)
    a.accumulate_path(x[:600], ids[:600], 1.0); a.accumulate_path(x[:600], ids[:600], -1.0)
    assert np.allclose(a.count, a.den) and np.allclose(a.dcount, a.dden) and np.abs(a.sumO).max() < 1e-3
    mean0, var0, val0 = m.mean.copy(), (1.0 / m.cv.astype(np.float64)), m.val.copy()
    a.update_mmi(3, E=2.0, merialdo=merialdo)
    big = a.count > a.minCount
    assert big.sum() >= 8
    assert np.abs(m.mean - mean0)[big].max() <= 1e-5 * np.abs(mean0).max() + np.abs(a.sumO).max()   # float rounding of the update
    assert np.allclose(m.cv[big], var0[big], rtol=1e-4, atol=1e-4)                   # variances come back (cv holds variances after the update)
    assert np.allclose(m.cv[~big], var0[~big], rtol=1e-6)                            # the low-count branch inverts in place
    if not merialdo:
        assert np.allclose(m.val, val0, atol=1e-5)


@pytest.mark.parametrize("merialdo", [False, True])
def test_mmi_consistency_errors(merialdo):
    """dT:166-222.  C is the largest derivative, so with finite accumulators no count can come out negative -- even when the denominator
    outweighs the numerator the weights stay a distribution; the consistency error that can be reached is the NaN weight, which a
    non-finite accumulator gives."""
    m = T.random_model([3], 2, seed=3)
    a = T.Accu(m); a.dcount[:] = [1.0, 2.0, 0.5]; a.dden[:] = [4.0, 1.0, 3.0]; a.count[:] = 0.0
    a.update_mmi(2, merialdo=merialdo)
    assert np.isfinite(m.val).all() and abs(np.exp(-m.val.astype(np.float64)).sum() - 1.0) < 1e-5
    val = m.val.copy()
    a.dcount[1] = -np.inf
    with pytest.raises(T.ConsistencyError):
        a.update_mmi(2, merialdo=merialdo)
    assert np.array_equal(m.val, val)


def test_split_conserves_weight_and_count_and_stops_at_256():
    m = T.random_model([3, 2], 4, seed=8)
    m.count[:] = [4.0, 9.0, 2.0, 1.0, 6.0]
    a = T.Accu(m); a.count[:] = 1.0; a.dcount[:] = 1.0; a.sumO[:] = 1.0
    w0 = np.exp(-m.val[:3].astype(np.float64)).sum(); mean1, cv1, det1 = m.mean[1].copy(), m.cv[1].copy(), m.det[1]
    assert a.split(0, 0.0, 0.2) == 1
    assert m.refN == [4, 2] and m.off == [0, 4, 6] and m.mean.shape == (6, 4) and a.sumO.shape == (6, 4)
    assert abs(np.exp(-m.val[:4].astype(np.float64)).sum() - w0) < 1e-6 and m.count[:4].sum() == 15.0 and m.count[1] == m.count[3] == 4.5
    p = (0.2 / np.sqrt(cv1.astype(np.float64))).astype(f32)
    assert np.array_equal(m.mean[1], mean1 + p) and np.array_equal(m.mean[3], mean1 - p) and np.array_equal(m.cv[3], cv1) and m.det[3] == det1
    assert not a.count[:4].any() and not a.dcount[:4].any() and not a.sumO[:4].any()     # fresh accumulators for the split codebook ...
    assert a.count[4:].all() and a.sumO[4:].all()                                         # ... the others keep theirs, one row further up
    with pytest.raises(T.ParameterError):
        a.split(1, 100.0, 0.2)                                                             # maxCount < minCount
    big = T.random_model([256], 2, seed=1)
    with pytest.raises(T.DimensionError):
        T.Accu(big).split(0)


def test_posterior_special_cases():
    m = T.random_model([1, 4], 5, seed=2, scale=[1.3, 0.7])
    x = np.random.default_rng(0).standard_normal(5).astype(f32)
    s, mix = T.posterior(m, x, 0)
    assert mix.tolist() == [1.0]                                                           # refN == 1, cB:742-747
    m.mean[2] += 100.0                                                                     # far away: exponent below -100, posterior exactly 0
    info = {}
    s, mix = T.posterior(m, x, 1, info)
    assert mix[1] == 0.0 and min(info["exps"]) < -100.0 and abs(float(mix.sum()) - 1.0) < 1e-6
    with pytest.raises(T.NumericError):
        T.posterior(m, np.full(5, np.nan, f32), 1)
    with pytest.raises(T.NumericError):
        T.posterior(m, np.full(5, np.nan, f32), 0)


def test_cpp_facade_training_classes(tmp_path):
    """host/dsr_streams.hpp: CodebookSetTrain / DistribSetTrain / DistribTrain under the reference's names compile with plain g++ and map
    the library's errors (without model files: JIO, without a device: JINITIALIZATION)"""
    import os
    import subprocess
    from tests.conftest import PKG
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
int main() {
  try {
    VectorFloatFeatureStreamPtr s(new SampleFeature("", 320, 160));
    FeatureSetPtr fs(new FeatureSet()); fs->add(s);
    CodebookSetTrainPtr cbs(new CodebookSetTrain("", fs, "/nonexistent.cb", 3.0));
    try { cbs->update(); } catch (jconsistency_error& e) { printf("noaccu %d\n", (int) e.getCode()); }
    DistribSetTrainPtr dss(new DistribSetTrain(cbs, "", "/nonexistent.ds"));
    DistribPath path; path.push_back("ds0");
    dss->accumulate(path, 1.0f); cbs->update(); dss->update(); cbs->floorVariances(); cbs->fixGConsts(); cbs->invertVariances();
    dss->find(0u).split(0.0f, 0.2f); dss->saveAccus("/dev/null"); cbs->saveAccus("/dev/null"); dss->updateMMI(1, 1, true); cbs->updateMMI(1, 1, 2.0);
    LatticePtr lat; dss->accumulateLattice(lat, -1.0f);
  } catch (j_error& e) { printf("err %d\n", (int) e.getCode()); }
  return 0;
}
""")
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "noaccu 3" and lines[1] in ("err 7", "err 6")
