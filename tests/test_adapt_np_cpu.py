"""MLLR without a GPU: the numpy restatement (tests/adapt_np.py) on known answers, and the host side of the library -- the speaker
parameter tree and its text files (csrc/adapt.cpp through dsr._capi.ParamTree) -- against it byte for byte.

The codebook files with the regression-class table are exercised in tests/test_gpu_adapt.py: dsr_gmm_load puts the model on the device, so
no model can be made here (tests/test_abi_cpu.py::test_no_cpu_fallback)."""
import numpy as np
import pytest

from tests import adapt_np as A

f32 = np.float32

W2 = np.array([[1.25, -0.5, 0.125], [1e-7, 3.0, -2.5e10]])
W2b = np.array([[0.333333333333, 2.0, 1.0], [0.1, 0.2, 0.3]])


def _file(tmp_path, name, text):
    p = tmp_path / name; p.write_bytes(text.encode()); return str(p)


HAND = ("<AdaptType> MLLR\n<RegClass> 1\n<MLLRParam> 2\n 1.25 -0.5\n 1e-07 3\n<BiasOffset> 2\n 0.125 -2.5e+10\n<EndClass>\n"
        "<AdaptType> MLLR\n<RegClass> 6\n<MLLRParam> 2\n 0.333333 2\n 0.1 0.2\n<BiasOffset> 2\n 1 0.3\n<EndClass>\n")


def test_hand_built_parameter_file_reads_and_writes_byte_for_byte(dsr, tmp_path):
    ref = A.ParamTree(HAND)
    assert sorted(ref.map) == [1, 6] and ref.type == A.MLLR and ref.text() == HAND
    assert np.array_equal(ref.map[1].W(), W2) and np.array_equal(ref.map[6].matrix, [[0.333333, 2.0], [0.1, 0.2]])
    t = dsr.ParamTree(_file(tmp_path, "hand.mllr", HAND))
    assert t.indices() == [1, 6] and t.type() == 3 and t.hasIndex(6) and not t.hasIndex(3)
    assert np.array_equal(t.find(1, False), W2)
    out = str(tmp_path / "out.mllr"); t.write(out)
    assert open(out, "rb").read() == HAND.encode()
    # values that are not round in %g: the writer and the restatement print the same digits
    t2 = dsr.ParamTree(); t2.set(6, W2b); t2.set(1, W2); t2.write(out)                     # written in index order, not insertion order
    r2 = A.ParamTree(); r2.findMLLR(6).assign(W2b); r2.findMLLR(1).assign(W2)
    assert open(out, "rb").read() == r2.text().encode() == HAND.encode()
    t.clear()
    assert t.indices() == [] and t.type() == 0
    t.read(out)
    assert t.indices() == [1, 6]
    t.read("")                                                                          # ParamTree::read(""): cleared, nothing read
    assert t.indices() == [] and t.type() == 0


def test_class_zero_is_written_as_one(dsr, tmp_path):
    text = "<AdaptType> MLLR\n<RegClass> 0\n<MLLRParam> 1\n 2\n<BiasOffset> 1\n 0.5\n<EndClass>\n"
    ref = A.ParamTree(text)
    assert list(ref.map) == [0] and ref.text() == text.replace("<RegClass> 0", "<RegClass> 1")
    t = dsr.ParamTree(_file(tmp_path, "zero.mllr", text))
    assert t.indices() == [0]
    out = str(tmp_path / "out.mllr"); t.write(out)
    assert open(out).read() == ref.text()


def test_free_layout_and_missing_bias(dsr, tmp_path):
    text = "\n  <AdaptType>MLLR <RegClass>3\n<MLLRParam>  2\n1 2\n\n3 4 <EndClass>"
    ref = A.ParamTree(text); t = dsr.ParamTree(_file(tmp_path, "free.mllr", text))
    want = "<AdaptType> MLLR\n<RegClass> 3\n<MLLRParam> 2\n 1 2\n 3 4\n<EndClass>\n"            # no <BiasOffset> for an empty bias (tr:309-319)
    out = str(tmp_path / "out.mllr"); t.write(out)
    assert ref.text() == want and open(out).read() == want


@pytest.mark.parametrize("text, status, exc", [
    ("<AdaptType> RAPT\n<RegClass> 1\n<RAPTParam> 1\n 0.1\n<EndClass>\n", 15, A.TypeError_),              # jtype_error: another adaptation type
    ("<AdaptType> SLAPT\n<RegClass> 1\n<EndClass>\n", 15, A.TypeError_),
    ("<RegClass> 1\n<EndClass>\n", 15, A.TypeError_),                                                      # "Unable to determine adaptation type."
    ("<AdaptType> MLLR\n<RegClass> 1\n<RAPTParam> 1\n 0.1\n<EndClass>\n", 13, A.ParameterError),           # jparameter_error
    ("<AdaptType> MLLR\n<AdaptType> SLAPT\n<EndClass>\n", 13, A.ParameterError),                          # type consistency inside a class
    ("<AdaptType> MLLR\n<RegClass> 1\n<STCParam> 1\n<EndClass>\n", 13, A.ParameterError),                  # unexpected symbol
])
def test_wrong_type_files_raise(dsr, tmp_path, text, status, exc):
    with pytest.raises(exc):
        A.ParamTree(text)
    t = dsr.ParamTree(); t.set(2, W2)
    with pytest.raises(dsr.DsrError) as e:
        t.read(_file(tmp_path, "bad.mllr", text))
    assert e.value.status == status
    assert t.indices() == []                                                            # read() clears first
    with pytest.raises(dsr.DsrError) as e:
        t.read(_file(tmp_path, "empty.mllr", ""))
    assert e.value.status == 4                                                          # jconsistency_error: no parameters at all
    with pytest.raises(A.ConsistencyError):
        A.ParamTree().read("")
    with pytest.raises(dsr.DsrError) as e:
        t.read(_file(tmp_path, "blank.mllr", "\n"))                                     # a character, but no symbol: ParamBase::param's jtype_error
    assert e.value.status == 15
    with pytest.raises(A.TypeError_):
        A.ParamTree().read("\n")
    with pytest.raises(dsr.DsrError) as e:
        t.read(str(tmp_path / "missing.mllr"))
    assert e.value.status == 8


def test_find_copies_the_nearest_ancestor(dsr, tmp_path):
    t = dsr.ParamTree(); r = A.ParamTree()
    for tree_set in (lambda rc, W: t.set(rc, W), lambda rc, W: r.findMLLR(rc).assign(W)):
        tree_set(1, W2); tree_set(5, W2b)
    assert np.array_equal(t.find(11), W2b) and np.array_equal(r.find(11).W(), W2b)      # 11 -> 5
    assert np.array_equal(t.find(12), W2) and np.array_equal(r.find(12).W(), W2)        # 12 -> 6 -> 3 -> 1
    assert t.indices() == sorted(r.map) == [1, 5, 11, 12]
    t.set(5, 2 * W2b)                                                                   # a copy, not a link
    assert np.array_equal(t.find(11), W2b)
    out = str(tmp_path / "out.mllr"); t.write(out); r.map[5].assign(2 * W2b)
    assert open(out).read() == r.text()
    for bad, useAncestor in ((0, True), (7, False)):
        with pytest.raises(dsr.DsrError) as e:
            t.find(bad, useAncestor)
        assert e.value.status == 6                                                      # jindex_error
        with pytest.raises(A.IndexError_):
            r.find(bad, useAncestor)
    u = dsr.ParamTree(); u.set(4, W2)
    with pytest.raises(dsr.DsrError) as e:
        u.find(3)                                                                       # "No ancestor for node 3."
    assert e.value.status == 6
    assert u.findMLLR(3).shape == (0, 1) and u.indices() == [3, 4]                      # findMLLR inserts an empty parameter instead (tr:919)
    with pytest.raises(dsr.DsrError) as e:
        t.set(5, np.zeros((3, 4)))                                                      # bias sizes do not match (tr:637-640)
    assert e.value.status == 5


def test_is_ancestor(dsr):
    for a in range(1, 20):
        for c in range(1, 40):
            want = any((c >> k) == a for k in range(6))
            assert A.is_ancestor(a, c) == want and dsr.is_ancestor(a, c) == want
    for a, c in ((0, 3), (3, 0)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.is_ancestor(a, c)
        assert e.value.status == 6
        with pytest.raises(A.IndexError_):
            A.is_ancestor(a, c)


def _exact_case(D, nG, seed):
    """statistics whose every float product of _calcGi / _calcZ is exact: small integer means, inverse variances and counts that are powers of
    two or small integers, (A | b) in eighths"""
    rng = np.random.default_rng(seed)
    mean = rng.integers(-3, 4, (nG, D)).astype(f32); iv = rng.choice(np.array([0.5, 1.0, 2.0], f32), (nG, D))
    c = rng.integers(1, 5, nG).astype(np.float64)
    W = np.concatenate([np.eye(D) + rng.integers(-2, 3, (D, D)) / 8.0, rng.integers(-8, 9, (D, 1)) / 4.0], axis=1)
    xi = np.concatenate([mean.astype(np.float64), np.ones((nG, 1))], axis=1)
    sumO = c[:, None] * (xi @ W.T)
    return mean, iv, c, sumO, W


@pytest.mark.parametrize("D, nG", [(1, 4), (3, 8), (5, 12), (13, 40), (39, 80)])
def test_known_answer_gives_back_the_transform(D, nG):
    assert nG >= 2 * (D + 1)
    mean, iv, c, sumO, W = _exact_case(D, nG, seed=7 * D + nG)
    G, Z, ttl = A.calc_stats(mean, iv, c, sumO, range(nG))
    assert ttl == c.sum() and np.array_equal(G, np.transpose(G, (0, 2, 1)))
    xi = np.concatenate([mean.astype(np.float64), np.ones((nG, 1))], axis=1)
    for i in (0, D - 1):                                                                # the exact statistics
        assert np.array_equal(G[i], (xi.T * (c * iv[:, i])) @ xi) and np.array_equal(Z[i], G[i] @ W[i])
    West = A.estimate_W(G, Z)
    assert np.abs(West - W).max() <= 1e-9, np.abs(West - W).max()
    # a zero count is skipped for G AND z, whatever its sumO (eA:2110, 2138)
    c2 = np.concatenate([c, [0.0]]); mean2 = np.concatenate([mean, mean[:1] + 1]); iv2 = np.concatenate([iv, iv[:1]]); sumO2 = np.concatenate([sumO, 100 + sumO[:1]])
    G2, Z2, _ = A.calc_stats(mean2, iv2, c2, sumO2, range(nG + 1))
    assert np.array_equal(G2, G) and np.array_equal(Z2, Z)


@pytest.mark.parametrize("D, nG, seed", [(3, 8, 1), (13, 28, 2), (39, 80, 3)])
def test_auxiliary_function_does_not_go_down(D, nG, seed):
    """Q(W) = sum (sumO - c mu' / 2) mu' iv (_calcMixLhood, eA:1603-1620): the estimate is its maximiser, so it is not below the identity's"""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((nG, D)).astype(f32); iv = (1.0 / rng.uniform(0.5, 2.0, (nG, D))).astype(f32)
    c = rng.uniform(5.0, 50.0, nG)
    Wtrue = np.concatenate([np.eye(D) + 0.1 * rng.standard_normal((D, D)), 0.5 * rng.standard_normal((D, 1))], axis=1)
    xi = np.concatenate([mean.astype(np.float64), np.ones((nG, 1))], axis=1)
    sumO = c[:, None] * (xi @ Wtrue.T + 0.05 * rng.standard_normal((nG, D)))
    G, Z, _ = A.calc_stats(mean, iv, c, sumO, range(nG))
    West = A.estimate_W(G, Z)
    ident = np.concatenate([np.eye(D), np.zeros((D, 1))], axis=1)
    q0 = A.mix_lhood(ident, mean, iv, c, sumO, range(nG)); q1 = A.mix_lhood(West, mean, iv, c, sumO, range(nG)); qt = A.mix_lhood(Wtrue, mean, iv, c, sumO, range(nG))
    assert q1 >= q0 and q1 >= qt - 1e-6 * abs(qt), (q0, q1, qt)


def test_svd_solve_drops_small_singular_values():
    rng = np.random.default_rng(5); n = 6
    X = rng.standard_normal((3, n)); Gi = X.T @ X; z = Gi @ rng.standard_normal(n)
    w, rank = A.svd_solve(Gi, z)
    assert rank == 3 and np.allclose(w, np.linalg.pinv(Gi, rcond=1e-7) @ z, rtol=1e-9, atol=1e-12)
    w0, r0 = A.svd_solve(np.zeros((n, n)), np.ones(n))
    assert r0 == 0 and not w0.any()


def test_back_off_copies_or_estimates_at_the_ancestor():
    classes = [4] * 3 + [5] * 3 + [3] * 3
    Ws = {k: np.full((2, 3), float(k)) for k in (1, 2, 3, 4, 5)}
    # every leaf above the threshold: three estimates, each stored under its own class (twice the same key)
    tree, plan = A.estimate_tree(classes, {1: 90.0, 2: 60.0, 3: 30.0, 4: 30.0, 5: 30.0}, lambda n: Ws[n], 10.0)
    assert plan == [(0, 3, 3, 0), (0, 4, 4, 0), (0, 5, 5, 0)] and sorted(tree.map) == [3, 4, 5]
    # leaf 4 is below: estimated at node 2 and stored under 4 and 2; leaf 5 is below as well: node 2 is there, copy
    tree, plan = A.estimate_tree(classes, {1: 90.0, 2: 60.0, 3: 30.0, 4: 5.0, 5: 10.0}, lambda n: Ws[n], 10.0)
    assert plan == [(0, 3, 3, 0), (0, 2, 4, 0), (0, 2, 5, 1)] and sorted(tree.map) == [2, 3, 4, 5]
    assert np.array_equal(tree.map[4].W(), Ws[2]) and np.array_equal(tree.map[2].W(), Ws[2]) and np.array_equal(tree.map[5].W(), Ws[2])
    assert tree.map[5].regClass == 5 and tree.map[3].W()[0, 0] == 3.0
    # leaf 5 above, leaf 4 below: 4 backs off to 2 (estimate, stored twice), 5 is estimated at itself
    tree, plan = A.estimate_tree(classes, {1: 90.0, 2: 60.0, 3: 30.0, 4: 5.0, 5: 30.0}, lambda n: Ws[n], 10.0)
    assert plan == [(0, 3, 3, 0), (0, 2, 4, 0), (0, 5, 5, 0)] and np.array_equal(tree.map[5].W(), Ws[5])
    # nobody has enough: everything from node 1 -- the first leaf estimates there, the others copy
    tree, plan = A.estimate_tree(classes, {1: 9.0, 2: 6.0, 3: 3.0, 4: 3.0, 5: 3.0}, lambda n: Ws[n], 10.0)
    assert plan == [(0, 1, 3, 0), (0, 1, 4, 1), (0, 1, 5, 1)] and sorted(tree.map) == [1, 3, 4, 5]
    assert all(np.array_equal(tree.map[k].W(), Ws[1]) for k in tree.map)
    # the comparison is strict and against the float threshold
    tree, plan = A.estimate_tree([2, 3], {1: 20.0, 2: 10.0, 3: 10.000001}, lambda n: Ws[n], 10.0)
    assert plan == [(0, 1, 2, 0), (0, 3, 3, 0)]
    with pytest.raises(A.IndexError_):
        A.estimate_tree([1, 0], {1: 1.0}, lambda n: Ws[n], 0.0)


def test_transform_restated_in_float():
    rng = np.random.default_rng(9); D = 7
    W = np.concatenate([np.eye(D) + 0.3 * rng.standard_normal((D, D)), rng.standard_normal((D, 1))], axis=1)
    mu = rng.standard_normal((5, D)).astype(f32)
    out = A.transform_means(W, mu)
    for g in range(5):
        for m in range(D):
            comp = f32(W[m, D])
            for n in range(D):
                comp = f32(float(comp) + W[m, n] * float(mu[g, n]))
            assert out[g, m] == comp
    tree = A.ParamTree(); tree.findMLLR(2).assign(W); tree.findMLLR(7).assign(2 * W)
    new = A.transform_tree(tree, [2, 5, 7, 15, 4], mu)                                  # 5 -> 2, 15 -> 7, 4 -> 2
    assert np.array_equal(new[[0, 1, 4]], out[[0, 1, 4]]) and np.array_equal(new[[2, 3]], A.transform_means(2 * W, mu[[2, 3]]))
    with pytest.raises(A.KeyError_):
        A.transform_tree(tree, [3], mu[:1])                                             # 3 -> 1: not there
    with pytest.raises(A.IndexError_):
        A.transform_tree(tree, [0], mu[:1])


def test_codebook_file_restatement_carries_the_table():
    from tests import train_np as T
    m = T.random_model([2, 3], 4, seed=3)
    plain = A.codebook_file(m); tab = A.codebook_file(m, [1, 2, 3, 4, 5])
    per = 4 + 4 * 4 + 4 * 4 + 4
    assert len(tab) == len(plain) + 5 * 4 and len(plain) == 12 + 2 * (2 + 3 + 1 + 7 * 4 + 4) + 5 * per


def test_cpp_facade_adaptation_classes(tmp_path):
    """host/dsr_streams.hpp: ParamTree, CodebookSetAdapt, TransformerTree, adaptCbk, EstimatorTreeMLLR and estimateAdaptationParameters under
    the reference's names compile with plain g++; the parameter tree works without a device and the library's errors are mapped"""
    import os
    import subprocess
    from tests.conftest import PKG
    (tmp_path / "in.mllr").write_text(HAND)
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
int main(int argc, char** argv) {
  ParamTreePtr pt(new ParamTree(argv[1]));
  std::vector<double> W = pt->find(13);                       // 13 -> 6
  printf("tree %d %d %d %g %g\n", pt->type(), (int) pt->hasIndex(13), (int) pt->hasIndex(3), W[0], W[5]);
  pt->write(argv[2]);
  try { pt->find(0); } catch (jindex_error& e) { printf("zero %d\n", (int) e.getCode()); }
  try {
    VectorFloatFeatureStreamPtr s(new SampleFeature("", 320, 160));
    FeatureSetPtr fs(new FeatureSet()); fs->add(s);
    CodebookSetTrainPtr cbs(new CodebookSetTrain("", fs, "/nonexistent.cb", 3.0));
    try { adaptCbk(cbs, pt); } catch (jconsistency_error& e) { printf("nomodel %d\n", (int) e.getCode()); }
    try { cbs->setRegClasses(1); } catch (jconsistency_error& e) { printf("nomodel %d\n", (int) e.getCode()); }
    cbs->resetMean();
    EstimatorTreeMLLRPtr tree(new EstimatorTreeMLLR(cbs, pt, 1, 1500.0f));
    estimateAdaptationParameters(tree); tree->writeParams("/dev/null"); printf("%g\n", tree->ttlFrames()); tree->transform();
  } catch (j_error& e) { printf("err %d\n", (int) e.getCode()); }
  return 0;
}
""")
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(tmp_path / "in.mllr"), str(tmp_path / "out.mllr")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.strip().split("\n") if ln and ln != "Transforming Means"]
    assert lines == ["tree 3 1 0 0.333333 0.3", "zero 5", "nomodel 3", "nomodel 3", "err 3"], lines
    want = A.ParamTree(HAND); want.find(13)
    assert (tmp_path / "out.mllr").read_text() == want.text()
