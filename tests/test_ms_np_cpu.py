"""CPU tests of multi-stream decoding (include/dsr.h section 8b): the numpy restatement against an element-by-element loop, the DistribMap C-ABI
against the restatement (needs no device), the dispatch query, the near-cancellation set that tells a fused multiply-add from the reference's
arithmetic, and the C++ facade's host-only part."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ms_cases, ms_np
from tests.conftest import ROOT, PKG

# (KA, KV) of the LDS paths and the rows of the gather shape, as tests/test_gpu_multistream.py uses them
LDS_SHAPES = [(1, 1), (5, 3), (24, 6), (260, 7), (24, 24)]


@pytest.fixture(scope="module")
def ms(dsr):
    import dsr._ms as M
    return M


def test_combine_against_a_python_loop():
    rng = np.random.default_rng(3)
    sA, sV = ms_cases.scores(rng, (7, 5)), ms_cases.scores(rng, (7, 3))
    table = np.array([2, 0, 0, 1, 2], np.int32)
    for wA, wV in ms_cases.WEIGHTS:
        got = ms_np.combine(sA, sV, table, wA, wV)
        assert got.dtype == np.float32 and got.shape == sA.shape
        for n in range(7):
            for k in range(5):
                p = float(wA) * float(sA[n, k]); q = float(wV) * float(sV[n, table[k]])          # Python floats are doubles: two products,
                assert got[n, k] == np.float32(p + q)                                          # one sum, one rounding
    assert np.array_equal(ms_np.combine(sA, sV, table, 1.0, 0.0), sA)


def test_resolve_and_its_two_errors():
    A, V = ["a", "b", "c"], ["x", "b", "a", "c", "a"]
    assert list(ms_np.resolve(A, V)) == [2, 1, 3]
    assert list(ms_np.resolve(A, V, {"a": "x", "b": "x", "c": "b"})) == [0, 0, 1]
    with pytest.raises(ms_np.MsError) as e:
        ms_np.resolve(A, ["a", "b"])
    assert e.value.status == 11
    with pytest.raises(ms_np.MsError) as e:
        ms_np.resolve(A, V, {"a": "x", "b": "x"})
    assert e.value.status == 6
    with pytest.raises(ms_np.MsError) as e:
        ms_np.resolve(A, V, {"a": "x", "b": "x", "c": "nope"})
    assert e.value.status == 11


def test_distribmap_file_is_the_restatements(ms, dsr, tmp_path):
    pairs = [("ds9", "v1"), ("ds10", "v0"), ("Zed", "v2"), ("ds9", "v3"), ("", "v0"), ("a" * 19, "b" * 19)]      # unsorted, one overwrite
    ref = {}
    m = ms.DistribMap()
    for f, t in pairs:
        m.add(f, t); ref[f] = t
    assert len(m) == len(ref) == 5 and m.mapped("ds9") == "v3"
    p = str(tmp_path / "m.bin"); m.write(p)
    data = open(p, "rb").read()
    assert data == ms_np.distribmap_bytes(ref) and ms_np.parse_distribmap(data) == ref
    assert data[:4] == b"\0\0\0\5" and data[4:7] == b"\0\0\0"                          # the count, then the empty name: length 0 and its NUL
    # read -> write round trip; read clears what the map held
    r = ms.DistribMap({"old": "gone"}); r.read(p)
    assert len(r) == 5 and {k: r.mapped(k) for k in ref} == ref
    with pytest.raises(dsr.DsrError) as e:
        r.mapped("old")
    assert e.value.status == 6 and "No mapping for old" in str(e.value)
    q = str(tmp_path / "q.bin"); r.write(q)
    assert open(q, "rb").read() == data
    # a file the restatement wrote reads back to the same map
    other = {"k%d" % i: "t%d" % (i % 3) for i in range(12)}
    open(tmp_path / "o.bin", "wb").write(ms_np.distribmap_bytes(other))
    r.read(str(tmp_path / "o.bin"))
    assert len(r) == 12 and {k: r.mapped(k) for k in other} == other


def test_distribmap_errors(ms, dsr, tmp_path):
    L = dsr.load()
    m = ms.DistribMap()
    m.add("f" * 19, "t" * 19)                                                          # 19 characters fit the reference's char[20]
    for f, t in (("f" * 20, "t"), ("f", "t" * 20)):
        with pytest.raises(dsr.DsrError) as e:
            m.add(f, t)
        assert e.value.status == 13
    assert len(m) == 1
    long = {"x" * 20: "y"}
    open(tmp_path / "long.bin", "wb").write(ms_np.distribmap_bytes(long))
    with pytest.raises(dsr.DsrError) as e:
        m.read(str(tmp_path / "long.bin"))
    assert e.value.status == 13 and len(m) == 1                                        # refused, and the map is as it was
    with pytest.raises(dsr.DsrError) as e:
        m.read(str(tmp_path / "missing.bin"))
    assert e.value.status == 8
    with pytest.raises(dsr.DsrError) as e:
        m.write(str(tmp_path / "no" / "such" / "dir.bin"))
    assert e.value.status == 8
    for call in (m.read, m.write):
        with pytest.raises(dsr.DsrError) as e:
            call("")
        assert e.value.status == 1 and "Distribution map file name is null." in str(e.value)
    h = C.c_void_p(); to = C.c_char_p()
    for st in (L.dsr_distribmap_create(None), L.dsr_distribmap_add(None, b"a", b"b"), L.dsr_distribmap_add(m.h, None, b"b"),
               L.dsr_distribmap_add(m.h, b"a", None), L.dsr_distribmap_mapped(m.h, b"a", None), L.dsr_distribmap_mapped(None, b"a", C.byref(to)),
               L.dsr_distribmap_read(m.h, None), L.dsr_distribmap_write(None, b"x"), L.dsr_ms_create(None, None, None, 0.5, 0.5, C.byref(h)),
               L.dsr_ms_combine(None, None, None, 1, None, None), L.dsr_ms_combine_path(4, 4, 1, None, None, None),
               L.dsr_distribset_create_multistream(None, None, None, 0.5, 0.5, C.byref(h)), L.dsr_distribset_set_weights(None, 0.5, 0.5)):
        assert st == 13 and L.dsr_last_error() == b"null argument"
    assert L.dsr_distribmap_size(None) == 0


def test_combine_path_reaches_every_path(ms):
    budget = ms.LDS_BUDGET
    seen = set()
    for KA, KV in LDS_SHAPES:
        for aligned in (True, False):
            path, rows, lds = ms.combine_path(KA, KV, aligned)
            assert path == (ms.VECTOR_LDS if KA % 4 == 0 and aligned else ms.SCALAR_LDS), (KA, KV, aligned)
            assert 1 <= rows <= 16 and rows * KV * 4 <= budget and rows * KV * 4 + 12 <= lds <= budget + 32 and lds % 16 == 0
            seen.add(path)
    assert ms.combine_path(8, budget // 4, True)[0] == ms.VECTOR_LDS and ms.combine_path(8, budget // 4, True)[1] == 1
    path, rows, lds = ms.combine_path(8, budget // 4 + 1, True)                        # one video row alone exceeds the budget
    assert path == ms.GATHER and lds == 0 and rows >= 1
    seen.add(path)
    assert seen == {ms.VECTOR_LDS, ms.SCALAR_LDS, ms.GATHER}
    assert ms.combine_path(1024, 1024, True)[:2] == (ms.VECTOR_LDS, 2) and ms.combine_path(1024, 64, True)[1] == 4 and ms.combine_path(1023, 64, True)[0] == ms.SCALAR_LDS


@pytest.mark.parametrize("wA,wV", ms_cases.FMA_WEIGHTS)
def test_cancellation_set_tells_a_fused_multiply_add(wA, wV):
    c = ms_cases.fma_case(wA, wV)
    table = np.arange(ms_cases.FMA_COLS, dtype=np.int32)
    assert np.array_equal(ms_np.combine(c["a"], c["v"], table, wA, wV), c["unfused"])        # numpy's three rounded steps = exact arithmetic's
    nA = int((c["fmaA"] != c["unfused"]).sum()); nV = int((c["fmaV"] != c["unfused"]).sum())
    print("weights (%g, %g): %d of %d differ under fma(wA, a, .), %d under fma(wV, v, .)" % (wA, wV, nA, c["a"].size, nV))
    assert nA >= 64 and nV >= 64


def test_cpp_facade_multistream_classes(tmp_path):
    """DistribMap / DistribSetMultiStream in host/dsr_streams.hpp with the reference's constructor order (distribBasic.cc:381-410), compiled with
    plain g++; the host-only part runs: a DistribMap round trip and its key error."""
    src = tmp_path / "m.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
#include <cstdio>
int main(int argc, char** argv) {
  DistribMapPtr m(new DistribMap());
  m->add("b", "y"); m->add("a", "x"); m->add("b", "z");
  m->write(argv[1]);
  DistribMapPtr r(new DistribMap()); r->add("q", "q"); r->read(argv[1]);
  printf("map %u %s %s\n", r->size(), r->mapped("a").c_str(), (*r).mapped("b").c_str());
  try { r->mapped("q"); } catch (jindex_error& e) { printf("index %d %s\n", (int) e.getCode(), e.what()); }
  try { m->add("12345678901234567890", "x"); } catch (jparameter_error& e) { printf("param %d\n", (int) e.getCode()); }
  try {
    VectorFloatFeatureStreamPtr s(new SampleFeature("", 320, 160));
    FeatureSetPtr fs(new FeatureSet()); fs->add(s);
    CodebookSetBasicPtr cbs(new CodebookSetBasic("", fs, "/nonexistent.cb"));
    DistribSetBasicPtr a(new DistribSetBasic(cbs, "", "/nonexistent.ds")), v(new DistribSetBasic(cbs, "", "/nonexistent.ds"));
    DistribSetMultiStreamPtr byName(new DistribSetMultiStream(a, v, 0.9, 0.1));
    DistribSetMultiStreamPtr dss(new DistribSetMultiStream(a, v, m, 0.9, 0.1));
    dss->setWeights(1.0, 0.0); dss->find(0u).audioWeight(); dss->find("a").score(0); dss->resetCache(); dss->resetFeature();
    DecoderFlyWeightPtr d(new DecoderFlyWeight(dss, 100.0, 12.0, 0.0, 0.0, "SIL-m", "</s>", 5000, 0, true));
    d->decode(); LatticePtr l = d->lattice(); l->gammaProbsDist(dss);
  } catch (j_error& e) { printf("err %d\n", (int) e.getCode()); }
  return 0;
}
""")
    exe = tmp_path / "m"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    f = tmp_path / "map.bin"
    out = subprocess.run([str(exe), str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "map 2 x z" and lines[1] == "index 5 No mapping for q" and lines[2] == "param 12"
    assert lines[3] in ("err 7", "err 6")                                # the model files do not exist (JIO) / no device (JINITIALIZATION)
    assert f.read_bytes() == ms_np.distribmap_bytes({"a": "x", "b": "z"})
