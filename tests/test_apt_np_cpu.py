"""CPU tests of the all-pass transforms: properties of the numpy restatement (tests/apt_np.py), and the library's host code -- the RAPT / SLAPT
parameter reader and writer and the line search of csrc/apt.cpp -- against it."""
import numpy as np
import pytest

from tests import adapt_np as A
from tests import apt_cases as Cs
from tests import apt_np as P

f32 = np.float32


def _file(tmp_path, name, text):
    p = tmp_path / name; p.write_text(text); return str(p)


def test_identity_and_first_column():
    for L in (2, 13, 17):
        assert np.array_equal(P.matrix(P.RAPT, [0.0], L), np.eye(L)) and np.array_equal(P.matrix(P.SLAPT, [0.0], L), np.eye(L))
    e0 = np.zeros(13); e0[0] = 1.0
    for alpha in Cs.BLT_ALPHAS:
        assert np.array_equal(P.matrix(P.RAPT, [alpha], 13) @ e0, e0)          # c_0 maps to itself: column 0 is the unit sample sequence
    with pytest.raises(A.ParameterError):
        P.bilinear(1.0)


@pytest.mark.parametrize("kind, params", [(P.RAPT, (a,)) for a in Cs.BLT_ALPHAS] + [(P.SLAPT, p) for p in Cs.SLAPT_PARAMS])
def test_mapped_point_is_on_the_unit_circle(kind, params):
    """an all-pass function maps the unit circle to itself (_calcMappedPoint, tr:1199-1210); 150 coefficients a side hold it to 1e-9.  The
    bilinear series is geometric, so what the cut after z^149 drops is (1 + |alpha|) |alpha|^149: above 1e-9 only at the edge of the search
    range, alpha = -0.899, where that tail is the bound"""
    seq = P.calc_sequence(kind, params)
    tail = (1.0 + abs(params[0])) * abs(params[0]) ** 149 if kind == P.RAPT else 0.0
    assert tail < 1.0e-9 or params[0] == -0.899
    for omega in np.linspace(0.0, np.pi, 17):
        assert abs(abs(P.mapped_point(np.exp(1j * omega), seq)) - 1.0) <= max(1.0e-9, tail)


def test_shift_keeps_the_first_element():
    """shift (tr:78-83) moves every coefficient up by one and leaves element -last as it was"""
    seq = P.slapt_sequence([0.2]); e = P.e_coefficients()
    assert e[0] == 1.0 and e[1] == 1.0 and e[2] == 0.5 and e[3] == 0.5 / 3
    assert seq[0] == seq[1]


@pytest.mark.parametrize("kind", [P.RAPT, P.SLAPT])
@pytest.mark.parametrize("biasType", [P.NONE, P.CEPSTRA_ONLY, P.ALL_COMPONENTS])
def test_likelihood_does_not_go_down(kind, biasType):
    L, nSub = 13, 3
    m, classes = Cs.model(L, nSub, [65], [1], seed=3)
    c, sumO = Cs.stats(m, 1, seed=4)
    st = P.Stats(m.mean, m.cv, c[0], sumO[0], range(m.G), L, nSub, biasType)
    x, bias, pts, vals = P.estimate_node(kind, st)
    assert len(bias) == P.bias_size(biasType, L, nSub) and 3 <= len(pts) <= 40
    assert max(vals) >= vals[0] and P.calc_log_lhood(kind, x, st) == max(vals)
    assert P.calc_log_lhood(kind, x, st) >= P.calc_log_lhood(kind, 0.0, st)                 # the start point b = 0 of either search
    assert P.lhood_bound(kind, x, st) < 1.0e-3 * abs(max(vals))


@pytest.mark.parametrize("kind", [P.RAPT, P.SLAPT])
@pytest.mark.parametrize("shape", Cs.RECOVERY_SHAPES)
def test_recovery_condition_on_the_restatement(kind, shape):
    """statistics made with A(alpha*) and no bias give alpha* back to within the interval Brent's method stops at"""
    L, nSub, G = shape
    m, _ = Cs.model(L, nSub, [G], [1], seed=5, decay=True)
    for alpha in Cs.RECOVERY_ALPHAS:
        c, sumO = Cs.recovery_stats(kind, m, L, nSub, alpha, seed=9)
        st = P.Stats(m.mean, m.cv, c, sumO, range(m.G), L, nSub, P.NONE)
        x, _, pts, _ = P.estimate_node(kind, st)
        assert abs(x - alpha) <= Cs.recovery_bound(alpha), (alpha, x)
        assert len(pts) <= 16


# ---- the library's host code ------------------------------------------------------------------------------------------------------------------
def _functions():
    rng = np.random.default_rng(11); fs = []
    for _ in range(12):
        x0 = rng.uniform(-0.6, 0.6); w = rng.uniform(0.5, 20.0); q = rng.uniform(-3.0, 3.0)
        fs.append(lambda x, x0=x0, w=w, q=q: -w * (x - x0) ** 2 + q * (x - x0) ** 3 - 2.0)
    fs.append(lambda x: x)                                                      # rising over the whole range: bracket runs into the bound
    fs.append(lambda x: -x)
    fs.append(lambda x: -abs(x) ** 0.5)
    fs.append(lambda x: np.cos(9.0 * x))
    return fs


@pytest.mark.parametrize("kind", [P.RAPT, P.SLAPT])
def test_line_search_visits_the_restatements_points(dsr, kind):
    """csrc/apt.cpp's bracket + brentsMethod, fed the values of a function point by point, asks for the restatement's points bit for bit"""
    for f in _functions():
        x, pts, vals = P.line_search(kind, f)
        got = []; state, point, _ = dsr.apt_line_search(kind, got)
        while state == 0:
            assert len(got) < len(pts) and np.float64(point).tobytes() == np.float64(pts[len(got)]).tobytes()
            got.append(vals[len(got)])
            state, point, seen = dsr.apt_line_search(kind, got)
        assert state == 1 and len(got) == len(pts) and np.float64(point).tobytes() == np.float64(x).tobytes()
        assert seen.tobytes() == np.array(pts).tobytes()


@pytest.mark.parametrize("kind", [P.RAPT, P.SLAPT])
def test_line_search_fails_on_a_nan_in_bracket(dsr, kind):
    for n in range(3):                                                          # bracket's three checked evaluations (eA:122-130)
        vals = [-1.0 - k for k in range(n)] + [float("nan")]
        assert dsr.apt_line_search(kind, vals)[0] == 2
        with pytest.raises(P.NotANumber):
            P.line_search(kind, lambda x, it=iter(vals): next(it))
    # a NaN after bracket's checks is not looked at (eA:132-240): every comparison with it is false, and both searches walk the same points
    f = lambda x, seen=[]: (seen.append(x), float("nan") if len(seen) > 3 else (-1.0, -2.0, -1.5)[len(seen) - 1])[1]      # noqa: E731
    x, pts, vals = P.line_search(kind, f)
    state, point, seen = dsr.apt_line_search(kind, vals)
    assert state == 1 and seen.tobytes() == np.array(pts).tobytes() and np.float64(point).tobytes() == np.float64(x).tobytes()


def test_parameter_files_round_trip(dsr, tmp_path):
    rng = np.random.default_rng(2)
    for typ, nConf in ((P.RAPT, 1), (P.RAPT, 5), (P.SLAPT, 1), (P.SLAPT, 4)):
        ref = P.Params(); t = dsr.AptParams()
        for rc, nb in ((0 + 4, 0), (1, 13), (6, 39), (3, 2)):
            conf = rng.uniform(-0.5, 0.5, nConf) * np.array([1.0e-7, 1.0, 123456.789, -1.0, -1.0e5][:nConf])
            bias = (rng.standard_normal(nb) * 10.0 ** rng.integers(-8, 8, nb)).astype(f32)
            p = ref.findAPT(rc, typ); p.conf = conf; p.bias = bias
            t.set(rc, typ, conf, bias)
        out = str(tmp_path / "a.par"); t.write(out); text = open(out).read()
        assert text == ref.text() and t.type() == typ and t.indices() == [1, 3, 4, 6]
        back = dsr.AptParams(out); again = P.Params(text)                       # %g keeps six digits: the second pass is a fixed point
        out2 = str(tmp_path / "b.par"); back.write(out2)
        assert open(out2).read() == again.text() and back.type() == again.type == typ
        for rc in back.indices():
            conf, bias = back.findAPT(rc, typ, False)
            assert np.array_equal(conf, again.map[rc].conf) and np.array_equal(bias, again.map[rc].bias) and bias.dtype == f32


def test_rapt_writes_fabs_of_even_parameters_and_class_zero_as_one(dsr, tmp_path):
    ref = P.Params(); p = ref.findAPT(2, P.RAPT); p.conf = np.array([-0.1, -0.2, -0.3, -0.4, -0.5]); p.regClass = 0
    want = "<AdaptType> RAPT\n<RegClass> 1\n<RAPTParam> 5\n -0.1 -0.2 0.3 -0.4 0.5\n<EndClass>\n"
    assert ref.text() == want
    t = dsr.AptParams(_file(tmp_path, "z.par", "<AdaptType> RAPT\n<RegClass> 0\n<RAPTParam> 5\n -0.1 -0.2 -0.3 -0.4 -0.5\n<EndClass>\n"))
    out = str(tmp_path / "o.par"); t.write(out)
    assert open(out).read() == want and t.indices() == [0]


def test_find_apt(dsr):
    t = dsr.AptParams(); ref = P.Params()
    t.set(2, P.SLAPT, [0.25], [1.0, 2.0]); p = ref.findAPT(2, P.SLAPT); p.conf = np.array([0.25]); p.bias = np.array([1.0, 2.0], f32)
    conf, bias = t.findAPT(5, P.SLAPT); q = ref.findAPT(5, P.SLAPT)             # a copy of the nearest ancestor
    assert np.array_equal(conf, q.conf) and np.array_equal(bias, q.bias) and t.indices() == sorted(ref.map)
    conf, bias = t.findAPT(3, P.SLAPT); q = ref.findAPT(3, P.SLAPT)             # no ancestor: an empty parameter
    assert len(conf) == 0 and len(bias) == 0 and len(q.conf) == 0
    for args, exc in (((7, P.RAPT), A.ConsistencyError), ((0, P.SLAPT), A.IndexError_), ((9, P.SLAPT, False), A.IndexError_)):
        with pytest.raises(exc):
            ref.findAPT(*args)
        with pytest.raises(dsr.DsrError) as e:
            t.findAPT(*args)
        assert e.value.status == (dsr.E_CONSISTENCY if exc is A.ConsistencyError else dsr.E_INDEX)


@pytest.mark.parametrize("text, status, exc", [
    ("<AdaptType> MLLR\n<RegClass> 1\n<MLLRParam> 1\n 1\n<EndClass>\n", 13, A.ParameterError),             # an MLLR block: dsr_param_tree reads those
    ("<RegClass> 1\n<EndClass>\n", 15, A.TypeError_),                                                      # "Unable to determine adaptation type."
    ("<AdaptType> RAPT\n<RegClass> 1\n<SLAPTParam> 1\n 0.1\n<EndClass>\n", 13, A.ParameterError),          # "Attempted to read RAPT parameters."
    ("<AdaptType> RAPT\n<RegClass> 1\n<MLLRParam> 1\n 0.1\n<EndClass>\n", 13, A.ParameterError),
    ("<AdaptType> SLAPT\n<RegClass> 1\n<RAPTParam> 1\n 0.1\n<EndClass>\n", 13, A.ParameterError),          # "Attempted to read SLAPT parameters."
    ("<AdaptType> SLAPT\n<AdaptType> RAPT\n<EndClass>\n", 13, A.ParameterError),                          # type consistency inside a class
    ("<AdaptType> SLAPT\n<RegClass> 1\n<STCParam> 1\n<EndClass>\n", 13, A.ParameterError),                 # unexpected symbol
    ("<AdaptType> SLAPT\n<RegClass> 1\n<SLAPTParam> 1\n 0.1\n<EndClass>\n<AdaptType> RAPT\n<RegClass> 2\n<RAPTParam> 1\n 0.1\n<EndClass>\n", 4,
     A.ConsistencyError),                                                                                  # both types in one file
])
def test_wrong_type_files_raise(dsr, tmp_path, text, status, exc):
    with pytest.raises(exc):
        P.Params(text)
    t = dsr.AptParams(); t.set(2, P.SLAPT, [0.5])
    with pytest.raises(dsr.DsrError) as e:
        t.read(_file(tmp_path, "bad.par", text))
    assert e.value.status == status
    assert t.indices() == []                                                    # read clears first (tr:927-929)


def test_free_layout(dsr, tmp_path):
    text = "\n <AdaptType>SLAPT <RegClass>3\n<SLAPTParam>  2\n0.5\n\n-2e-3 <BiasOffset> 2 1 2<EndClass>"
    ref = P.Params(text); t = dsr.AptParams(_file(tmp_path, "free.par", text))
    want = "<AdaptType> SLAPT\n<RegClass> 3\n<SLAPTParam> 2\n 0.5 -0.002\n<BiasOffset> 2\n 1 2\n<EndClass>\n"
    out = str(tmp_path / "out.par"); t.write(out)
    assert ref.text() == want and open(out).read() == want
    # the SLAPT type reads an <MLLRParam> symbol as its own parameters (tr:397-400 refuses it for RAPT only)
    text = "<AdaptType> SLAPT\n<RegClass> 1\n<MLLRParam> 1\n 0.1\n<EndClass>\n"
    assert P.Params(text).map[1].conf[0] == 0.1 and dsr.AptParams(_file(tmp_path, "m.par", text)).findAPT(1, P.SLAPT, False)[0][0] == 0.1


def test_cpp_facade_apt_classes(tmp_path):
    """host/dsr_streams.hpp: APTParamTree, RAPTParam, SLAPTParam, BLTTransformer, SLAPTTransformer, EstimatorTreeSLAPT / EstimatorTreeBLT and
    estimateAdaptationParameters under the reference's names compile with plain g++; the parameters work without a device and the library's
    errors are mapped"""
    import os
    import subprocess
    from tests.conftest import PKG
    text = "<AdaptType> SLAPT\n<RegClass> 6\n<SLAPTParam> 1\n 0.25\n<BiasOffset> 2\n 1 2\n<EndClass>\n"
    (tmp_path / "in.par").write_text(text)
    src = tmp_path / "t.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
int main(int argc, char** argv) {
  APTParamTreePtr pt(new APTParamTree(argv[1]));
  std::vector<double> conf; std::vector<float> bias;
  pt->findAPT(13, APT_SLAPT, conf, bias);                     // 13 -> 6
  printf("tree %d %d %d %g %g\n", pt->type(), (int) conf.size(), (int) bias.size(), conf[0], bias[1]);
  pt->write(argv[2]);
  try { pt->findAPT(3, APT_RAPT, conf, bias); } catch (jconsistency_error& e) { printf("type %d\n", (int) e.getCode()); }
  RAPTParam(0.5, std::vector<float>(2, 1.5f), 4).write(argv[3]);
  SLAPTParam par(std::vector<double>(2, 0.1));
  printf("par %u %g %u\n", par.size(), par[1], par.regClass());
  try {
    VectorFloatFeatureStreamPtr s(new SampleFeature("", 320, 160));
    FeatureSetPtr fs(new FeatureSet()); fs->add(s);
    CodebookSetTrainPtr cbs(new CodebookSetTrain("", fs, "/nonexistent.cb", 3.0));
    cbs->setSubFeatures(13, 3);
    try { adaptCbk(cbs, pt); } catch (jconsistency_error& e) { printf("nomodel %d\n", (int) e.getCode()); }
    try { EstimatorTreeSLAPTPtr t(new EstimatorTreeSLAPT(cbs, pt, "Nonsense")); } catch (jtype_error& e) { printf("bias %d\n", (int) e.getCode()); }
    try { EstimatorTreeBLTPtr t(new EstimatorTreeBLT(cbs, pt)); estimateAdaptationParameters(t); } catch (jconsistency_error& e) { printf("nomodel %d\n", (int) e.getCode()); }
    try { BLTTransformer tr(RAPTParam(0.1), 13, 3); tr.transform(std::vector<float>(39, 1.0f)); SLAPTTransformer t2(par, 13); } catch (j_error& e) { printf("nodevice %d\n", (int) e.getCode()); }
  } catch (j_error& e) { printf("err %d\n", (int) e.getCode()); }
  return 0;
}
""")
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(tmp_path / "in.par"), str(tmp_path / "out.par"), str(tmp_path / "rapt.par")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.strip().split("\n") if ln and ln != "Transforming Means"]
    assert lines[:6] == ["tree 2 1 2 0.25 2", "type 3", "par 2 0.1 0", "nomodel 3", "bias 14", "nomodel 3"], lines
    assert len(lines) == 6 or lines[6:] == ["nodevice 6"]                                # JINITIALIZATION where there is no HIP device
    ref = P.Params(text); ref.findAPT(13, P.SLAPT)
    assert open(tmp_path / "out.par").read() == ref.text()
    assert open(tmp_path / "rapt.par").read() == "<AdaptType> RAPT\n<RegClass> 4\n<RAPTParam> 1\n 0.5\n<BiasOffset> 2\n 1.5 1.5\n<EndClass>\n"
