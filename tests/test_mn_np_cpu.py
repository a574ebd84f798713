"""CPU tests of maximum negentropy beamforming and GG model training without a device: the deterministic fp64 log / exp / pow / digamma
(csrc/det_math.h, restated in tests/mn_np.py) against np.longdouble and, through the library, bit for bit against the restatement; the model's
constants, update and files; the device-order restatement within the derived bound of the reference-order one; refusals of the C-ABI."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dsr._mn as M                                        # the product: without it nothing here can pass
from tests import mk_cases, mk_np, mn_np

LD = np.longdouble
U53 = 2.0 ** -53
SHAPES_F = (0.07, 0.1, 0.5, 1.0, 1.5, 2.0)


@pytest.fixture(scope="module")
def mn(dsr):
    return M


def sweep_x():
    rng = np.random.default_rng(11)
    x = [10.0 ** rng.uniform(-90.0, 12.0, 4000), np.array([1.0, 1.0e-90, 1.0e12]), 2.0 ** np.arange(-298, 40, dtype=np.float64)]
    s = mn_np.SQRT_HALF
    edge = np.array([np.nextafter(s, 0.0), s, np.nextafter(s, 1.0), np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)])
    x += [edge * 2.0 ** k for k in (-200, -1, 0, 1, 2, 30)]
    return np.concatenate(x)


def test_det_log_and_pow_against_longdouble():
    x = sweep_x(); ref = np.log(x.astype(LD))
    err = np.abs(mn_np.det_log(x).astype(LD) - ref); rel = np.where(ref != 0, err / np.where(ref != 0, np.abs(ref), 1), err)
    print("det_log: largest relative error %.3f x 2^-53" % float(rel.max() / U53))
    assert mn_np.det_log(1.0) == 0.0 and (rel <= 4 * U53).all()
    worst = 0.0
    for f in SHAPES_F:
        refp = np.exp(LD(f) * ref)
        ok = (refp > 1e-300) & (refp < 1e300)
        got = mn_np.det_pow(x, f).astype(LD)
        ratio = np.abs(got - refp)[ok] / refp[ok] / mn_np.eps_pow(f, x)[ok].astype(LD)
        worst = max(worst, float(ratio.max()))
    print("det_pow: largest relative error / (4 (|f ln x| + 2) 2^-53): %.3f" % worst)
    assert worst <= 1.0
    assert mn_np.det_pow(0.0, 0.5) == 0.0 and np.isnan(mn_np.det_pow(-1.0, 0.5)) and mn_np.det_log(0.0) == -np.inf and np.isnan(mn_np.det_log(-1.0))
    assert mn_np.det_log(5e-324) == pytest.approx(math.log(5e-324), rel=1e-15)       # a subnormal


def test_det_exp_against_longdouble_and_at_the_limits():
    x = np.concatenate([np.random.default_rng(12).uniform(-708.0, 709.0, 4000), [-708.0, 708.0, 0.0, 709.0, 1e-300, -1e-300]])
    ref = np.exp(x.astype(LD)); got = mn_np.det_exp(x).astype(LD)
    rel = np.abs(got - ref) / ref
    print("det_exp: largest relative error %.3f x 2^-53" % float(rel.max() / U53))
    assert (rel <= 4 * U53).all()
    assert mn_np.det_exp(-710.0) == 0.0 and mn_np.det_exp(710.0) == np.inf and mn_np.det_exp(0.0) == 1.0 and np.isnan(mn_np.det_exp(np.nan))
    assert mn_np.det_exp(-np.inf) == 0.0 and mn_np.det_exp(np.inf) == np.inf


def psi_longdouble(x):
    x = LD(x); r = LD(0)
    while x < 40:
        r -= 1 / x; x += 1
    w = 1 / (x * x)
    return r + np.log(x) - 1 / (2 * x) - w * (LD(1) / 12 - w * (LD(1) / 120 - w * (LD(1) / 252 - w * (LD(1) / 240 - w * (LD(1) / 132)))))


def test_det_psi_against_a_longdouble_series():
    xs = np.linspace(0.5, 30.0, 60)
    rel = max(abs(LD(mn_np.det_psi(v)) - psi_longdouble(v)) / abs(psi_longdouble(v)) for v in xs)
    print("det_psi: largest relative error %.3g" % float(rel))
    assert rel <= 1e-13
    assert abs(mn_np.det_psi(1.0) + 0.5772156649015329) < 1e-15


def test_library_det_functions_equal_the_restatement_bit_for_bit(mn):
    x = sweep_x()
    assert np.array_equal(mn.det_log(x), mn_np.det_log(x))
    e = np.concatenate([np.random.default_rng(13).uniform(-720.0, 720.0, 4000), [-708.0, 708.0, 709.0, -710.0, 710.0, 0.0]])
    assert np.array_equal(mn.det_exp(e), mn_np.det_exp(e))
    ps = np.concatenate([np.linspace(0.05, 40.0, 500), 1.0 / np.array(SHAPES_F), 2.0 / np.array(SHAPES_F)])
    assert np.array_equal(mn.det_psi(ps), np.array([mn_np.det_psi(v) for v in ps]))
    assert mn.det_log(np.array([0.0]))[0] == -np.inf and np.isnan(mn.det_log(np.array([-1.0]))[0])
    with pytest.raises(mn.DsrError):
        mn.det_psi(np.array([0.0]))


def lib_constants(mn):
    """constants(p) for the restatements from the library's dsr_ggd_constants (its lgamma is the C library's, math.lgamma is Python's own)"""
    def constants(p):
        Bc, lNF, Ng, Ll = (float(v[0]) for v in mn.ggd_constants(np.array([p])))
        return dict(Bc=Bc, lNF=lNF, NgConst=Ng, LlConst=Ll, logBc=mn_np.det_log(Bc))
    return constants


def test_model_constants_against_lgamma(mn):
    """The constants against the same formulas with math.lgamma, each lgamma value allowed 4 ulp.  An ulp here is the spacing at max(1, |lgamma(1/p)|,
    |lgamma(2/p)|): Python's math.lgamma is an implementation of its own and carries an absolute error of that size where lgamma is small (against a
    200-bit evaluation it is off by up to 41 ulp of its own value at 1/p = 1.43, the C library's lgamma by at most 1.2).  lNF, NgConst and LlConst hold
    lgamma(1/p) twice and lgamma(2/p) once: 3 x 4 such ulp, plus 4 ulp of the constant for the other operations; Bc = exp(lgamma(1/p) - lgamma(2/p)):
    2 x 4 such ulp relative, plus 4 ulp."""
    p = np.array(SHAPES_F + (0.7, 0.33, 1.2))
    Bc, lNF, Ng, Ll = mn.ggd_constants(p)
    for i, v in enumerate(p):
        lg1, lg2 = math.lgamma(1 / v), math.lgamma(2 / v); lB = lg1 - lg2
        ulp4 = 4 * np.spacing(max(abs(lg1), abs(lg2), 1.0))
        want = (math.exp(lB), math.log(math.pi) + lg1 + lB)
        want += (want[1] - math.log(v) + 1 / v, math.log(v) - want[1])
        assert abs(Bc[i] - want[0]) <= want[0] * 2 * ulp4 + 4 * np.spacing(want[0]), (v, Bc[i], want[0])
        for got, w in zip((lNF[i], Ng[i], Ll[i]), want[1:]):
            assert abs(got - w) <= 3 * ulp4 + 4 * np.spacing(abs(w)), (v, got, w)
        c = mn_np.ggd_constants(v)                                    # the restatement with math.lgamma: the same bound
        assert abs(c["Bc"] - Bc[i]) <= Bc[i] * 2 * ulp4 + 4 * np.spacing(Bc[i]) and abs(c["NgConst"] - Ng[i]) <= 3 * ulp4 + 4 * np.spacing(abs(Ng[i]))
    with pytest.raises(mn.DsrError) as e:
        mn.ggd_constants(np.array([0.5, 0.0]))
    assert e.value.status == 13


def test_model_update_equals_the_restatement_bit_for_bit(mn):
    rng = np.random.default_rng(14); F = 9
    p = rng.uniform(0.2, 1.6, F); sa = rng.uniform(0.1, 3.0, F); n = 500.0
    acc = np.stack([rng.uniform(100, 900, F), rng.uniform(-300, 300, F), rng.uniform(100, 900, F), np.full(F, n), rng.uniform(-2000, -500, F)])
    acc[3, 4] = 0.0                                                   # a bin without a sample keeps its parameters
    acc[0, 5] = 1e-30                                                 # the variance floor
    for kw in (dict(), dict(nItr=3, alpha=1e-4), dict(alpha=1e-9), dict(alpha=1.0), dict(sigmaOnly=True), dict(floorP=5.0, alpha=1e-4)):
        got = mn.ggd_update(acc, p, sa, **kw); want = mn_np.ggd_update(acc, p, sa, constants=lib_constants(mn), **kw)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (kw, g, w)
        assert got[0][4] == sa[4] and got[1][4] == p[4] and got[0][5] == 10e-8
    assert mn.ggd_update(acc, p, sa, alpha=1e-9)[2][[0, 1, 2, 3, 5]].all()          # a step below thresh: converged
    assert not mn.ggd_update(acc, p, sa, sigmaOnly=True)[2].any() and np.array_equal(mn.ggd_update(acc, p, sa, sigmaOnly=True)[1], p)
    assert (mn.ggd_update(acc, p, sa, alpha=1.0)[1] >= 0.07).all() and (mn.ggd_update(acc, p, sa, floorP=5.0, alpha=1e-4)[1] == 5.0).any()


def test_parameter_and_accumulator_files(mn, tmp_path):
    from dsr.btk import GGDcEst as G
    a = G.MLE4CGGaussianD(p=0.43, sigma=1.7); a.fixConst()
    fn = str(tmp_path / "g.param"); a.writeParam(fn)
    lines = open(fn).read().split("\n")
    assert lines[0] == "%e %e %e" % (1.7, 0.43, 0.0) and lines[1] == "%e %e" % (a.getB(), a._lNF) and lines[2] == ""
    b = G.CGGaussianD(); assert b.readParam(fn) and not G.CGGaussianD().readParam(str(tmp_path / "missing"))
    assert b.getShapePar() == float("%e" % 0.43) and b.getScalingPar() == float("%e" % 1.7) and b.fixed()
    for v in (0.3 + 0.1j, 0.0, -2.0):
        a.acc(v)
    acc0 = a.accs()
    assert acc0[3] == 3 and np.array_equal(acc0, mn_np.ggd_acc_dev(np.array([0.3 + 0.1j, 0.0, -2.0], np.complex64)[None, :, None], [3], [0.43], [1.7], constants=lib_constants(mn))[:, 0])
    fa = str(tmp_path / "g.acc"); a._nItr = 1; a.writeAccs(fa)
    assert len(open(fa).read().strip().split("\n")) == 10 and open(fa).read().split("\n")[3] == "3"
    c = G.MLE4CGGaussianD(p=0.43, sigma=1.7); c.fixConst()
    assert c.readAccs(fa) and c.readAccs(fa)
    assert np.array_equal(c.accs(), 2 * np.array([float("%e" % v) for v in acc0]))
    a._nItr = 2; a.writeAccs(fa)
    assert not c.readAccs(fa) and np.array_equal(c.accs(), 2 * np.array([float("%e" % v) for v in acc0]))     # ignored
    assert G.CGGaussianD(p=0.5, sa=0.0).entropy(0) == G.LZERO
    with pytest.raises(mn.DsrError) as e:
        G.CGGaussianD(zeroMean=False, mean=0.1)
    assert e.value.status == 13


# ---- the restatements
@functools.lru_cache(maxsize=None)
def inputs(name):
    return mk_cases.case_inputs(name)


def shapes_of(F):
    """per-bin shape parameters spread over [0.1, 1.5], with exactly 1.0 (2f - 2 = 0) and one value above 1"""
    s = np.linspace(0.1, 1.5, F); s[F // 2] = 1.0
    return s


def problems(name, u, f, beta=0.5):
    inp = inputs(name); F = inp["F"]; sh = shapes_of(F)[f]; c = mn_np.ggd_constants(sh)
    sel = mk_np.select_frames(inp["sFrame"], inp["eFrame"], inp["R"], int(inp["nframes"][u]), inp["X"].shape[2])
    Xf = np.ascontiguousarray(inp["X"][u][:, sel, :][:, :, f].T) if sel else np.zeros((0, inp["C"]), np.complex64)
    r = mn_np.RefProblem(Xf, inp["wq"][f], inp["B"][f], 1.0e-2, beta, sh, c["Bc"], c["NgConst"])
    d = mn_np.DevProblem(Xf, inp["wq"][f], inp["B"][f], 1.0e-2, beta, sh, c["Bc"], c["NgConst"], c["logBc"])
    return r, d


@pytest.mark.parametrize("name", sorted(mk_cases.CASES))
def test_device_order_is_within_the_bound_of_reference_order(name):
    inp = inputs(name); n = inp["C"] - 1; rng = np.random.default_rng(5); worst = 0.0
    for u in (0, 2):
        for f in range(inp["F"]) if inp["C"] < 64 else (0, 1):
            r, d = problems(name, u, f)
            for scale in (0.1, 2.0):
                x = scale * rng.standard_normal(2 * n)
                fd, gd = d._eval(x, True)
                bc, bg = r.bound(x, inp["C"])
                worst = max(worst, abs(r._cost(x) - fd) / bc)
                gr = r._grad(x)
                worst = max(worst, np.max(np.abs(gr[0::2] - gd[0::2]) / bg), np.max(np.abs(gr[1::2] - gd[1::2]) / bg))
    print(name, "largest |ref - device order| / bound: %.4f" % worst)
    assert worst <= 1.0
    assert math.isnan(problems(name, 1, 0)[1]._eval(np.zeros(2 * n), True)[0])       # the empty utterance


def test_reference_gradient_is_half_the_real_gradient():
    r, _ = problems("c4_t63", 0, 2); n2 = 6; x = 0.1 * np.random.default_rng(6).standard_normal(n2); g = r._grad(x); h = 1e-6
    for i in range(n2):
        e = np.zeros(n2); e[i] = h
        fd = (r._cost(x + e) - r._cost(x - e)) / (2 * h)
        assert abs(fd - 2 * g[i]) <= 1e-7 * max(1.0, abs(fd)), (i, fd, g[i])


def test_a_frame_with_zero_output_is_counted_out():
    inp = inputs("c4_t63"); f = 1; sh = 0.6; c = mn_np.ggd_constants(sh)
    X = np.ascontiguousarray(inp["X"][0][:, :, f].T).copy(); X[3] = 0; X[40] = 0
    args = (X, inp["wq"][f], inp["B"][f], 1.0e-2, 0.5, sh, c["Bc"], c["NgConst"])
    x = 0.1 * np.random.default_rng(7).standard_normal(6)
    keep = [t for t in range(63) if t not in (3, 40)]
    for cls, extra in ((mn_np.RefProblem, ()), (mn_np.DevProblem, (c["logBc"],))):
        full = cls(*args, *extra)._grad(x)
        less = cls(X[keep], *args[1:], *extra)._grad(x)
        # without the two frames the sums are the same and T' = 61 both times, but sigma2 and Sf are means over T = 63 and 61 frames: the
        # data terms differ by the factor 63 / 61 (by 1 if the zero frames were counted into T' as well)
        assert np.allclose(full - 1.0e-2 * x, (less - 1.0e-2 * x) * (63.0 / 61.0), rtol=1e-11, atol=1e-14)
    assert np.isnan(mn_np.DevProblem(np.zeros_like(X), *args[1:], c["logBc"])._eval(x, True)[0])
    res = mn_np.minimize(mn_np.DevProblem(np.zeros_like(X), *args[1:], c["logBc"]), np.zeros(6))
    assert res["reason"] == mk_np.SKIPPED and res["evals"] == 1


def test_minimiser_runs_on_both_orders_and_lowers_the_cost():
    r, d = problems("c4_t63", 0, 2)
    f0 = d._cost(np.zeros(6))
    rd = mn_np.minimize(d, np.zeros(6)); rr = mn_np.minimize(r, np.zeros(6))
    assert rd["reason"] != mk_np.SKIPPED and rd["f"] <= f0 and rr["f"] <= f0 and rd["iters"] >= 1
    assert abs(rd["f"] - rr["f"]) < 1e-3


def gg_samples(p, sa, n, rng):
    """complex GG samples: |X|^2 = Bc sa G^(1/p) with G ~ Gamma(1/p), a uniform phase"""
    r2 = mn_np.ggd_constants(p)["Bc"] * sa * rng.gamma(1.0 / p, 1.0, n) ** (1.0 / p)
    return (np.sqrt(r2) * np.exp(1j * rng.uniform(0, 2 * np.pi, n))).astype(np.complex64)


@pytest.mark.parametrize("ptrue,step,tol", [(0.5, 1.0, 0.0453), (1.0, 2.0, 0.0693)])
def test_training_recovers_the_shape_of_gg_samples(ptrue, step, tol):
    """20 000 samples of shape ptrue and scaling 2, start (p, sa) = (0.7, 1), up to 200 updates with alpha = step / nSample (update() does not
    divide its gradient by the sample count).  Measured with this restatement over the seeds 100..107: p = 0.5 gives 0.4998 .. 0.5148 (spread
    0.0151, mean 0.5074), p = 1.0 gives 0.9745 .. 0.9976 (spread 0.0231, mean 0.9881); the tolerance is three times the spread."""
    n = 20000; X = gg_samples(ptrue, 2.0, n, np.random.default_rng(100))[None, :, None]
    p = np.array([0.7]); sa = np.array([1.0])
    for it in range(200):
        sa, p, cv = mn_np.ggd_update(mn_np.ggd_acc_dev(X, [n], p, sa), p, sa, nItr=it, alpha=step / n)
        if cv.all():
            break
    print("shape %.1f recovered as %.4f, scaling 2 as %.4f after %d updates" % (ptrue, p[0], sa[0], it + 1))
    assert abs(p[0] - ptrue) <= tol


def test_refusals_through_the_c_abi(mn):
    L = mn.load(); h = C.c_void_p()
    for args, status in (((8, 4, 2, 1, 0), 1), ((8, 4, 1, 2, 0), 13), ((8, 4, 1, 1, 1), 1), ((8, 1, 1, 1, 0), 5), ((8, 65, 1, 1, 0), 5)):
        assert L.dsr_mn_create(*args, C.byref(h)) == status, args
    assert L.dsr_mn_create(8, 4, 2, 1, 0, C.byref(h)) == 1 and L.dsr_last_error() == b"not yet implemented in the case of NC > 2 (NC = 2)"
    assert L.dsr_mn_create(8, 4, 1, 1, 1, C.byref(h)) == 1 and L.dsr_last_error() == b"not support halfBandShift==True yet"
    b = mn.MnBeamformer(8, 4)
    for bad in ([0.5, 0.5, 0.0, 0.5, 0.5], [0.5, -1.0, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, np.inf, 0.5], [np.nan] * 5):
        with pytest.raises(mn.DsrError) as e:
            b.setGGD(bad)
        assert e.value.status == 13
    buf = np.zeros(4096); ptr = buf.ctypes.data_as(C.c_void_p)

    def estimate():
        return L.dsr_mn_estimate(b.h, ptr, None, 1, 3, 0, 3, 1, -1, ptr, ptr, ptr, None)
    assert estimate() == 1 and b"dsr_mn_set_ggd" in L.dsr_last_error()                 # before the model
    b.setGGD([0.5] * 5)
    assert estimate() == 1 and b"setFixedWeights" in L.dsr_last_error()               # before the fixed weights
    b.setFixedWeights(np.ones((5, 4)) / 4)
    assert L.dsr_mn_estimate(b.h, ptr, None, 1, 3, 0, 3, 1, 5, ptr, ptr, ptr, None) == 6      # fbinX >= F
    Bc, Ng, lB = b.getConstants(); c = lib_constants(mn)(0.5)
    assert Bc[0] == c["Bc"] and Ng[2] == c["NgConst"] and lB[4] == c["logBc"]
    assert L.dsr_ggd_write_param(b"/nonexistent-dir/x", 1.0, 0.5, 0.25) == 13          # a mean that is not zero


def test_importing_the_binding_imports_no_torch():
    import subprocess
    import sys
    from tests.conftest import PKG
    code = "import sys; sys.path.insert(0, %r); import dsr._mn, dsr.btk.mnBeamforming, dsr.btk.GGDcEst; assert 'torch' not in sys.modules; print('ok')" % PKG
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
