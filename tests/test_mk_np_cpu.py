"""The numpy restatements of maximum empirical kurtosis beamforming (tests/mk_np.py) against each other and against what they claim: the packed
gradient is half the real gradient, the reference's order and the device's order agree to a derived rounding bound, the weights found lower the
interferer's power, and every case named for a branch of the minimisers takes that branch."""
import numpy as np
import pytest

from tests import mk_cases, mk_np

bound_factor = mk_np.bound_factor


def test_packed_gradient_is_half_the_real_gradient():
    """central difference (h = 1e-6, no normalisation) over the reference's packed gradient = 2, to 1e-5 relative (of the largest entry)"""
    h = 1.0e-6
    for name in ("c2_t1", "c4_t63", "c8_t65"):
        inp = mk_cases.case_inputs(name)
        for f in (1, inp["F"] - 1):
            p = mk_cases.problem(mk_np.RefProblem, mk_np.PR, inp, 0, f)
            x = 0.1 * np.random.default_rng(5).standard_normal(2 * (inp["C"] - 1))
            g = p._grad(x)
            fd = np.zeros_like(g)
            for i in range(len(x)):
                e = np.zeros_like(x); e[i] = h
                fd[i] = (p._cost(x + e) - p._cost(x - e)) / (2 * h)
            ratio = fd / g
            print(name, f, "central difference / packed gradient:", ratio)
            assert np.abs(fd - 2.0 * g).max() <= 1.0e-5 * np.abs(2.0 * g).max(), (name, f, ratio)


def ref_dev_ratio(inp, kind, u, f, x, prev=(0.0, 0.0, 0.0)):
    """max over cost and gradient entries of |ref - dev| / (bound factor x S)"""
    r = mk_cases.problem(mk_np.RefProblem, kind, inp, u, f, prev); d = mk_cases.problem(mk_np.DevProblem, kind, inp, u, f, prev)
    Sc, Sg = r.magnitudes(x)
    b = bound_factor(r.T, inp["C"])
    fr, gr = r._cost(x), r._grad(x); fd, gd = d._eval(x, True)
    rc = abs(fr - fd) / (b * Sc)
    rg = max(np.abs(gr[0::2] - gd[0::2]) / (b * Sg)).item(), max(np.abs(gr[1::2] - gd[1::2]) / (b * Sg)).item()
    return max(rc, *rg)


@pytest.mark.parametrize("name", sorted(mk_cases.CASES))
def test_reference_order_and_device_order_agree(name):
    inp = mk_cases.case_inputs(name); rng = np.random.default_rng(9)
    worst = 0.0
    for kind in (mk_np.PR, mk_np.NRM):
        for u in (0, 2):
            for f in sorted({0, 1, inp["F"] - 1}):
                for scale, prev in ((0.1, (0.0, 0.0, 0.0)), (2.0, (0.8, 5.0, 40.0))):       # scale 2: beyond |gamma|, the clipping is active for _nrm
                    x = scale * rng.standard_normal(2 * (inp["C"] - 1))
                    worst = max(worst, ref_dev_ratio(inp, kind, u, f, x, prev))
    print(name, "largest |ref - dev| / bound: %.4f" % worst)
    assert worst <= 1.0, worst


def test_nrm_weights_lower_the_interferer():
    """broadside look direction (see tests/mk_cases.py), 1000 frames for 6 real unknowns a bin: the empirical kurtosis then stands for the
    expected one, which an added Gaussian lowers"""
    fftLen, C, T, look = 8, 4, 1000, 90.0
    X, tgt, itf = mk_cases.observations(1, C, T, fftLen, seed=31, parts=True, look=look)
    wq, B = mk_cases.fixed_weights(fftLen, C, look=look)
    inp = dict(fftLen=fftLen, C=C, T=T, sFrame=0, eFrame=T, R=1, X=X, wq=wq, B=B, nframes=np.array([T]), F=fftLen // 2 + 1)
    p_ds = p_mk = 0.0
    for f in range(1, inp["F"]):                                    # at bin 0 every direction has the same steering vector
        prob = mk_cases.problem(mk_np.DevProblem, mk_np.NRM, inp, 0, f)
        res = mk_np.minimize(prob, np.zeros(2 * (C - 1)), **mk_np.DEFAULTS[mk_np.NRM])
        assert np.isfinite(res["x"]).all() and res["iters"] >= 1
        wa = res["x"][0::2] + 1j * res["x"][1::2]
        wo = wq[f] - B[f] @ wa
        v = itf[0, :, :, f]                                          # [C][T]
        p_ds += (np.abs(np.conj(wq[f]) @ v) ** 2).sum(); p_mk += (np.abs(np.conj(wo) @ v) ** 2).sum()
        assert abs(np.vdot(wo, mk_cases.steering(fftLen, C, look)[f]) - 1.0) < 1e-12       # the target keeps gain 1
    print("interferer power at the output: delay and sum %.4f, maximum kurtosis %.4f" % (p_ds, p_mk))
    assert p_mk < p_ds


@pytest.mark.parametrize("name", sorted(mk_cases.BRANCH_CASES))
@pytest.mark.parametrize("cls", [mk_np.RefProblem, mk_np.DevProblem])
def test_named_case_takes_its_branch(name, cls):
    inp, kind, u, f, x0, settings, branch, reason = mk_cases.branch_inputs(name)
    prob = mk_cases.problem(cls, kind, inp, u, f)
    kw = dict(mk_np.DEFAULTS[kind]); kw.update(settings)
    res = mk_np.minimize(prob, x0, **kw)
    print(name, cls.__name__, {k: res[k] for k in ("iters", "evals", "failed", "reason", "f")}, sorted(res["branches"]))
    if branch is not None:
        assert branch in res["branches"]
        if branch in ("failed_trial", "intermediate_retry"):
            assert res["failed"] >= 1
    if reason is not None:
        assert res["reason"] == reason
    if reason == mk_np.SKIPPED:
        assert np.array_equal(res["x"], x0, equal_nan=True) and res["iters"] == 0
    else:
        assert res["reason"] != mk_np.EVAL_CAP_HIT and np.isfinite(res["x"]).all()


def test_ref_and_dev_minimisers_walk_the_same_path():
    """the same minimiser on the two orders of summation: same iteration and evaluation counts and exit, weights equal far beyond the stop tolerances"""
    inp = mk_cases.case_inputs("c4_t63")
    for kind in (mk_np.PR, mk_np.NRM):
        r = mk_np.minimize(mk_cases.problem(mk_np.RefProblem, kind, inp, 0, 2), np.zeros(6), **mk_np.DEFAULTS[kind])
        d = mk_np.minimize(mk_cases.problem(mk_np.DevProblem, kind, inp, 0, 2), np.zeros(6), **mk_np.DEFAULTS[kind])
        assert (r["iters"], r["evals"], r["failed"], r["reason"]) == (d["iters"], d["evals"], d["failed"], d["reason"])
        assert np.abs(r["x"] - d["x"]).max() < 1e-9 and abs(r["f"] - d["f"]) < 1e-12 * max(1.0, abs(r["f"]))


def test_carried_statistics_ref_and_dev():
    """_nrm over two blocks: storeStatistics advances prevFrameN before it divides the new terms, the old averages are not rescaled"""
    inp = mk_cases.case_inputs("c4_t63"); X2 = mk_cases.observations(mk_cases.U, inp["C"], inp["T"], inp["fftLen"], seed=4242)
    out = []
    for cls in (mk_np.RefProblem, mk_np.DevProblem):
        p1 = mk_cases.problem(cls, mk_np.NRM, inp, 0, 2)
        r1 = mk_np.minimize(p1, np.zeros(6), **mk_np.DEFAULTS[mk_np.NRM])
        assert p1.prev[2] == inp["T"] and p1.prev[0] > 0
        p2 = mk_cases.problem(cls, mk_np.NRM, inp, 0, 2, prev=tuple(p1.prev), X=X2)
        r2 = mk_np.minimize(p2, r1["x"], **mk_np.DEFAULTS[mk_np.NRM])
        assert p2.prev[2] == 2 * inp["T"]
        out.append((p1.prev, p2.prev, r2["x"]))
    for a, b in zip(out[0][:2], out[1][:2]):
        assert np.allclose(a, b, rtol=1e-9, atol=0)
    assert np.abs(out[0][2] - out[1][2]).max() < 1e-8


def test_host_side_of_the_c_abi(dsr):
    """what dsr_mk_* does without a device: the refusals, the fixed weights (B = NULL gives the shared _calcBlockingMatrix, equal to the numpy
    restatement bit for bit), the dispatch query; computing needs a HIP device -- there is no CPU path"""
    import torch
    for kw, status in ((dict(halfBandShift=True), 1), (dict(NC=2), 1), (dict(nSource=2), 13)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.MkBeamformer(8, 4, **kw)
        assert e.value.status == status, kw
    wq, B = mk_cases.fixed_weights(8, 8)
    mk = dsr.MkBeamformer(8, 8, dsr.MK_NRM); mk.setFixedWeights(wq, None)
    w2, B2 = mk.getFixedWeights()
    assert np.array_equal(w2, wq) and np.array_equal(B2, B)
    bf = dsr.Beamformer(8, 8); bf.calcGSCWeights(mk_cases.FS, mk_cases.delays(8, mk_cases.LOOK_DEG)); mk.setFixedWeightsFromBeamformer(bf)
    w3, B3 = mk.getFixedWeights()
    assert np.array_equal(w3, bf.get(0)[:5]) and np.array_equal(B3, bf.get(3)[:5]) and np.abs(w3 - wq).max() < 1e-15
    assert dsr.mk_path(8, 1024) == ((8, dsr.MK_FRAMES_LDS), (1024, 7 * 14 * 8 + 1024 * 8 * 16))
    assert dsr.mk_path(8, 1025)[0] == (8, dsr.MK_FRAMES_STREAMED) and dsr.mk_path(6, 10)[0][0] == 6 and dsr.mk_path(4, 10)[0][0] == 4
    assert dsr.mk_path(64, 128)[0] == (0, dsr.MK_FRAMES_LDS) and dsr.mk_path(64, 129)[0] == (0, dsr.MK_FRAMES_STREAMED) and dsr.mk_path(2, 5)[0][0] == 0
    with pytest.raises(dsr.DsrError) as e:
        dsr.mk_path(65, 10)
    assert e.value.status == 5
    if not torch.cuda.is_available():
        L = dsr.load(); z = np.zeros(8 * 8 * 5 * 2, np.float32); wa = np.zeros(5 * 7 * 2); info = np.zeros(5 * 4, np.int32); cost = np.zeros(5)
        p = lambda a: a.ctypes.data_as(dsr.vp)
        assert L.dsr_mk_estimate(mk.h, p(z), None, 1, 1, 0, 1, 1, -1, p(wa), None, p(info), p(cost), None) == 7      # JINITIALIZATION
