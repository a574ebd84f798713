"""Maximum negentropy beamforming and GG model training on the device (csrc/mn_kernels.hip through dsr._mn and dsr.btk.mnBeamforming / GGDcEst)
against the numpy restatements of tests/mn_np.py: bit for bit against the device-order restatement (cost, gradient, weights, iteration / evaluation /
failed-trial counts, exit reasons, final cost, training statistics), within the derived bound of the reference-order one.

The cases are those of the maximum-kurtosis tests (tests/mk_cases.py).  At 64 channels numpy follows the few problems tests/test_gpu_mk.py follows;
the device runs them all.  The model's constants come from the library (getConstants, ggd_constants): its lgamma is the C library's."""
import functools

import numpy as np
import pytest
import torch

import dsr._mn as M                                        # the product: without it nothing here can pass
from tests import mk_cases, mk_np, mn_np
from tests.test_gpu_mk import _Bank, packed

pytestmark = pytest.mark.gpu

MIN_KEYS = ("MAXITNS", "TOLERANCE", "STOPTOLERANCE", "DIFFSTOPTOLERANCE", "STEPSIZE")


@pytest.fixture(scope="module")
def mn(dsr):
    return M


@functools.lru_cache(maxsize=None)
def inputs(name):
    return mk_cases.case_inputs(name)


def shapes_of(F):
    """per-bin shape parameters spread over [0.1, 1.5], with exactly 1.0 (2f - 2 = 0) and one value above 1"""
    s = np.linspace(0.1, 1.5, F); s[F // 2] = 1.0
    return s


def settings_of(over=()):
    kw = dict(mn_np.DEFAULTS); kw.update(dict(over))
    return kw


def make(mn, inp, over=()):
    kw = settings_of(over)
    b = mn.MnBeamformer(inp["fftLen"], inp["C"], shapes_of(inp["F"]), kw["alpha"], kw["beta"], kw["gamma"])
    b.setFixedWeights(inp["wq"], inp["B"]); b.minimizer(**{k: kw[k] for k in MIN_KEYS})
    return b


@functools.lru_cache(maxsize=None)
def constants_of(F):
    b = M.MnBeamformer(2 * (F - 1), 2, shapes_of(F))
    return b.getConstants()


def problem(cls, inp, u, f, X=None, beta=0.5):
    X = inp["X"] if X is None else X
    Bc, Ng, lB = constants_of(inp["F"]); sh = shapes_of(inp["F"])[f]
    sel = mk_np.select_frames(inp["sFrame"], inp["eFrame"], inp["R"], int(inp["nframes"][u]), X.shape[2])
    Xf = np.ascontiguousarray(X[u][:, sel, :][:, :, f].T) if sel else np.zeros((0, inp["C"]), X.dtype)
    a = (Xf, inp["wq"][f], inp["B"][f], 1.0e-2, beta, sh, Bc[f], Ng[f])
    return cls(*a, lB[f]) if cls is mn_np.DevProblem else cls(*a)


def problems_of(inp):
    """the problems numpy minimises too (about 900 evaluations each where no stop test is met): all of them at 5 bins; at 17 bins four bins, the
    one with shape 1.0 among them; at 64 channels those of tests/test_gpu_mk.py.  The eval test compares every problem."""
    F = inp["F"]
    if inp["C"] == 64:
        return [(0, 1), (1, 0), (1, 2)]
    return [(u, f) for u in range(mk_cases.U) for f in (range(F) if F <= 5 else (0, 5, F // 2, F - 1))]


@functools.lru_cache(maxsize=None)
def dev_estimate(name, over=()):
    """{(u, f): result of the device-order restatement from a zero start}"""
    inp = inputs(name); kw = settings_of(over); out = {}
    for (u, f) in problems_of(inp):
        out[(u, f)] = mn_np.minimize(problem(mn_np.DevProblem, inp, u, f, beta=kw["beta"]), np.zeros(2 * (inp["C"] - 1)), **kw)
    return out


def dev_args(inp, cuda, X=None):
    X = inp["X"] if X is None else X
    return torch.from_numpy(X).to(cuda), dict(nframes=torch.from_numpy(inp["nframes"]).to(cuda), sFrame=inp["sFrame"], eFrame=inp["eFrame"], R=inp["R"])


def run_estimate(b, X, kw, **more):
    wa, info, cost = b.estimate(X, **kw, **more)
    return packed(wa), info.cpu().numpy(), cost.cpu().numpy()


def assert_matches(got, want, where):
    wa, info, cost = got
    for (u, f), r in want.items():
        assert np.array_equal(wa[u, f], r["x"], equal_nan=True), (where, u, f, wa[u, f], r["x"])
        assert tuple(info[u, f]) == (r["iters"], r["evals"], r["failed"], r["reason"]), (where, u, f, info[u, f], r)
        assert np.array_equal(cost[u, f], r["f"], equal_nan=True), (where, u, f, cost[u, f], r["f"])


@pytest.mark.parametrize("name", sorted(mk_cases.CASES))
def test_eval_equals_device_order_and_bounds_reference_order(mn, cuda, name):
    inp = inputs(name); X, kw = dev_args(inp, cuda); n = inp["C"] - 1; F = inp["F"]; rng = np.random.default_rng(3)
    b = make(mn, inp)
    for scale in (0.1, 2.0):
        wa = scale * (rng.standard_normal((mk_cases.U, F, n)) + 1j * rng.standard_normal((mk_cases.U, F, n)))
        cost, grad = b.eval(X, wa, **kw)
        cost, grad = cost.cpu().numpy(), grad.cpu().numpy(); xs = packed(torch.from_numpy(wa))
        worst = 0.0
        for u in range(mk_cases.U):
            for f in range(F):
                d = problem(mn_np.DevProblem, inp, u, f)
                fd, gd = d._eval(xs[u, f], True)
                assert np.array_equal(cost[u, f], fd, equal_nan=True) and np.array_equal(grad[u, f], gd, equal_nan=True), (u, f, cost[u, f], fd, grad[u, f], gd)
                if d.T == 0 or inp["C"] == 64 and f not in (0, 1):
                    continue
                r = problem(mn_np.RefProblem, inp, u, f)
                bc, bg = r.bound(xs[u, f], inp["C"]); gr = r._grad(xs[u, f])
                worst = max(worst, abs(r._cost(xs[u, f]) - cost[u, f]) / bc, np.max(np.abs(gr[0::2] - grad[u, f][0::2]) / bg),
                            np.max(np.abs(gr[1::2] - grad[u, f][1::2]) / bg))
        print(name, scale, "largest |ref - device| / bound: %.4f" % worst)
        assert worst <= 1.0


@pytest.mark.parametrize("name", sorted(mk_cases.CASES))
def test_estimate_equals_device_order_at_the_defaults(mn, dsr, cuda, name):
    inp = inputs(name); X, kw = dev_args(inp, cuda)
    b = make(mn, inp)
    start, _ = b.eval(X, np.zeros((mk_cases.U, inp["F"], inp["C"] - 1), np.complex128), **kw)
    got = run_estimate(b, X, kw)
    assert_matches(got, dev_estimate(name), name)
    again = run_estimate(b, X, kw)                                    # a second call repeats bit for bit
    for a, c in zip(got, again):
        assert np.array_equal(a, c, equal_nan=True)
    assert dsr.mk_path(inp["C"], inp["T"])[0][1] == dsr.MK_FRAMES_LDS
    b.forceStreamed(True)                                             # the forced streamed path equals the LDS path bit for bit
    streamed = run_estimate(b, X, kw)
    for a, c in zip(got, streamed):
        assert np.array_equal(a, c, equal_nan=True)
    reasons = got[1][..., 3]
    assert (reasons[1] == dsr.MK_EXIT_SKIPPED).all() and (reasons[0] != dsr.MK_EXIT_SKIPPED).all() and (reasons != dsr.MK_EXIT_EVAL_CAP).all()
    ran = reasons != dsr.MK_EXIT_SKIPPED
    assert (got[2][ran] <= start.cpu().numpy()[ran]).all()            # the final cost is no larger than the starting cost


@pytest.mark.parametrize("name", mk_cases.STEP5_CASES)
def test_estimate_equals_device_order_at_stepsize_5(mn, cuda, name):
    inp = inputs(name); X, kw = dev_args(inp, cuda); over = (("STEPSIZE", 5.0),)
    got = run_estimate(make(mn, inp, over), X, kw)
    assert_matches(got, dev_estimate(name, over), (name, "STEPSIZE 5"))


def test_stepsize_5_retries_and_a_forced_conjugate_restart(mn, cuda):
    tot = sum(r["failed"] for name in mk_cases.STEP5_CASES for r in dev_estimate(name, (("STEPSIZE", 5.0),)).values())
    assert tot >= 1                                                   # intermediate_point retried, on the device as in the restatement (above)
    name = "c2_t200_r2"; over = (("DIFFSTOPTOLERANCE", 0.0), ("MAXITNS", 4), ("STOPTOLERANCE", 0.0))
    inp = inputs(name); X, kw = dev_args(inp, cuda)
    want = dev_estimate(name, over)
    assert any("restart" in r["branches"] for r in want.values())
    assert_matches(run_estimate(make(mn, inp, over), X, kw), want, "restart")


def test_zero_frames_are_counted_out_and_zero_observations_skipped(mn, dsr, cuda):
    inp = inputs("c4_t63"); Xz = inp["X"].copy(); Xz[0, :, 3, :] = 0; Xz[0, :, 40, :] = 0
    X, kw = dev_args(inp, cuda, Xz); n = inp["C"] - 1; F = inp["F"]
    b = make(mn, inp)
    wa = 0.1 * (np.random.default_rng(4).standard_normal((mk_cases.U, F, n)) + 0j)
    cost, grad = b.eval(X, wa, **kw); xs = packed(torch.from_numpy(wa))
    for f in range(F):
        d = problem(mn_np.DevProblem, inp, 0, f, X=Xz)
        fd, gd = d._eval(xs[0, f], True)
        assert np.array_equal(cost[0, f].item(), fd) and np.array_equal(grad[0, f].cpu().numpy(), gd)
        # T' = T - 2: the restatement over the frames left has the same sums; its data term is smaller by 61 / 63 (the means run over T)
        keep = [t for t in range(63) if t not in (3, 40)]
        less = mn_np.DevProblem(np.ascontiguousarray(Xz[0][:, keep, f].T), inp["wq"][f], inp["B"][f], 1.0e-2, 0.5, d.shape, d.Bc, d.NgConst, d.logBc)
        assert np.allclose(gd - 1.0e-2 * xs[0, f], (less._eval(xs[0, f], True)[1] - 1.0e-2 * xs[0, f]) * (63.0 / 61.0), rtol=1e-11, atol=1e-14)
    Xall = torch.zeros_like(X)
    start = 0.3 * (np.random.default_rng(5).standard_normal((mk_cases.U, F, n)) + 0j)
    w, info, c = run_estimate(b, Xall, kw, wa=start)
    assert (info[..., 3] == dsr.MK_EXIT_SKIPPED).all() and np.array_equal(w, packed(torch.from_numpy(start)))


def test_single_bin_and_index_refusal(mn, dsr, cuda):
    inp = inputs("c6_t200"); X, kw = dev_args(inp, cuda); b = make(mn, inp); k = 3
    allb = run_estimate(b, X, kw)
    one = run_estimate(b, X, kw, fbinX=k)
    for a, c in zip(allb, one):
        assert np.array_equal(a[:, k], c[:, k], equal_nan=True)
    assert (one[1][:, (k + 1) % inp["F"]] == 0).all()                 # a bin that was not asked for is left alone
    with pytest.raises(dsr.DsrError) as e:
        b.estimate(X, fbinX=inp["F"], **kw)
    assert e.value.status == 6


def test_apply_equals_the_kurtosis_beamformers_apply(mn, dsr, cuda):
    inp = inputs("c8_t65"); X, _ = dev_args(inp, cuda)
    b = make(mn, inp); mk = dsr.MkBeamformer(inp["fftLen"], inp["C"]); mk.setFixedWeights(inp["wq"], inp["B"])
    wa = 0.2 * (np.random.default_rng(8).standard_normal((mk_cases.U, inp["F"], 7)) + 1j * np.random.default_rng(9).standard_normal((mk_cases.U, inp["F"], 7)))
    Y = b.apply(X, wa)
    assert torch.equal(Y, mk.apply(X, wa)) and Y.abs().max().item() > 0.1


def test_python_classes_return_what_the_batch_face_returns(mn, cuda):
    from dsr.btk import mnBeamforming as MN
    from dsr.btk import GGDcEst as G
    inp = inputs("c4_t200_r2"); C, F, fftLen = inp["C"], inp["F"], inp["fftLen"]
    Xu = inp["X"][0]; kwsel = dict(sFrame=inp["sFrame"], eFrame=inp["eFrame"], R=inp["R"])
    Xd = torch.from_numpy(inp["X"][:1]).to(cuda)
    ggdL = [G.CGGaussianD(p=float(s), sa=1.0) for s in shapes_of(F)]
    for cls, beta in ((MN.MNSubbandBeamformerGGDc_pr, 0.5), (MN.MNSubbandBeamformerGGDc_nrm, 1.0)):
        obj = cls([_Bank(Xu[c], fftLen) for c in range(C)], ggdL)
        obj.setFixedWeights([inp["wq"]], updateBlockingMatrix=True)
        obs = obj.accumObservations(inp["sFrame"], inp["eFrame"], inp["R"])
        sel = mk_np.select_frames(inp["sFrame"], inp["eFrame"], inp["R"], inp["T"], inp["T"])
        assert obj.getSampleN() == len(sel) and np.array_equal(obs, Xu[:, sel, :].transpose(1, 2, 0))
        b = mn.MnBeamformer(fftLen, C, shapes_of(F), beta=beta); b.setFixedWeights(inp["wq"], None)
        wa, info, cost = b.estimate(Xd, **kwsel)
        allw = obj.estimateAllActiveWeights()
        assert np.array_equal(allw, packed(wa)[0]) and np.array_equal(obj.lastInfo()[0], info[0].cpu().numpy())
        one = obj.estimateActiveWeights(3, np.zeros(2 * (C - 1)))
        assert np.array_equal(one, allw[3])
        x = 0.1 * np.random.default_rng(2).standard_normal(2 * (C - 1)); w = obj.UnpackWeights(x)
        full = np.zeros((1, F, C - 1), np.complex128); full[0, 3] = w[0]
        c, g = b.eval(Xd, full, fbinX=3, **kwsel)
        assert MN.fun_MN(x, (3, obj, 1)) == c[0, 3].item() and np.array_equal(MN.dfun_MN(x, (3, obj, 1)), g[0, 3].cpu().numpy())
        obj.calcEntireWeights_f(3, w); obj.calcCovarOutputs_f(3)
        assert obj.negentropy(0, 3) == float(1.0e-2 * np.sum(np.abs(w[0]) ** 2) - c[0, 3].item())
        gg = g[0, 3].cpu().numpy()
        assert np.array_equal(obj.gradient(0, 3), -((gg[0::2] + 1j * gg[1::2]) - 1.0e-2 * w[0]))
        Y = obj.apply(allw)                                           # the frames accumObservations read: 0 .. eFrame - 1
        assert Y.shape[0] == inp["eFrame"] and torch.equal(Y, b.apply(Xd, wa)[0][:inp["eFrame"]])
        obj.openLogFile("unused"); obj.writeLogFile("x"); obj.closeLogFile()
        obj.nextSpkr()
        assert obj.getSampleN() == 0
    with pytest.raises(mn.DsrError):
        MN.MNSubbandBeamformerGGDc_pr(Xd[0], ggdL, nSource=2)
    with pytest.raises(mn.DsrError):
        MN.MNSubbandBeamformerGGDc_nrm(Xd[0], ggdL, NC=2)
    with pytest.raises(mn.DsrError):
        MN.MNSubbandBeamformerGGDc_pr(Xd[0], ggdL, halfBandShift=True)


# ---- GG model training
def lib_constants(mn):
    def constants(p):
        Bc, lNF, Ng, Ll = (float(v[0]) for v in mn.ggd_constants(np.array([p])))
        return dict(Bc=Bc, lNF=lNF, NgConst=Ng, LlConst=Ll, logBc=mn_np.det_log(Bc))
    return constants


def ggd_inputs(T, F, seed):
    rng = np.random.default_rng(seed); U = 3
    X = ((rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))) * np.abs(rng.standard_normal((U, T, F)))).astype(np.complex64)
    X[0, 0, 0] = 0; X[0, T // 2, F - 1] = 0; X[2, 0, 1] = 3e-12 + 2e-12j            # exact zeros, one value below 1e-11
    nframes = np.array([T, 0, (T + 1) // 2], np.int32)
    p = np.linspace(0.2, 1.4, F); sa = np.linspace(0.5, 2.5, F)
    return X, nframes, p, sa


@pytest.mark.parametrize("T,F", [(1, 5), (63, 5), (64, 65), (65, 65), (300, 17)])
def test_ggd_accumulate_equals_device_order_and_bounds_reference_order(mn, cuda, T, F):
    X, nframes, p, sa = ggd_inputs(T, F, 100 + T + F); cst = lib_constants(mn)
    Xd = torch.from_numpy(X).to(cuda); nf = torch.from_numpy(nframes).to(cuda)
    acc = mn.ggd_accumulate(Xd, p, sa, nf)
    want = mn_np.ggd_acc_dev(X, nframes, p, sa, constants=cst)
    assert np.array_equal(acc, want), np.abs(acc - want).max()
    assert np.array_equal(acc, mn.ggd_accumulate(Xd, p, sa, nf))      # a call repeats bit for bit
    assert (acc[3] == nframes.sum()).all()
    ref = mn_np.ggd_acc_ref(X, nframes, p, sa); bound = mn_np.acc_bound(X, nframes, p, sa)
    ratio = np.abs(acc - ref)[[0, 1, 2, 4]] / bound[[0, 1, 2, 4]]
    print("T %d F %d: largest |ref - device| / bound %.4f" % (T, F, ratio.max()))
    assert (ratio <= 1.0).all()
    # chaining over two half-batches: acc_in is added first, so the order is that of the same chaining, not that of one call
    a1 = mn.ggd_accumulate(Xd[:2], p, sa, nf[:2]); a2 = mn.ggd_accumulate(Xd[2:], p, sa, nf[2:], acc_in=a1)
    w1 = mn_np.ggd_acc_dev(X[:2], nframes[:2], p, sa, constants=cst); w2 = mn_np.ggd_acc_dev(X[2:], nframes[2:], p, sa, acc_in=w1, constants=cst)
    assert np.array_equal(a1, w1) and np.array_equal(a2, w2)


def test_training_on_device_data_equals_the_restatement(mn, cuda):
    from dsr.btk import GGDcEst as G
    X, nframes, p, sa = ggd_inputs(300, 17, 9); cst = lib_constants(mn); n = int(nframes.sum())
    Xd = torch.from_numpy(X).to(cuda); nf = torch.from_numpy(nframes).to(cuda)
    ggdL, pt, st, conv = G.trainGGD(Xd, nf, p=p, sa=sa, alpha=1.0 / n, maxUpdates=3)
    pw, sw = p.copy(), sa.copy()
    for it in range(3):
        sw, pw, cv = mn_np.ggd_update(mn_np.ggd_acc_dev(X, nframes, pw, sw, constants=cst), pw, sw, nItr=it, alpha=1.0 / n, constants=cst)
        assert not cv.any()
    assert np.array_equal(pt, pw) and np.array_equal(st, sw) and ggdL[4].getShapePar() == pw[4] and ggdL[4].fixed()
    # MLE4CGGaussianD on the samples of one bin, three updates
    m = G.MLE4CGGaussianD(p=0.7, sigma=1.0, alpha=1.0 / n); m.fixConst()
    x1 = np.ascontiguousarray(X[0, :, 3]); pw, sw = np.array([0.7]), np.array([1.0])
    for it in range(3):
        m.acc(torch.from_numpy(x1).to(cuda)); got = m.update()
        sw, pw, cv = mn_np.ggd_update(mn_np.ggd_acc_dev(x1[None, :, None], [len(x1)], pw, sw, constants=cst), pw, sw, nItr=it, alpha=1.0 / n, constants=cst)
        assert got == [sw[0], pw[0], bool(cv[0])]


def test_interferer_power_before_and_after(mn, cuda):
    """printed, not asserted: a broadside look direction, where the blocking matrix blocks the target exactly"""
    fftLen, C, T = 8, 4, 200; F = fftLen // 2 + 1
    X, tgt, itf = mk_cases.observations(1, C, T, fftLen, seed=77, parts=True, look=90.0)
    wq, B = mk_cases.fixed_weights(fftLen, C, look=90.0)
    b = mn.MnBeamformer(fftLen, C, np.full(F, 0.4)); b.setFixedWeights(wq, B)
    wa, info, cost = b.estimate(torch.from_numpy(X).to(cuda))
    w = wa.cpu().numpy()[0]
    for f in range(1, F):
        weff = wq[f] - B[f] @ w[f]
        before = np.mean(np.abs(np.conj(wq[f]) @ itf[0, :, :, f]) ** 2); after = np.mean(np.abs(np.conj(weff) @ itf[0, :, :, f]) ** 2)
        print("bin %d: interferer image power %.4f -> %.4f, exit %d after %d evaluations" % (f, before, after, info[0, f, 3].item(), info[0, f, 1].item()))
