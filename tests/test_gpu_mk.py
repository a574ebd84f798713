"""Maximum empirical kurtosis beamforming on the device (csrc/k_mk.hip through dsr._capi.MkBeamformer and dsr.btk.mkBeamforming) against the
numpy restatements of tests/mk_np.py: bit for bit against the device-order restatement (cost, gradient, weights, iteration / evaluation /
failed-trial counts, exit reasons, final cost, carried statistics), within the derived rounding bound of the reference-order one.

Every problem of a case is compared, except at 64 channels: there the conjugate-gradient minimiser (about 900 evaluations a problem at the defaults:
40 iterations that never meet a stop test, the cost being unbounded below without the norm constraint) has its numpy counterpart run on one bin
of the first utterance and two of the empty one, the steepest-descent minimiser on two bins more; the device runs all of them."""
import functools

import numpy as np
import pytest
import torch

from tests import mk_cases, mk_np

pytestmark = pytest.mark.gpu

MIN_KEYS = ("MAXITNS", "TOLERANCE", "STOPTOLERANCE", "DIFFSTOPTOLERANCE", "STEPSIZE")


@functools.lru_cache(maxsize=None)
def inputs(name):
    return mk_cases.case_inputs(name)


def settings_of(kind, over=()):
    kw = dict(mk_np.DEFAULTS[kind]); kw.update(dict(over))
    return kw


def problems_of(inp, kind):
    F, full = inp["F"], [(u, f) for u in range(mk_cases.U) for f in range(inp["F"])]
    if inp["C"] == 64:
        return [(0, 1), (1, 0), (1, 2)] + ([(0, 0), (2, F - 1)] if kind == mk_np.NRM else [])
    return full


@functools.lru_cache(maxsize=None)
def dev_estimate(name, kind, over=()):
    """{(u, f): result of the device-order restatement from a zero start}"""
    inp = inputs(name); kw = settings_of(kind, over); out = {}
    for (u, f) in problems_of(inp, kind):
        prob = mk_cases.problem(mk_np.DevProblem, kind, inp, u, f, **{k: kw[k] for k in ("alpha", "beta", "gamma")})
        res = mk_np.minimize(prob, np.zeros(2 * (inp["C"] - 1)), **kw); res["prev"] = list(prob.prev)
        out[(u, f)] = res
    return out


def make(dsr, inp, kind, over=()):
    kw = settings_of(kind, over)
    mk = dsr.MkBeamformer(inp["fftLen"], inp["C"], kind, kw["alpha"], kw["beta"], kw["gamma"])
    mk.setFixedWeights(inp["wq"], inp["B"]); mk.minimizer(**{k: kw[k] for k in MIN_KEYS})
    return mk


def dev_args(inp, cuda, X=None):
    X = inp["X"] if X is None else X
    return torch.from_numpy(X).to(cuda), dict(nframes=torch.from_numpy(inp["nframes"]).to(cuda), sFrame=inp["sFrame"], eFrame=inp["eFrame"], R=inp["R"])


def packed(wa):
    w = wa.cpu().numpy(); out = np.zeros(w.shape[:-1] + (2 * w.shape[-1],)); out[..., 0::2] = w.real; out[..., 1::2] = w.imag
    return out


def assert_matches(got, want, where):
    wa, info, cost = got
    for (u, f), r in want.items():
        assert np.array_equal(wa[u, f], r["x"], equal_nan=True), (where, u, f, wa[u, f], r["x"])
        assert tuple(info[u, f]) == (r["iters"], r["evals"], r["failed"], r["reason"]), (where, u, f, info[u, f], r)
        assert np.array_equal(cost[u, f], r["f"], equal_nan=True), (where, u, f, cost[u, f], r["f"])


def run_estimate(mk, X, kw, **more):
    wa, info, cost = mk.estimate(X, **kw, **more)
    return packed(wa), info.cpu().numpy(), cost.cpu().numpy()


@pytest.mark.parametrize("name", sorted(mk_cases.CASES))
def test_eval_equals_device_order_and_bounds_reference_order(dsr, cuda, name):
    inp = inputs(name); X, kw = dev_args(inp, cuda); n = inp["C"] - 1; F = inp["F"]; rng = np.random.default_rng(3)
    for kind in (mk_np.PR, mk_np.NRM):
        mk = make(dsr, inp, kind)
        for scale, carried in ((0.1, False), (2.0, True)):           # scale 2: beyond |gamma|, so _nrm clips
            wa = scale * (rng.standard_normal((mk_cases.U, F, n)) + 1j * rng.standard_normal((mk_cases.U, F, n)))
            prevs = np.zeros((3, mk_cases.U, F))
            if carried:
                prevs[0] = 0.8; prevs[1] = 5.0; prevs[2] = 40.0
            cost, grad = mk.eval(X, wa, stats=torch.from_numpy(prevs).to(cuda) if carried else None, **kw)
            cost, grad = cost.cpu().numpy(), grad.cpu().numpy(); xs = packed(torch.from_numpy(wa))
            worst = 0.0
            for u in range(mk_cases.U):
                for f in range(F):
                    prev = tuple(prevs[:, u, f])
                    d = mk_cases.problem(mk_np.DevProblem, kind, inp, u, f, prev)
                    fd, gd = d._eval(xs[u, f], True)
                    assert np.array_equal(cost[u, f], fd, equal_nan=True) and np.array_equal(grad[u, f], gd, equal_nan=True), (kind, u, f, cost[u, f], fd)
                    if d.T == 0 or inp["C"] == 64 and f not in (0, 1):
                        continue
                    r = mk_cases.problem(mk_np.RefProblem, kind, inp, u, f, prev)
                    Sc, Sg = r.magnitudes(xs[u, f]); b = mk_np.bound_factor(r.T, inp["C"])
                    gr = r._grad(xs[u, f])
                    worst = max(worst, abs(r._cost(xs[u, f]) - cost[u, f]) / (b * Sc), np.max(np.abs(gr[0::2] - grad[u, f][0::2]) / (b * Sg)),
                                np.max(np.abs(gr[1::2] - grad[u, f][1::2]) / (b * Sg)))
            print(name, kind, scale, "largest |ref - device| / bound: %.4f" % worst)
            assert worst <= 1.0


@pytest.mark.parametrize("kind", [mk_np.PR, mk_np.NRM])
@pytest.mark.parametrize("name", sorted(mk_cases.CASES))
def test_estimate_equals_device_order_at_the_defaults(dsr, cuda, name, kind):
    inp = inputs(name); X, kw = dev_args(inp, cuda)
    mk = make(dsr, inp, kind)
    got = run_estimate(mk, X, kw)
    assert_matches(got, dev_estimate(name, kind), (name, kind))
    again = run_estimate(mk, X, kw)                                   # a second call repeats bit for bit
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True)
    # the forced streamed path equals the LDS path bit for bit
    assert dsr.mk_path(inp["C"], inp["T"])[0][1] == dsr.MK_FRAMES_LDS
    mk.forceStreamed(True)
    streamed = run_estimate(mk, X, kw)
    for a, b in zip(got, streamed):
        assert np.array_equal(a, b, equal_nan=True)
    reasons = got[1][..., 3]
    assert (reasons[1] == dsr.MK_EXIT_SKIPPED).all() and (reasons[0] != dsr.MK_EXIT_SKIPPED).all() and (reasons != dsr.MK_EXIT_EVAL_CAP).all()


@pytest.mark.parametrize("kind", [mk_np.PR, mk_np.NRM])
@pytest.mark.parametrize("name", mk_cases.STEP5_CASES)
def test_estimate_equals_device_order_at_stepsize_5(dsr, cuda, name, kind):
    inp = inputs(name); X, kw = dev_args(inp, cuda); over = (("STEPSIZE", 5.0),)
    got = run_estimate(make(dsr, inp, kind, over), X, kw)
    assert_matches(got, dev_estimate(name, kind, over), (name, kind, "STEPSIZE 5"))


def test_stepsize_5_takes_failed_trials(dsr, cuda):
    """across the STEPSIZE 5.0 cases both minimisers reject trial points, on the device as in the restatement"""
    for kind in (mk_np.PR, mk_np.NRM):
        tot = 0
        for name in mk_cases.STEP5_CASES:
            tot += sum(r["failed"] for r in dev_estimate(name, kind, (("STEPSIZE", 5.0),)).values())
        assert tot >= 1, kind


@pytest.mark.parametrize("name", ["c4_t63", "c8_t65", "c3_t65"])
def test_carried_statistics_over_two_blocks(dsr, cuda, name):
    inp = inputs(name); kind = mk_np.NRM; F, n = inp["F"], inp["C"] - 1
    X1, kw = dev_args(inp, cuda)
    Xb = mk_cases.observations(mk_cases.U, inp["C"], inp["T"], inp["fftLen"], seed=4242); X2, _ = dev_args(inp, cuda, Xb)
    mk = make(dsr, inp, kind)
    stats = torch.zeros((3, mk_cases.U, F), dtype=torch.float64, device=cuda)
    wa1, info1, cost1 = mk.estimate(X1, stats=stats, **kw)
    first = dev_estimate(name, kind)
    s1 = stats.cpu().numpy().copy()
    for (u, f), r in first.items():
        assert np.array_equal(s1[:, u, f], r["prev"]), (u, f, s1[:, u, f], r["prev"])
    assert (s1[2, 1] == 0).all() and (s1[2, 0] == len(mk_np.select_frames(inp["sFrame"], inp["eFrame"], inp["R"], inp["T"], inp["T"]))).all()
    got = run_estimate(mk, X2, kw, wa=wa1, stats=stats)
    s2 = stats.cpu().numpy()
    want = {}
    kwm = settings_of(kind)
    for (u, f), r in first.items():
        prob = mk_cases.problem(mk_np.DevProblem, kind, inp, u, f, prev=tuple(r["prev"]), X=Xb)
        want[(u, f)] = mk_np.minimize(prob, r["x"], **kwm)
        assert np.array_equal(s2[:, u, f], prob.prev), (u, f, s2[:, u, f], prob.prev)
    assert_matches(got, want, (name, "second block"))


def test_unforced_streamed_path(dsr, cuda):
    """U = 2, fftLen 8, C = 8 and more frames than dsr_mk_path reports as LDS resident: the streamed path without the switch"""
    C, fftLen = 8, 8
    (ct, res), (tcap, _) = dsr.mk_path(C, 1)
    assert ct == 8 and res == dsr.MK_FRAMES_LDS and tcap == 1024
    T = tcap + 6
    assert dsr.mk_path(C, tcap)[0][1] == dsr.MK_FRAMES_LDS and dsr.mk_path(C, T)[0][1] == dsr.MK_FRAMES_STREAMED
    X = mk_cases.observations(2, C, T, fftLen, seed=99); wq, B = mk_cases.fixed_weights(fftLen, C)
    inp = dict(fftLen=fftLen, C=C, T=T, sFrame=0, eFrame=T, R=1, X=X, wq=wq, B=B, nframes=np.array([T, T - 1], np.int32), F=fftLen // 2 + 1)
    Xd, kw = dev_args(inp, cuda)
    for kind, probs in ((mk_np.NRM, [(u, f) for u in range(2) for f in range(inp["F"])]), (mk_np.PR, [(1, 2)])):
        got = run_estimate(make(dsr, inp, kind), Xd, kw)
        want = {}
        for (u, f) in probs:
            want[(u, f)] = mk_np.minimize(mk_cases.problem(mk_np.DevProblem, kind, inp, u, f), np.zeros(2 * (C - 1)), **settings_of(kind))
        assert_matches(got, want, ("streamed", kind))


@pytest.mark.parametrize("name", sorted(mk_cases.BRANCH_CASES))
def test_branch_cases_on_the_device(dsr, cuda, name):
    """the cases named for a branch, one bin at a time (fbinX): the device takes the path the restatement takes"""
    inp, kind, u, f, x0, settings, branch, reason = mk_cases.branch_inputs(name)
    over = tuple(sorted(settings.items())); kwm = settings_of(kind, over)
    X, kw = dev_args(inp, cuda)
    n = inp["C"] - 1
    start = np.zeros((mk_cases.U, inp["F"], n), np.complex128); start[:, :] = x0[0::2] + 1j * x0[1::2]
    got = run_estimate(make(dsr, inp, kind, over), X, kw, wa=start, fbinX=f)
    want = {}
    for uu in range(mk_cases.U):
        want[(uu, f)] = mk_np.minimize(mk_cases.problem(mk_np.DevProblem, kind, inp, uu, f), x0, **kwm)
    assert_matches(got, want, name)
    if reason is not None:
        assert got[1][u, f, 3] == reason
    other = (f + 1) % inp["F"]                                        # a bin that was not asked for is left alone
    assert (got[1][:, other] == 0).all() and np.array_equal(got[0][:, other], packed(torch.from_numpy(start))[:, other], equal_nan=True)


def test_apply_equals_the_gsc_with_the_same_weights(dsr, cuda):
    """U = 1: Beamformer.apply after setActiveWeights_f with the weights dsr_mk_apply is given.  SubbandGSC takes the quiescent vector alone at bin 0,
    so the active weights of bin 0 are zero here.  Both round wq - B wa to fp32 and add C complex products in fp32, one with fused multiply-adds
    and one without: each is within sqrt(2) (C + 2) 2^-24 S of the exact sum, S = sum_c |w_c| |x_c|, so they differ by less than 4 (C + 2) 2^-24 S."""
    fftLen, C, T = 32, 8, 37; F = fftLen // 2 + 1
    X = torch.from_numpy(mk_cases.observations(1, C, T, fftLen, seed=5)).to(cuda)
    d = mk_cases.delays(C, mk_cases.LOOK_DEG)
    bf = dsr.Beamformer(fftLen, C); bf.calcGSCWeights(mk_cases.FS, d); bf.select("gsc")
    mk = dsr.MkBeamformer(fftLen, C); mk.setFixedWeightsFromBeamformer(bf)
    wq, B = mk.getFixedWeights()
    assert np.array_equal(wq, bf.get(0)[:F]) and np.array_equal(B, bf.get(3)[:F])
    mk2 = dsr.MkBeamformer(fftLen, C); mk2.setFixedWeights(wq, None)                        # B = NULL: the shared _calcBlockingMatrix
    assert np.array_equal(mk2.getFixedWeights()[1], B)
    rng = np.random.default_rng(8)
    wa = 0.2 * (rng.standard_normal((1, F, C - 1)) + 1j * rng.standard_normal((1, F, C - 1))); wa[0, 0] = 0
    pk = packed(torch.from_numpy(wa))
    for f in range(1, F):
        bf.setActiveWeights_f(f, pk[0, f])
    Y1 = bf.apply(X).cpu().numpy(); Y2 = mk.apply(X, wa).cpu().numpy()
    w = bf.get(4)                                                     # [F][C]
    S = np.einsum("fc,ctf->tf", np.abs(w), np.abs(X[0].cpu().numpy()))
    assert Y1.shape == Y2.shape == (1, T, F)
    assert (np.abs(Y1[0] - Y2[0]) <= 4 * (C + 2) * 2.0 ** -24 * S).all()
    assert np.abs(Y2).max() > 0.1
    # per-utterance weights: utterance 1 of a batch of two gets its own
    X2 = torch.cat([X, X]); wa2 = np.concatenate([wa, np.zeros_like(wa)])
    Yb = mk.apply(X2, wa2).cpu().numpy()
    assert np.array_equal(Yb[0], Y2[0])
    bf.zeroActiveWeights()
    assert (np.abs(Yb[1] - bf.apply(X).cpu().numpy()[0]) <= 4 * (C + 2) * 2.0 ** -24 * S).all()


class _Bank(object):
    """a stand-in for an analysis filter bank: next() hands out fftLen subband samples a frame"""

    def __init__(self, frames, fftLen):
        self._x = frames; self._M = fftLen; self._t = 0                # frames [T][F]

    def fftLen(self):
        return self._M

    def reset(self):
        self._t = 0

    def next(self):
        if self._t >= len(self._x):
            raise StopIteration
        h = self._x[self._t]; self._t += 1
        return np.concatenate([h, np.conj(h[-2:0:-1])])


def test_python_classes_return_what_the_batch_face_returns(dsr, cuda):
    from dsr.btk import mkBeamforming as M
    inp = inputs("c4_t200_r2"); C, F, fftLen = inp["C"], inp["F"], inp["fftLen"]
    Xu = inp["X"][0]                                                  # [C][T][F]
    kwsel = dict(sFrame=inp["sFrame"], eFrame=inp["eFrame"], R=inp["R"])
    Xd = torch.from_numpy(inp["X"][:1]).to(cuda)
    for cls, kind in ((M.MEKSubbandBeamformer_pr, mk_np.PR), (M.MEKSubbandBeamformer_nrm, mk_np.NRM)):
        obj = cls([_Bank(Xu[c], fftLen) for c in range(C)])
        obj.setFixedWeights([inp["wq"]], updateBlockingMatrix=True)
        obs = obj.accumObservations(inp["sFrame"], inp["eFrame"], inp["R"])
        sel = mk_np.select_frames(inp["sFrame"], inp["eFrame"], inp["R"], inp["T"], inp["T"])
        assert obj.getSampleN() == len(sel) and obj.getChanN() == C and obj.getFftLen() == fftLen and np.array_equal(obs, Xu[:, sel, :].transpose(1, 2, 0))
        assert np.allclose(obj.calcCov()[3], np.einsum("tc,td->cd", obs[:, 3, :], np.conj(obs[:, 3, :])) / len(sel))
        mk = dsr.MkBeamformer(fftLen, C, kind); mk.setFixedWeights(inp["wq"], None)
        assert np.array_equal(obj.getWq(0, 2), inp["wq"][2]) and np.array_equal(obj.getB(0, 2), mk.getFixedWeights()[1][2]) and obj.getAlpha() == mk.alpha
        stats = torch.zeros((3, 1, F), dtype=torch.float64, device=cuda)
        wa, info, cost = mk.estimate(Xd, stats=stats, **kwsel)
        allw = obj.estimateAllActiveWeights()
        assert np.array_equal(allw, packed(wa)[0]) and np.array_equal(obj.lastInfo()[0], info[0].cpu().numpy())
        obj.resetStatistics()
        one = obj.estimateActiveWeights(3, np.zeros(2 * (C - 1)))
        assert np.array_equal(one, allw[3])
        obj.resetStatistics()
        x = 0.1 * np.random.default_rng(2).standard_normal(2 * (C - 1)); w = obj.UnpackWeights(x)
        assert np.array_equal(w[0], x[0::2] + 1j * x[1::2])
        full = np.zeros((1, F, C - 1), np.complex128); full[0, 3] = w[0]
        c, g = mk.eval(Xd, full, fbinX=3, **kwsel)
        wn = obj.normalizeWa(3, w)[0]
        assert obj.calcKurtosis(0, 3, w) == float(mk.alpha * np.sum(np.abs(wn) ** 2) - c[0, 3].item())
        gg = g[0, 3].cpu().numpy()
        assert np.array_equal(obj.gradient(0, 3, w), -((gg[0::2] + 1j * gg[1::2]) - mk.alpha * wn))
        d = mk_cases.delays(C, mk_cases.LOOK_DEG)
        obj.calcFixedWeights(mk_cases.FS, [d])
        bf = dsr.Beamformer(fftLen, C); bf.calcGSCWeights(mk_cases.FS, d)
        assert np.array_equal(obj.getWq(0, 5), bf.get(0)[5]) and np.array_equal(obj.getB(0, 5), bf.get(3)[5])
        obj.nextSpkr()
        assert obj.getSampleN() == 0


def test_refusals(dsr, cuda):
    from dsr.btk import mkBeamforming as M
    for kw, status in ((dict(halfBandShift=True), 1), (dict(NC=2), 1), (dict(nSource=2), 13)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.MkBeamformer(8, 4, **kw)
        assert e.value.status == status, kw
    with pytest.raises(dsr.DsrError) as e:
        dsr.MkBeamformer(8, 1)
    assert e.value.status == 5
    with pytest.raises(dsr.DsrError) as e:
        dsr.MkBeamformer(8, 65)
    assert e.value.status == 5
    X = torch.zeros((1, 4, 3, 5), dtype=torch.complex64, device=cuda)
    for cls in (M.MEKSubbandBeamformer_pr, M.MEKSubbandBeamformer_nrm):
        with pytest.raises(dsr.DsrError):
            cls(X[0], halfBandShift=True)
        with pytest.raises(dsr.DsrError):
            cls(X[0], NC=2)
    mk = dsr.MkBeamformer(8, 4)
    with pytest.raises(dsr.DsrError) as e:
        mk.estimate(X)                                                # no fixed weights yet
    assert e.value.status == 1
    with pytest.raises(dsr.DsrError) as e:
        mk.setFixedWeightsFromBeamformer(dsr.Beamformer(8, 4))        # before calcGSCWeights
    assert e.value.status == 1
    bf = dsr.Beamformer(16, 4); bf.calcGSCWeights(16000.0, np.zeros(4))
    with pytest.raises(dsr.DsrError) as e:
        mk.setFixedWeightsFromBeamformer(bf)
    assert e.value.status == 5
    mk.setFixedWeights(np.ones((5, 4)) / 4, None)
    with pytest.raises(dsr.DsrError) as e:
        mk.estimate(X, fbinX=5)
    assert e.value.status == 6
    with pytest.raises(dsr.DsrError) as e:
        mk.estimate(torch.zeros((1, 3, 3, 5), dtype=torch.complex64, device=cuda))
    assert e.value.status == 5
