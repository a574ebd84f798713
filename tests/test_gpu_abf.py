"""The adaptive subband beamformers of btk/lib/subbandBeamforming.py (k_abf_gj, k_abf_smi, csrc/abf_kernels.hip) in every cell their dispatch can select,
on the ragged batches of tests/abf_cases.py: 9 utterances x 17 bins = 153 series in three workgroups (the last one partial, utterance boundaries
inside workgroups), frame counts full, shorter, 1 and 0 (tests/test_abf_np_cpu.py shows that the cases are what they are named for).

Every case first asserts its cell through dsr_abf_path, the helper the launch itself goes through.  The reference is the numpy restatement
(tests/abf_np.py) per utterance on its own length.  Tolerance -- nothing of it is taken from the device: 8 x the case's yardstick (the difference
of the restatement's two evaluations, floored at 1e-14), times the RMS of the compared quantity; it applies to the final fp64 weights and to the
output, which adds one float32 rounding of the reference value, 2^-22 |ref|, because Y is stored as complex64.  The factor 8: the device orders
its sums differently and uses Cholesky where the reference uses LU; both are backward stable with modest constants.
Run with -s for the yardstick, the measured error and the cell of every case."""
import numpy as np
import pytest

from tests import abf_cases as AC
from tests import abf_np as A
from tests import synth

pytestmark = pytest.mark.gpu

_ID = dict(ids=lambda c: c["name"])


@pytest.fixture(scope="module")
def abf(dsr):
    from dsr import _abf
    return _abf


def _set_env(monkeypatch, env):
    for k in AC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_cell(abf, case, expect=None):
    got = abf.abf_path(case["kind"], case["C"])[0]
    expect = expect or case["expect"]
    assert got == expect, "%s: the dispatch takes <%d, %s, %d> with the state in %s, the case is there for %s" % (
        case["name"], got[0], got[2] == AC.REGS, got[1], ("registers", "LDS", "memory")[got[2]], (expect,))
    return got


def _beamformer(abf, case, r):
    bf = abf.AdaptiveBeamformer(case["kind"], AC.M, case["C"], **case["params"])
    bf.setFixedWeights(r["wq"], r["B"])
    bf.reset()                                                                  # nextSpkr(): Griffiths-Jim has no state before it
    return bf


def _run(bf, cuda, case, r, lo=0, hi=None):
    """frames [lo, hi) of the batch -> (Y [U][hi-lo][F], final weights) as numpy; Y is NaN before the call, so unwritten rows show"""
    import torch
    lens = AC.lens_of(case); hi = case["T"] if hi is None else hi
    nb = torch.tensor(AC.block_lens(lens, lo, hi), dtype=torch.int32, device=cuda)
    kw = {}
    if r["wp"] is not None:
        wp = np.ones((AC.U, case["T"], AC.F), np.float32); wp[:, :case["wp"]] = r["wp"][:, :case["T"]]
        kw = dict(wp=torch.from_numpy(np.ascontiguousarray(wp[:, lo:hi])).to(cuda),
                  wpFrames=torch.full((AC.U,), int(min(max(case["wp"] - lo, 0), hi - lo)), dtype=torch.int32, device=cuda))
    Y = torch.full((AC.U, hi - lo, AC.F), float("nan"), dtype=torch.complex64, device=cuda)
    Y, w = bf.run(torch.from_numpy(np.array(r["X"][:, :, lo:hi])).to(cuda), nframes=nb, Y=Y, **kw)
    return Y.cpu().numpy(), w.cpu().numpy()


def _check(case, what, r, Y, w, cell):
    """-> the measured errors in units of the tolerance; asserts them, the zero rows and the untouched stream of 0 frames"""
    lens = AC.lens_of(case)
    ty, tw = 8 * max(r["yard_y"], 1e-14) * r["rms_y"], 8 * max(r["yard_w"], 1e-14) * r["rms_w"]
    worst_y = worst_w = 0.0
    for u, n in enumerate(lens):
        ref = r["runs"][u][0]
        assert np.all(Y[u][n:] == 0), "%s %s: utterance %d has rows past its %d frames that are not zero (NaN: never written)" % (case["name"], what, u, n)
        assert np.isfinite(Y[u]).all() and np.isfinite(w[u]).all(), "%s %s: utterance %d is not finite" % (case["name"], what, u)
        if n == 0:
            assert not w[u].any(), "%s %s: the stream of 0 frames does not return the state as created" % (case["name"], what)
            continue
        worst_y = max(worst_y, float((np.abs(Y[u][:n] - ref["Y"]) / (ty + 2.0 ** -22 * np.abs(ref["Y"]))).max()))
        worst_w = max(worst_w, float(np.abs(w[u] - ref["w"]).max() / tw))
    print("%s %s, cell %s: yardstick %.2e / %.2e (output / weights), output at %.3g of its tolerance, weights at %.3g (largest errors %.2e / %.2e of the RMS)" % (
        case["name"], what, cell, r["yard_y"], r["yard_w"], worst_y, worst_w,
        max(np.abs(Y[u][:n] - r["runs"][u][0]["Y"]).max() for u, n in enumerate(lens) if n) / r["rms_y"],
        max(np.abs(w[u] - r["runs"][u][0]["w"]).max() for u, n in enumerate(lens) if n) / r["rms_w"]))
    assert worst_y <= 1.0, "%s %s: output at %.3g times its tolerance" % (case["name"], what, worst_y)
    assert worst_w <= 1.0, "%s %s: final weights at %.3g times their tolerance" % (case["name"], what, worst_w)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("case", AC.CASES, **_ID)
def test_one_shot_blocks_and_reset(abf, cuda, monkeypatch, case):
    """one shot on the ragged batch against the restatement; then the three carried blocks, which equal the one shot bit for bit on the same cell
    (the middle block gives one live stream zero frames: its state stays); then reset, after which the first block repeats bit for bit"""
    _set_env(monkeypatch, case["env"])
    cell = _assert_cell(abf, case)
    r = AC.reference(case)
    bf = _beamformer(abf, case, r)
    Y, w = _run(bf, cuda, case, r)
    _check(case, "one shot", r, Y, w, cell)
    if case["kind"] == "gj":
        assert max(np.abs(ref["w"]).max() for ref, _ in r["runs"]) > 1e-3       # (the adaptation moved the weights)
    bf.carry(True); bf.reset()
    parts = [_run(bf, cuda, case, r, lo, hi) for lo, hi in AC.blocks_of(case)]
    Yb = np.concatenate([p[0] for p in parts], axis=1)
    assert np.array_equal(_bits(Yb), _bits(Y)), "%s: the carried blocks are not the one-shot run's bits" % case["name"]
    assert np.array_equal(_bits(parts[-1][1]), _bits(w)), "%s: the final weights after the carried blocks are not the one-shot run's bits" % case["name"]
    bf.reset()
    lo, hi = AC.blocks_of(case)[0]
    Yr, wr = _run(bf, cuda, case, r, lo, hi)
    assert np.array_equal(_bits(Yr), _bits(parts[0][0])) and np.array_equal(_bits(wr), _bits(parts[0][1])), \
        "%s: the first block after reset is not the first block's bits" % case["name"]


@pytest.mark.parametrize("case", AC.CROSS_CASES, **_ID)
def test_carried_through_the_three_residences(abf, cuda, monkeypatch, case):
    """block 1 with the state in registers, block 2 in LDS, block 3 in memory: one stream, the one-shot restatement"""
    _set_env(monkeypatch, {})
    r = AC.reference(case)
    bf = _beamformer(abf, case, r); bf.carry(True)
    parts = []
    for (lo, hi), (env, res) in zip(AC.blocks_of(case), AC.CROSS_ENVS):
        _set_env(monkeypatch, env)
        _assert_cell(abf, case, case["expect"][:2] + (res,))
        parts.append(_run(bf, cuda, case, r, lo, hi))
    _check(case, "registers -> LDS -> memory", r, np.concatenate([p[0] for p in parts], axis=1), parts[-1][1], "all three")


def test_carried_state_of_another_batch_size_is_refused(dsr, abf, cuda):
    case = AC.CASES[0]; r = AC.reference(case)
    bf = _beamformer(abf, case, r); bf.carry(True)
    _run(bf, cuda, case, r)
    import torch
    with pytest.raises(dsr.DsrError) as e:
        bf.run(torch.from_numpy(np.array(r["X"][:4])).to(cuda))
    assert e.value.status == dsr.E_CONSISTENCY
    bf.reset()
    bf.run(torch.from_numpy(np.array(r["X"][:4])).to(cuda))


def test_griffiths_jim_needs_next_spkr_first(dsr, abf, cuda):
    import torch
    case = AC.CASES[0]; r = AC.reference(case)
    bf = abf.AdaptiveBeamformer("gj", AC.M, case["C"], **case["params"]); bf.setFixedWeights(r["wq"], r["B"])
    with pytest.raises(dsr.DsrError) as e:
        bf.run(torch.from_numpy(np.array(r["X"])).to(cuda))
    assert e.value.status == 1


@pytest.mark.parametrize("case", [c for c in AC.CASES if c["kind"] != "gj" and c["params"]["end"] == 20 and c["T"] == 40 and not c["wp"]
                                  and c["name"].split("_")[1] in ("regs4", "regs8", "lds5", "mem12")], **_ID)
def test_frozen_weights_are_a_plain_apply(dsr, abf, cuda, monkeypatch, case):
    """after frame `end` the output is the fixed-weight apply with the returned weights: MPDR's wq - B wa through the existing per-utterance apply
    (MkBeamformer.apply, weights rounded to fp32), MVDR's w through the fixed-weight kind of this handle and against w^H x in numpy"""
    import torch
    _set_env(monkeypatch, case["env"])
    r = AC.reference(case); lens = AC.lens_of(case); end = case["params"]["end"]
    bf = _beamformer(abf, case, r)
    Y, w = _run(bf, cuda, case, r)
    Xd = torch.from_numpy(np.array(r["X"])).to(cuda)
    X = r["X"].astype(np.complex128)
    if case["kind"] == "mpdr":
        mk = dsr.MkBeamformer(AC.M, case["C"]); mk.setFixedWeights(r["wq"], r["B"])
        Ya = mk.apply(Xd, torch.from_numpy(w).to(cuda)).cpu().numpy()
        weff = r["wq"][None] - np.einsum("fcj,ufj->ufc", r["B"], w)
    else:
        Ya = np.zeros_like(Y); weff = w
        ds = abf.AdaptiveBeamformer("ds", AC.M, case["C"])
        for u in range(AC.U):
            ds.setFixedWeights(w[u]); Ya[u] = ds.run(Xd[u:u + 1])[0][0].cpu().numpy()
    # float32 rounding: of a weight, of its product, of C - 1 additions, and of the stored value on either side
    bound = (case["C"] + 3) * 2.0 ** -24 * np.einsum("ufc,uctf->utf", np.abs(weff), np.abs(X))
    Yn = np.einsum("ufc,uctf->utf", np.conj(weff), X)
    seen = 0
    for u, n in enumerate(lens):
        if n > end + 1:
            sl = slice(end + 1, n); seen += 1
            assert np.all(np.abs(Y[u][sl] - Ya[u][sl]) <= bound[u][sl] + 1e-30), "%s: utterance %d differs from the fixed-weight apply" % (case["name"], u)
            assert np.all(np.abs(Y[u][sl] - Yn[u][sl]) <= bound[u][sl] + 1e-30)
    assert seen >= 3


@pytest.mark.parametrize("NC", [1, 2])
def test_fixed_weight_kinds(abf, cuda, NC):
    """SubbandBeamformerDS and SubbandBeamformerGSC (one and two constraints, the null-steering design) against the restatement, wp shorter than the batch"""
    import torch
    Cn, T = 5, 13
    case = dict(C=Cn, T=T, kind="mvdr", name="static%d" % NC, scale=1.0)
    delays, wq, B = AC.design(Cn)
    if NC == 2:
        d2 = A.calcDelays(-300.0, 1200.0, 100.0, synth.linear_array(Cn, 25.0))
        wq = np.array([A.calcNullBeamformer(A.calcArrayManifold_f(f, AC.M, Cn, 16000.0, delays, norm=False),
                                            A.calcArrayManifold_f(f, AC.M, Cn, 16000.0, d2, norm=False), 2) for f in range(AC.F)])
        B = np.array([A.calcBlockingMatrix(wq[f], 2) for f in range(AC.F)])
    X = AC.snapshots(case, wq); lens = AC.lens_of(case)
    rng = np.random.default_rng(3); wa = 0.3 * (rng.standard_normal((AC.F, Cn - NC)) + 1j * rng.standard_normal((AC.F, Cn - NC)))
    wp = rng.uniform(0.2, 1.0, (AC.U, T, AC.F)).astype(np.float32); nwp = 7
    Xd = torch.from_numpy(X).to(cuda); nf = torch.tensor(lens, dtype=torch.int32, device=cuda)
    kw = dict(nframes=nf, wp=torch.from_numpy(wp).to(cuda), wpFrames=torch.full((AC.U,), nwp, dtype=torch.int32, device=cuda))
    for kind in (["ds", "gsc"] if NC == 1 else ["gsc"]):
        bf = abf.AdaptiveBeamformer(kind, AC.M, Cn, NC=NC); bf.setFixedWeights(wq, B)
        if kind == "gsc":
            bf.setActiveWeights(wa)
            wqd, Bd = bf.getFixedWeights()
            assert np.array_equal(wqd, wq) and np.array_equal(Bd, B)
        Y = torch.full((AC.U, T, AC.F), float("nan"), dtype=torch.complex64, device=cuda)
        Y = bf.run(Xd, Y=Y, **kw)[0].cpu().numpy()
        for u, n in enumerate(lens):
            w = wp[u][:nwp].astype(np.float64)
            ref = A.static_ds(X[u][:, :n], wq, w) if kind == "ds" else A.static_gsc(X[u][:, :n], wq, B, wa, w)
            assert np.all(Y[u][n:] == 0)
            if n:
                assert np.all(np.abs(Y[u][:n] - ref) <= 8e-14 * AC.rms(ref) + 2.0 ** -22 * np.abs(ref)), (kind, u)


def test_facade_end_to_end(dsr, abf, cuda, protos, headset):
    """dsr.btk.subbandBeamforming over analysis banks on the headset recording, 4 channels: each adaptive class's iterator equals the batch face,
    and the upper half of every vector is the conjugate mirror"""
    import torch
    from dsr.btk import subbandBeamforming as SB
    from dsr.btk.feature import SampleFeaturePtr
    from dsr.btk.modulated import OverSampledDFTAnalysisBankPtr
    M, m, r, h, g = protos["M256-m4-r1"]; D = M >> r; Fh = M // 2 + 1; Cn = 4
    n = 2 * m * M                                                               # two analysis banks' worth of samples
    rng = np.random.default_rng(8)
    x = np.stack([headset[4000 + 2 * c: 4000 + 2 * c + n] + 30.0 * rng.standard_normal(n) for c in range(Cn)]).astype(np.float32)

    def banks():
        out = []
        for c in range(Cn):
            s = SampleFeaturePtr(blockLen=D, shiftLen=D, padZeros=True); s.setSamples(x[c], 16000)
            out.append(OverSampledDFTAnalysisBankPtr(s, h, M, m, r))
        return out
    X = np.stack([np.array([np.array(v) for v in b]) for b in banks()])[:, :, :Fh].astype(np.complex64)         # [C][T][F]
    T = X.shape[1]
    assert T >= 2 * m
    delays = SB.calcDelays(500.0, 1200.0, 0.0, synth.linear_array(Cn, 40.0))
    wp = [np.full(M, 0.5 + 0.01 * t) for t in range(T)]
    made = [("gj", lambda s: SB.SubbandBeamformerGriffithsJim(s, staticAfter=T // 2), dict(staticAfter=T // 2), wp[:5]),
            ("mvdr", lambda s: SB.SubbandBeamformerMVDR(s, halfBandShift=False, end=T // 2, wp1L=wp), dict(end=T // 2), wp),
            ("mpdr", lambda s: SB.SubbandBeamformerMPDR(s, halfBandShift=False, end=T // 2), dict(end=T // 2), [])]
    for kind, make, params, wps in made:
        fac = make(banks())
        fac.calcArrayManifoldVectors(16000.0, delays)
        if kind == "gj":
            fac.setWp(wps)
        fac.nextSpkr()
        rows = np.array(list(fac))
        assert rows.shape == (T, M) and fac.size() == M
        assert np.array_equal(rows[:, Fh:], np.conj(rows[:, 1:Fh - 1][:, ::-1])), kind
        wq = np.array([SB.calcArrayManifold_f(f, M, Cn, 16000.0, delays, False) for f in range(Fh)])
        bf = abf.AdaptiveBeamformer(kind, M, Cn, **params); bf.setFixedWeights(wq); bf.reset()
        kw = {}
        if len(wps):
            w = np.ones((1, T, Fh), np.float32); w[0, :len(wps)] = np.array(wps)[:, :Fh]
            kw = dict(wp=torch.from_numpy(w).to(cuda), wpFrames=torch.tensor([len(wps)], dtype=torch.int32, device=cuda))
        Y, wfin = bf.run(torch.from_numpy(X)[None].to(cuda), **kw)
        assert np.array_equal(rows[:, :Fh], Y[0].cpu().numpy().astype(np.complex128)), kind
        assert np.isfinite(rows).all() and np.abs(rows).max() > 0
        assert np.array_equal(np.array(fac._weights()), wfin[0].cpu().numpy())
