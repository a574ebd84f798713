"""SubbandGSCRLS (k_gsc_rls, csrc/k_beamform.hip) in every cell its dispatch can select, on the ragged batches of tests/rls_cases.py: 9 utterances x 17 bins
= 153 series in three workgroups (the last one partial, utterance boundaries inside workgroups), frame counts full, shorter, 1 and 0
(tests/test_rls_cases_cpu.py shows that the cases are what they are named for and that each gate case lies on the named side).

Every case first asserts its cell through dsr_bf_rls_path (dsr.bf_rls_path), the helper the launch itself goes through.  What is compared:
  * one shot on the ragged batch with oracle.gsc_rls run per utterance on its own length: final active weights (rtol 1e-8 up to 8 channels, 1e-6
    above, atol 1e-11) and output (4e-6 of the largest reference magnitude) -- the project's bars (test_gsc_rls_ragged_and_carried); rows past an
    utterance's length are exactly 0, the utterance of 0 frames returns zero output and zero weights;
  * three carried blocks, the first of one frame, one live stream with 0 frames in the middle block, with the oracle run once over the whole stream;
  * after rlsResetState the first block repeats bit for bit;
  * one stream carried through the three residences (block 1 in registers, block 2 in LDS, block 3 in memory) with the one-shot oracle.

Template instance -> the case that launches it (tests/rls_cases.py):
  k_gsc_rls<4 | 6 | 8, true, 16>                  [regs4] [regs6] [regs8], [regs4_fixed] (adaptation off), test_carried_through_the_three_residences block 1
  k_gsc_rls<4 | 6 | 8, false, 16>, state in LDS   [lds4_noregs] [lds6_noregs] [lds8_noregs] (DSR_RLS_NOREGS), the three residences' block 2
  k_gsc_rls<4 | 6 | 8, false, 16>, in memory      [mem4_both] [mem6_both] [mem8_both] (DSR_RLS_NOREGS + DSR_RLS_MEMSTATE), the three residences' block 3
  k_gsc_rls<0, false, 16>, state in LDS           [lds2] (1 x 1 precision matrix), [lds5], [lds12] (135 168 bytes: the last size inside the gate), [lds5_fixed]
  k_gsc_rls<0, false, 16>, in memory, in place    [mem5_memstate] (DSR_RLS_MEMSTATE), [mem13] (159 744 bytes: the first size past it), [mem16], [mem13_fixed]
  k_gsc_rls<0, false, 64>, in memory, in place    [mem17_cap64] (the first size past the capacity of 16), [mem64_cap64]
Run with -s for the measured error of every case."""
import numpy as np
import pytest

from tests import rls_cases as RC

pytestmark = pytest.mark.gpu

_ID = dict(ids=lambda c: c["name"])
_REF = {}                                                                      # case -> design, snapshots and the oracle's runs, computed once


def _set_env(monkeypatch, env):
    for k in RC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_cell(dsr, case, expect=None):
    got = dsr.bf_rls_path(case["C"])[0]
    expect = expect or case["expect"]
    assert got == expect, "%s: the dispatch takes k_gsc_rls<%d, %s, %d> with the state in %s, the case is there for %s" % (
        case["name"], got[0], got[2] == RC.REGS, got[1], ("registers", "LDS", "memory")[got[2]], (expect,))


def _ref(oracle, bf, case):
    """design as the device holds it, snapshots, and the oracle per utterance on its own length: [(Y [n][F], wa [F][n])]"""
    if case["name"] not in _REF:
        _, _, wq_o, _ = RC.design(oracle, case["C"])
        wq = bf.get(0); B = bf.get(3)[:RC.F]
        assert np.abs(wq - wq_o).max() <= 1e-12
        X = RC.snapshots(case, wq_o)
        runs = [RC.oracle_run(oracle, case, X, wq, B, u, n) if n else (np.zeros((0, RC.F), complex), np.zeros((RC.F, case["C"] - 1), complex))
                for u, n in enumerate(RC.lens_of(case))]
        X.setflags(write=False)
        for y, w in runs:
            y.setflags(write=False); w.setflags(write=False)
        _REF[case["name"]] = (X, runs)
    return _REF[case["name"]]


def _beamformer(dsr, oracle, case):
    mp, delays, _, _ = RC.design(oracle, case["C"])
    bf = dsr.Beamformer(RC.M, case["C"]); bf.calcGSCWeights(16000.0, delays); bf.select(case["mode"]); bf.rlsConfig(RC.MYU, RC.SIGMA2)
    _start(bf, case)
    if case["qc"]:
        bf.setQuadraticConstraint(case["alpha"], case["qc"])
    bf.updateActiveWeightVecotrs(case["adapt"])
    return bf


def _start(bf, case):
    if case["p0"] == "set":
        for f, P in enumerate(RC.precision_start(case["C"])):
            bf.setPrecisionMatrix(f, P)
    else:
        bf.initPrecisionMatrix(RC.SIGMA2_INIT)


def _check(case, what, runs, lens, Y, wa):
    """the project's bars; Y [U][T][F] and wa [U][F][n] of the device against the oracle's runs; -> (weight error / bar, output error / bar), the worst"""
    tolw = 1e-8 if case["C"] <= 8 else 1e-6
    worst_w = worst_y = 0.0
    for u, n in enumerate(lens):
        Yo, wao = runs[u]
        assert np.all(Y[u][n:] == 0), "%s %s: utterance %d has non-zero rows past its %d frames" % (case["name"], what, u, n)
        assert np.isfinite(wa[u]).all() and np.isfinite(Y[u]).all()
        if n == 0:
            assert not wa[u].any(), "%s %s: the utterance of 0 frames has non-zero active weights" % (case["name"], what)
            continue
        assert not wa[u][0].any()                                            # bin 0 is never adapted
        err_w = np.abs(wa[u][1:] - wao[1:]); bar_w = 1e-11 + tolw * np.abs(wao[1:])
        worst_w = max(worst_w, float((err_w / bar_w).max()))
        worst_y = max(worst_y, float(np.abs(Y[u][:n] - Yo[:n]).max() / (4e-6 * np.abs(Yo).max())))
    print("%s %s: active weights at %.3g of their bar (rtol %g, atol 1e-11), output at %.3g of its bar (4e-6 of the largest magnitude)" % (
        case["name"], what, worst_w, tolw, worst_y))
    assert worst_w <= 1.0, "%s %s: active weights at %.3g times their bar" % (case["name"], what, worst_w)
    assert worst_y <= 1.0, "%s %s: output at %.3g times its bar" % (case["name"], what, worst_y)


@pytest.mark.parametrize("case", RC.CASES, **_ID)
def test_one_shot_on_the_ragged_batch(dsr, oracle, cuda, monkeypatch, case):
    import torch
    _set_env(monkeypatch, case["env"])
    _assert_cell(dsr, case)
    bf = _beamformer(dsr, oracle, case)
    X, runs = _ref(oracle, bf, case)
    lens = RC.lens_of(case)
    nf = torch.tensor(lens, dtype=torch.int32, device=cuda)
    Y, wa = bf.gsc_rls(torch.from_numpy(np.array(X)).to(cuda), nframes=nf)
    _check(case, "one shot", runs, lens, Y.cpu().numpy(), wa.cpu().numpy())
    if case["adapt"]:
        assert max(np.abs(w[1:]).max() for _, w in runs) > 1e-3                # (the adaptation moved the weights)
    else:
        assert not wa.cpu().numpy().any()


def _carried_blocks(bf, cuda, case, X, envs, monkeypatch, dsr):
    """the three blocks of the case with the state carried -> (Y of the whole stream [U][T][F], final active weights, the first block's Y and wa)"""
    import torch
    lens = RC.lens_of(case)
    Ys = []; first = None; wa = None
    for (lo, hi), (env, res) in zip(RC.blocks_of(case), envs):
        _set_env(monkeypatch, env)
        _assert_cell(dsr, case, case["expect"][:2] + (res,))
        nb = torch.tensor(RC.block_lens(lens, lo, hi), dtype=torch.int32, device=cuda)
        Yb, wa = bf.gsc_rls(torch.from_numpy(np.ascontiguousarray(X[:, :, lo:hi])).to(cuda), nframes=nb)
        Ys.append(Yb)
        if first is None:
            first = (Yb.clone(), wa.clone())
    return torch.cat(Ys, dim=1).cpu().numpy(), wa.cpu().numpy(), first


@pytest.mark.parametrize("case", RC.CASES, **_ID)
def test_three_carried_blocks_and_reset(dsr, oracle, cuda, monkeypatch, case):
    import torch
    _set_env(monkeypatch, case["env"])
    bf = _beamformer(dsr, oracle, case)
    X, runs = _ref(oracle, bf, case)
    lens = RC.lens_of(case)
    bf.rlsCarry(True)
    envs = [(case["env"], case["expect"][2])] * 3
    Y, wa, first = _carried_blocks(bf, cuda, case, X, envs, monkeypatch, dsr)
    # a stream's final weights are those after its own last frame: the blocks after it give it 0 frames and leave its state alone
    _check(case, "three carried blocks", runs, lens, Y, wa)
    bf.rlsResetState()                                                         # fresh streams start from P0 and zero weights again
    lo, hi = RC.blocks_of(case)[0]
    nb = torch.tensor(RC.block_lens(lens, lo, hi), dtype=torch.int32, device=cuda)
    Yr, wr = bf.gsc_rls(torch.from_numpy(np.ascontiguousarray(X[:, :, lo:hi])).to(cuda), nframes=nb)
    assert torch.equal(torch.view_as_real(Yr), torch.view_as_real(first[0])) and torch.equal(torch.view_as_real(wr), torch.view_as_real(first[1])), \
        "%s: the first block after rlsResetState is not the first block's bits" % case["name"]


def test_carried_through_the_three_residences(dsr, oracle, cuda, monkeypatch):
    """block 1 with the state in registers, block 2 in LDS, block 3 in memory (in place, in the carried array itself): one stream, the one-shot oracle"""
    case = RC.CROSS_CASE
    _set_env(monkeypatch, {})
    bf = _beamformer(dsr, oracle, case)
    X, runs = _ref(oracle, bf, case)
    bf.rlsCarry(True)
    Y, wa, _ = _carried_blocks(bf, cuda, case, X, RC.CROSS_ENVS, monkeypatch, dsr)
    _check(case, "registers -> LDS -> memory", runs, RC.lens_of(case), Y, wa)
