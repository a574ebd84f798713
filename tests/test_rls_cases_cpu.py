"""The cases of tests/rls_cases.py are what tests/test_gpu_rls_kernels.py takes them for -- conditions on the dispatch and on the INPUTS, checked
without a GPU (no kernel is involved):
  * the library's query (dsr_bf_rls_path, the helper gsc_rls_apply launches from) returns the cell every case is named for, and the same cell
    follows from the formulas stated here: state bytes (n^2 + n) x 16 x 64 against the 150 KB gate (C <= 12 | 13), vector capacity 16 | 64
    (C <= 16 | 17), register instances at C = 4, 6, 8; every gate case lies on the named side;
  * every row of the dispatch table has a case, every residence meets qctype 0 / 1 / 2, gsc_norm, adaptation off and a setPrecisionMatrix start;
  * the batches are ragged as named (full, shorter, 1 frame, 0 frames) and the middle carried block gives one live stream 0 frames;
  * for every qctype 2 case the numpy restatement of test_gsc_rls_against_numpy takes the threshold constraint at least 5 times and leaves it
    idle at least 5 times, and ends in the oracle's active weights (so the count is of the computation the GPU test compares with).
Run with -s for the counts."""
import numpy as np
import pytest

from tests import rls_cases as RC

_ID = dict(ids=lambda c: c["name"])


def _set_env(monkeypatch, env):
    for k in RC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def cell_from(C, env):
    """the dispatch as DESIGN 4.4e states it"""
    n = C - 1
    stateBytes = (n * n + n) * 16 * 64
    ct = C if C in (4, 6, 8) else 0
    cap = 16 if C <= 16 else 64
    if ct and "DSR_RLS_NOREGS" not in env:
        res = RC.REGS
    elif stateBytes <= RC.LDS_GATE and "DSR_RLS_MEMSTATE" not in env:
        res = RC.LDS
    else:
        res = RC.MEM
    return (ct, cap, res), stateBytes


@pytest.mark.parametrize("case", RC.CASES + [RC.CROSS_CASE], **_ID)
def test_case_reaches_the_cell_it_names(dsr, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    want, stateBytes = cell_from(case["C"], case["env"])
    assert want == case["expect"], (case["name"], want)
    got, lds = dsr.bf_rls_path(case["C"])
    assert got == case["expect"], "%s: the dispatch takes k_gsc_rls<%d, %s, %d> with the state in %s" % (
        case["name"], got[0], got[2] == RC.REGS, got[1], ("registers", "LDS", "memory")[got[2]])
    assert lds == (stateBytes, stateBytes if want[2] == RC.LDS else 0)
    for gate, inside in case["gates"].items():
        if gate == "lds":
            assert (stateBytes <= RC.LDS_GATE) == inside, (stateBytes, RC.LDS_GATE)
        else:
            assert gate == "cap16" and (case["C"] <= 16) == inside
    name = case["name"]
    assert name.startswith(("regs", "lds", "mem", "cross")) and (not name.startswith("regs") or want[2] == RC.REGS)
    assert (not name.startswith("lds") or want[2] == RC.LDS) and (not name.startswith("mem") or want[2] == RC.MEM)


def test_gates_are_met_from_both_sides(dsr, monkeypatch):
    """12 | 13 by LDS bytes, 16 | 17 by capacity, and the register instances against their neighbours; the state's bytes grow past the gate between 12 and 13"""
    _set_env(monkeypatch, {})
    by = {c["C"]: c for c in RC.CASES if not c["env"] and c["adapt"]}
    assert by[12]["expect"][2] == RC.LDS and by[13]["expect"][2] == RC.MEM
    assert dsr.bf_rls_path(12)[1][0] <= RC.LDS_GATE < dsr.bf_rls_path(13)[1][0]
    assert by[16]["expect"][1] == 16 and by[17]["expect"][1] == 64 and by[16]["expect"][2] == by[17]["expect"][2] == RC.MEM
    for C in range(2, 65):
        assert dsr.bf_rls_path(C)[0] == cell_from(C, {})[0], C
    for env in (RC.NOREGS, RC.MEMSTATE, RC.BOTH):
        _set_env(monkeypatch, env)
        for C in range(2, 65):
            assert dsr.bf_rls_path(C)[0] == cell_from(C, env)[0], (C, env)


def test_every_cell_and_every_variant_is_covered():
    cells = {(c["expect"], tuple(sorted(c["env"]))) for c in RC.CASES}
    rows = {(e[0] != 0, e[1], e[2]) for e, _ in cells}
    # the six rows of the dispatch table: <C, true, 16>; <C, false, 16> in LDS / in memory; <0, false, 16> in LDS / in memory; <0, false, 64>
    assert rows == {(True, 16, RC.REGS), (True, 16, RC.LDS), (True, 16, RC.MEM), (False, 16, RC.LDS), (False, 16, RC.MEM), (False, 64, RC.MEM)}
    for res in (RC.REGS, RC.LDS, RC.MEM):                                    # every compile-time instance in every residence
        assert {c["C"] for c in RC.CASES if c["expect"][2] == res and c["expect"][0]} == {4, 6, 8}
    assert {c["C"] for c in RC.CASES if c["expect"] == (0, 16, RC.LDS)} == {2, 5, 12}
    assert {c["C"] for c in RC.CASES if c["expect"] == (0, 16, RC.MEM)} == {5, 13, 16}
    assert {c["C"] for c in RC.CASES if c["expect"] == (0, 64, RC.MEM)} == {17, 64}
    for res in (RC.REGS, RC.LDS, RC.MEM):
        cs = [c for c in RC.CASES if c["expect"][2] == res]
        assert {c["qc"] for c in cs if c["adapt"]} == {0, 1, 2}
        assert any(c["mode"] == "gsc_norm" and c["adapt"] for c in cs) and any(not c["adapt"] for c in cs) and any(c["p0"] == "set" for c in cs)
    assert [res for _, res in RC.CROSS_ENVS] == [RC.REGS, RC.LDS, RC.MEM]


def test_switches_are_read_on_every_call(dsr, monkeypatch):
    _set_env(monkeypatch, {})
    assert dsr.bf_rls_path(6)[0] == (6, 16, RC.REGS)
    monkeypatch.setenv("DSR_RLS_NOREGS", "1")
    assert dsr.bf_rls_path(6)[0] == (6, 16, RC.LDS)
    monkeypatch.setenv("DSR_RLS_MEMSTATE", "1")
    assert dsr.bf_rls_path(6)[0] == (6, 16, RC.MEM)
    monkeypatch.delenv("DSR_RLS_NOREGS")
    assert dsr.bf_rls_path(6)[0] == (6, 16, RC.REGS) and dsr.bf_rls_path(5)[0] == (0, 16, RC.MEM)
    monkeypatch.delenv("DSR_RLS_MEMSTATE")
    assert dsr.bf_rls_path(5)[0] == (0, 16, RC.LDS)
    for C in (1, 65):
        with pytest.raises(dsr.DsrError):
            dsr.bf_rls_path(C)


def test_path_codes_are_the_headers(dsr):
    import os
    import re
    from tests.conftest import ROOT
    assert (RC.REGS, RC.LDS, RC.MEM) == (dsr.RLS_STATE_REGS, dsr.RLS_STATE_LDS, dsr.RLS_STATE_MEM)
    hdr = open(os.path.join(ROOT, "include", "dsr.h")).read()
    for name, val in (("REGS", 0), ("LDS", 1), ("MEM", 2)):
        assert re.search(r"\bDSR_RLS_STATE_%s\s*=\s*%d\b" % (name, val), hdr), name


@pytest.mark.parametrize("case", RC.CASES + [RC.CROSS_CASE], **_ID)
def test_batches_are_ragged_as_named(case):
    lens = RC.lens_of(case); T = case["T"]
    assert len(lens) == RC.U and RC.U * RC.F == 153 and RC.F % 64 and (RC.U * RC.F) % 64       # three workgroups, the last partial, boundaries inside
    assert max(lens) == T and lens.count(T) >= 2 and 0 in lens and 1 in lens and any(1 < n < T for n in lens) and min(lens) >= 0
    blocks = RC.blocks_of(case)
    assert blocks[0] == (0, 1) and blocks[-1][1] == T and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:])) and len(blocks) == 3
    mid = RC.block_lens(lens, *blocks[1]); first = RC.block_lens(lens, *blocks[0])
    assert any(f == 1 and m == 0 for f, m in zip(first, mid)), "no live stream with 0 frames in the middle block"
    assert sum(sum(RC.block_lens(lens, *b)) for b in blocks) == sum(lens)


@pytest.mark.parametrize("case", [c for c in RC.CASES + [RC.CROSS_CASE] if c["qc"] == 2], **_ID)
def test_threshold_constraint_is_taken_and_idle(oracle, case):
    _, _, wq, B = RC.design(oracle, case["C"])
    X = RC.snapshots(case, wq)
    taken = idle = 0; worst = 0.0
    for u, n in enumerate(RC.lens_of(case)):
        if n == 0:
            continue
        wa, a, b = RC.rls_numpy(case, X[u][:, :n], wq, B)
        taken += a; idle += b
        _, wao = RC.oracle_run(oracle, case, X, wq, B, u, n)
        worst = max(worst, float(np.abs(wao[1:] - wa[1:]).max()))
    print("%s (alpha %g): threshold constraint taken on %d steps, idle on %d; oracle against numpy restatement %.3g" % (
        case["name"], case["alpha"], taken, idle, worst))
    assert taken >= 5 and idle >= 5, (taken, idle)
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("case", [c for c in RC.CASES if c["p0"] == "set"][:2], **_ID)
def test_precision_start_is_hermitian_positive_definite(case):
    P = RC.precision_start(case["C"])
    assert np.abs(P - np.conj(np.swapaxes(P, 1, 2))).max() < 1e-12 and np.linalg.eigvalsh(P).min() > 1.0
    assert np.abs(P[3] - P[3][0, 0] * np.eye(case["C"] - 1)).max() > 1.0 or case["C"] == 2
