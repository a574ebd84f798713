"""The cases of tests/pf_dispatch_cases.py are what tests/test_gpu_postfilter_kernels.py takes them for -- conditions on the dispatch and on the INPUTS,
checked without a GPU (no kernel is involved):
  * the library's query (dsr_zelinski_path, the helper the launches go through) returns the cell every case is named for, the same cell follows from
    the dispatch as stated here, and every gate case lies on the named side of "C in {2, 3, 4, 6, 8}" and of "C <= 16";
  * every row of the dispatch table and every template instance has a case;
  * the sum kernels' frame counts are the ladder 1, 2, 15, 16, 17, 31, 33, 129, 272, the ragged lengths end inside a stretch, on a stretch edge, at
    ceil(Tmax / 2) and either side of it, and at 0; the carried blocks start with one frame and give k_zel_recur an empty last stretch with state carried in;
  * with the oracle, the inputs have teeth: "aligned" puts the Zelinski weight strictly inside (1e-4, 1) on at least 90 % of (frame, bin), "incoherent"
    with type 1 puts it on the 1e-4 floor on at least 30 %, "edge" puts it within 1e-6 of 1 everywhere; McCowan on "aligned" reaches its upper clamp on
    at least 5 % with type 2 and the floor on at least 5 % with type 1; the coherence clip R_ij > threshold is taken on some pairs and not on others.
Run with -s for the measured shares."""
import numpy as np
import pytest

from tests import pf_dispatch_cases as PC

_ID = dict(ids=lambda c: c["name"])


def _set_env(monkeypatch, env):
    for k in PC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def cell_from(kind, C, env, behind_fixed_bf):
    """the dispatch as DESIGN states it"""
    inset = C in PC.REG_SET
    if kind == 0 and (not inset or "DSR_PF_SUM" in env):
        return (PC.ZEL_SUM_BF if behind_fixed_bf and "DSR_PF_NOFUSE" not in env else PC.ZEL_SUM, 0)
    if C > 16 or "DSR_PF_WAVE" in env:
        return (PC.WAVE, kind)
    if kind >= 1:
        return (PC.MCCOWAN_REG, C) if inset and "DSR_PF_MEMSTATE" not in env else (PC.MCCOWAN_MEM, 0)
    return (PC.ZEL_REG, C)


@pytest.mark.parametrize("case", PC.ALL_CASES, **_ID)
def test_case_reaches_the_cell_it_names(dsr, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    bf = dsr.Beamformer(PC.M, case["C"]) if case["bf"] else None
    want = cell_from(case["kind"], case["C"], case["env"], bf is not None)
    assert want == case["expect"], (case["name"], want)
    got = dsr.zelinski_path(case["kind"], case["C"], bf)
    assert got == case["expect"], "%s: the dispatch takes %s with template argument %d, the case is there for %s with %d" % (
        case["name"], PC.CELL_NAMES[got[0]], got[1], PC.CELL_NAMES[case["expect"][0]], case["expect"][1])
    if case["inset"] is not None:
        assert (case["C"] in PC.REG_SET) == case["inset"]
    if bf is not None:                                                       # the twin of a fused case; an adapting beamformer has no fixed weights to fuse
        monkeypatch.setenv("DSR_PF_NOFUSE", "1")
        assert dsr.zelinski_path(0, case["C"], bf) == (PC.ZEL_SUM, 0)
        monkeypatch.delenv("DSR_PF_NOFUSE")
        assert dsr.zelinski_path(0, case["C"], None) == (PC.ZEL_SUM, 0)
        bf.rlsConfig(0.95, 0.01)
        assert dsr.zelinski_path(0, case["C"], bf) == (PC.ZEL_SUM, 0)


def test_gates_are_met_from_both_sides(dsr, monkeypatch):
    for env in ({}, PC.SUM, PC.NOFUSE, PC.WAVE_ENV, PC.MEMSTATE, dict(PC.SUM, **PC.WAVE_ENV), dict(PC.WAVE_ENV, **PC.MEMSTATE)):
        _set_env(monkeypatch, env)
        for kind in (0, 1, 2):
            bf = None
            for C in range(2, 65):
                assert dsr.zelinski_path(kind, C, bf) == cell_from(kind, C, env, False), (kind, C, env)
        for C in (2, 5, 8, 17):
            assert dsr.zelinski_path(0, C, dsr.Beamformer(PC.M, C)) == cell_from(0, C, env, True), (C, env)
    _set_env(monkeypatch, {})
    # in set | not in set: every member of the set has a neighbour outside it among the cases, for the Zelinski and the McCowan kernels
    for kind, inside, outside in ((0, PC.ZEL_REG, PC.ZEL_SUM), (1, PC.MCCOWAN_REG, PC.MCCOWAN_MEM), (2, PC.MCCOWAN_REG, PC.MCCOWAN_MEM)):
        cs = [c for c in PC.ALL_CASES if c["kind"] == kind and not c["env"] and not c["bf"]]
        assert {c["C"] for c in cs if c["expect"][0] == inside} == set(PC.REG_SET)
        assert {5} <= {c["C"] for c in cs if c["expect"][0] == outside}
        if kind:
            assert {c["C"] for c in cs if c["expect"][0] == outside} == {5, 7, 16}                 # 5 and 7: between members of the set
    # C <= 16 | 17: McCowan / Lefkimmiatis leave the thread kernels, Zelinski stays with the sum kernels
    for kind in (1, 2):
        assert dsr.zelinski_path(kind, 16, None) == (PC.MCCOWAN_MEM, 0) and dsr.zelinski_path(kind, 17, None) == (PC.WAVE, kind)
    assert dsr.zelinski_path(0, 16, None) == dsr.zelinski_path(0, 17, None) == (PC.ZEL_SUM, 0)
    for args in ((3, 4), (-1, 4), (0, 1), (0, 65)):
        with pytest.raises(dsr.DsrError):
            dsr.zelinski_path(args[0], args[1], None)


def test_every_cell_and_every_instance_is_covered():
    def sizes(cases, cell, env=None):
        return sorted(c["C"] for c in cases if c["expect"][0] == cell and (env is None or c["env"] == env))
    assert sizes(PC.ZEL_CASES, PC.ZEL_REG) == [2, 3, 4, 6, 8]
    assert sorted(set(sizes(PC.ZEL_CASES, PC.ZEL_SUM, {}))) == [5, 16, 17, 64] and sorted(set(sizes(PC.ZEL_CASES, PC.ZEL_SUM, PC.SUM))) == [2, 8]
    assert {(c["C"], c["bf"]) for c in PC.ZEL_BF_CASES} == {(5, "ds"), (5, "mvdr"), (17, "ds"), (17, "mvdr")}
    assert [(c["C"], c["expect"]) for c in PC.ZEL_WAVE_CASES] == [(3, (PC.WAVE, 0)), (8, (PC.WAVE, 0))]
    for kind, reg, mem, wave in ((1, PC.MC_REG_CASES, PC.MC_MEM_CASES, PC.MC_WAVE_CASES), (2, PC.LF_REG_CASES, PC.LF_MEM_CASES, PC.LF_WAVE_CASES)):
        assert [(c["C"], c["expect"]) for c in reg] == [(C, (PC.MCCOWAN_REG, C)) for C in PC.REG_SET]
        assert sizes(mem, PC.MCCOWAN_MEM, {}) == [5, 7, 16] and sizes(mem, PC.MCCOWAN_MEM, PC.MEMSTATE) == [4, 8]
        assert sizes(wave, PC.WAVE, {}) == [17, 64] and sizes(wave, PC.WAVE, PC.WAVE_ENV) == [4, 8]
        assert all(c["kind"] == kind and c["expect"][1] == kind for c in wave)
    # parameters: both alphas, both types, minFrames 0 and 5 within every group of kernels
    for group in (PC.ZEL_REG_CASES, PC.ZEL_SUM_CASES, PC.MC_REG_CASES, PC.MC_MEM_CASES, PC.LF_REG_CASES, PC.LF_MEM_CASES):
        assert {c["alpha"] for c in group} == {0.0, 0.7} and {c["type"] for c in group} == {1, 2} and {c["minFrames"] for c in group} == {0, 5}
    for group in (PC.ZEL_BF_CASES, PC.ZEL_WAVE_CASES, PC.MC_WAVE_CASES, PC.LF_WAVE_CASES):
        assert {c["type"] for c in group} == {1, 2} and {c["minFrames"] for c in group} == {0, 5}
    assert {c["family"] for c in PC.ZEL_REG_CASES} == {c["family"] for c in PC.ZEL_SUM_CASES} == {"aligned", "incoherent", "edge"}


def test_switches_are_read_on_every_call(dsr, monkeypatch):
    _set_env(monkeypatch, {})
    assert dsr.zelinski_path(0, 8, None) == (PC.ZEL_REG, 8) and dsr.zelinski_path(1, 8, None) == (PC.MCCOWAN_REG, 8)
    monkeypatch.setenv("DSR_PF_SUM", "1")
    assert dsr.zelinski_path(0, 8, None) == (PC.ZEL_SUM, 0) and dsr.zelinski_path(1, 8, None) == (PC.MCCOWAN_REG, 8)
    monkeypatch.delenv("DSR_PF_SUM"); monkeypatch.setenv("DSR_PF_MEMSTATE", "1")
    assert dsr.zelinski_path(0, 8, None) == (PC.ZEL_REG, 8) and dsr.zelinski_path(2, 8, None) == (PC.MCCOWAN_MEM, 0)
    monkeypatch.setenv("DSR_PF_WAVE", "1")
    assert dsr.zelinski_path(0, 8, None) == (PC.WAVE, 0) and dsr.zelinski_path(2, 8, None) == (PC.WAVE, 2)
    monkeypatch.delenv("DSR_PF_WAVE"); monkeypatch.delenv("DSR_PF_MEMSTATE")
    assert dsr.zelinski_path(0, 8, None) == (PC.ZEL_REG, 8) and dsr.zelinski_path(2, 8, None) == (PC.MCCOWAN_REG, 8)


def test_path_codes_are_the_headers(dsr):
    import os
    import re
    from tests.conftest import ROOT
    assert (PC.ZEL_REG, PC.ZEL_SUM, PC.ZEL_SUM_BF, PC.MCCOWAN_REG, PC.MCCOWAN_MEM, PC.WAVE) == (
        dsr.PF_ZEL_REG, dsr.PF_ZEL_SUM, dsr.PF_ZEL_SUM_BF, dsr.PF_MCCOWAN_REG, dsr.PF_MCCOWAN_MEM, dsr.PF_WAVE)
    hdr = open(os.path.join(ROOT, "include", "dsr.h")).read()
    for name, val in (("ZEL_REG", 0), ("ZEL_SUM", 1), ("ZEL_SUM_BF", 2), ("MCCOWAN_REG", 3), ("MCCOWAN_MEM", 4), ("WAVE", 5)):
        assert re.search(r"\bDSR_PF_%s\s*=\s*%d\b" % (name, val), hdr), name


def test_time_axis_of_the_sum_kernels():
    sums = PC.ZEL_SUM_CASES + PC.ZEL_BF_CASES
    assert {c["Tmax"] for c in PC.ZEL_SUM_CASES} == set(PC.LADDER)
    assert {PC.stretch(T) for T in (129, 272)} == {9, 17}                    # longer than the 8-frame prefetch: a second and a third batch
    for c in sums:
        T, lens = c["Tmax"], c["lens"]; L = PC.stretch(T); H = (T + 1) // 2
        assert len(lens) == PC.U and max(lens) == T == lens[0] and 0 in lens and min(lens) >= 0
        assert {min(max(H - 1, 0), T), H, min(H + 1, T)} <= set(lens)
        if L >= 2:
            assert any(0 < n < T and n % L for n in lens), "no length ends inside a stretch"
        if T > 2:
            assert any(0 < n < T and n % L == 0 for n in lens), "no length ends on a stretch edge"
    # an empty last stretch (Tmax <= 15 L) met with carried state: as a one-shot batch and as a carried block of 1, 17 or 33 frames
    empty_last = lambda T: T <= 15 * PC.stretch(T)
    assert all(empty_last(T) for T in (1, 17, 33)) and not empty_last(16) and not empty_last(272)
    second = {c["blocks"][1][1] - c["blocks"][1][0] for c in sums if len(c["blocks"]) > 1}
    assert second == {1, 17, 33}
    for c in PC.ALL_CASES:
        b = c["blocks"]; L = PC.stretch(c["Tmax"])
        assert b[0] == (0, 1) and b[-1][1] == c["Tmax"] and all(x[1] == y[0] and x[0] < x[1] for x, y in zip(b, b[1:] + [(c["Tmax"], 0)]))
        assert sum(sum(PC.block_lens(c["lens"], lo, hi)) for lo, hi in b) == sum(c["lens"])
        if len(b) == 4 and L >= 2:
            assert b[2][1] % L, "the last cut is on a stretch edge"
        if len(b) > 1:                                                       # a live stream with 0 frames in a middle block
            assert any(f == 1 and m == 0 for f, m in zip(PC.block_lens(c["lens"], *b[0]), PC.block_lens(c["lens"], *b[1])))
        if c["minFrames"]:
            assert c["minFrames"] == 5 and (c["Tmax"] < 7 or b[1][0] <= 6)   # frame index 6 is the first one filtered: past the first block
    assert PC.U * PC.F == 153 and PC.F % 64 and PC.F % 128


def _weights(oracle, case):
    """the oracle's weights over the valid (frame, bin) of the case"""
    wq = PC.manifold(oracle, case); X = PC.snapshots(case, wq); Y = PC.beamformed(X, wq)
    R = lam = None
    if case["kind"]:
        R = PC.coherence(oracle, case)
        if case["kind"] == 2:
            lam = oracle.lefkimmiatis_lambda(R, wq, PC.MIN_SV)
    w = np.concatenate([PC.oracle_run(oracle, case, X, Y, wq, u, n, R, lam)[1].ravel() for u, n in enumerate(case["lens"]) if n])
    assert np.isfinite(w).all() and w.min() >= 1e-4 and w.max() <= 1.0
    for u, n in enumerate(case["lens"]):
        assert not X[u, :, n:].any() and (n == 0 or X[u, :, :n].any())
    return w


@pytest.mark.parametrize("case", PC.ZEL_CASES, **_ID)
def test_zelinski_inputs_have_teeth(oracle, case):
    w = _weights(oracle, case)
    floor, inside, one, near1 = (w == 1e-4).mean(), ((w > 1e-4) & (w < 1.0)).mean(), (w == 1.0).mean(), (np.abs(w - 1.0) < 1e-6).mean()
    print("%s (%s, alpha %g, type %d): weight on the floor %.1f %%, strictly inside %.1f %%, exactly 1 %.1f %%, within 1e-6 of 1 %.1f %%" % (
        case["name"], case["family"], case["alpha"], case["type"], 100 * floor, 100 * inside, 100 * one, 100 * near1))
    if case["family"] == "aligned":
        assert inside >= 0.90
    elif case["family"] == "incoherent":
        assert case["type"] == 1 and floor >= 0.30 and inside > 0.0
    else:
        assert near1 == 1.0


@pytest.mark.parametrize("case", PC.NOISE_CASES, **_ID)
def test_mccowan_inputs_have_teeth(oracle, case):
    w = _weights(oracle, case)
    floor, inside, one = (w == 1e-4).mean(), ((w > 1e-4) & (w < 1.0)).mean(), (w == 1.0).mean()
    print("%s (alpha %g, type %d): weight on the floor %.1f %%, strictly inside %.1f %%, on the upper clamp %.1f %%" % (
        case["name"], case["alpha"], case["type"], 100 * floor, 100 * inside, 100 * one))
    assert case["family"] == "aligned" and inside > 0.0
    if case["kind"] == 1:
        if case["type"] == 2:
            assert one >= 0.05
        else:
            assert floor >= 0.05
    R = PC.coherence(oracle, case)
    iu = np.triu_indices(case["C"], 1)
    clip = np.array([(R[f][iu].real > PC.THRESHOLD) & (R[f][iu].imag <= 0.0) for f in range(PC.F)])
    print("%s: coherence clip taken on %.1f %% of pairs x bins" % (case["name"], 100 * clip.mean()))
    assert clip.any() and not clip.all()
