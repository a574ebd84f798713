"""The cases of tests/srp_cases.py are what tests/test_gpu_srp_kernels.py takes them for -- conditions on the dispatch and on the INPUTS, checked
without a GPU (no kernel is involved):
  * the library's queries (dsr_sph_srp_cell, dsr_doa_srp_cell, dsr_sph_beams_cell: the helpers the launches themselves switch on) return the
    cell every case is named for, and the same cell follows from the formulas stated here: NT = ceil(units / 16); TG 8 | 4 | 2 | 1 (fused) and
    4 | 2 | 1 (linear) by NT; DT 1 | 2 | 4 by dim <= 16 | <= 32; bin_chunk with LDS_ROWS = 128 and the pitch BC + 1 from BC = 4 up;
    KS = ceil(C / 4); LDS = C x 64 x pitch x 8 bytes; the grids have the units they are named for (gridN);
  * every cell has a case: the 12 fused (TG, DT), each TG with an NT that is no multiple of it and with units % 16 != 0, maxOrder 3..8, the linear
    TG 2 and 4 with a ragged NT, every BCT of the multi-beam MFMA kernel and a VALU case with a ragged last channel chunk;
  * every bin-chunk class has a channel count that is no multiple of 4, and its boundaries 7|8, 14|15, 25|26, 64|65 hold for every C in 1..128;
  * every BC class has a frequency range whose length is no multiple of BC and that excludes bins 0 and M/2, and the full range occurs;
  * the batches are ragged as named, and for every SRP case the restatement's energy alone gates exactly the planted silent frames."""
import numpy as np
import pytest

from tests import srp_cases as SC

_ID = dict(ids=lambda c: c["name"])
_PATH = "DSR_SPH_SRP_PATH"


def pitch(BC):
    return BC + 1 if BC >= 4 else BC


def bin_chunk(C):
    for BC in (16, 8, 4, 2):
        if C * pitch(BC) <= SC.LDS_ROWS:
            return BC
    return 1


def lds_bytes(C, BC):
    return C * 64 * pitch(BC) * 8


def tiles(units):
    return -(-units // 16)


def fused_cell(units, dim, C):
    NT = tiles(units)
    return (8 if NT >= 8 else 4 if NT >= 4 else 2 if NT >= 2 else 1, 1 if dim <= 16 else 2 if dim <= 32 else 4, bin_chunk(C), -(-C // 4))


def linear_cell(units, C):
    NT = tiles(units)
    return (4 if NT >= 4 else 2 if NT >= 2 else 1, bin_chunk(C), -(-C // 4))


def beams_cell(NB, C, F):
    rows = NB if NB <= 4 else 8 if NB <= 8 else 16
    if NB <= 4 and rows * F * 16 <= 48 * 1024:
        CC = min(C, 48 * 1024 // (rows * F * 16))
        return (SC.VALU, rows, CC), CC * rows * F * 16
    BCT = min(8, bin_chunk(C))
    return (SC.MFMA, BCT, -(-C // 4)), lds_bytes(C, BCT)


@pytest.mark.parametrize("case", SC.SPH_CASES + SC.FRAME_CASES, **_ID)
def test_sph_case_reaches_the_cell_it_names(dsr, monkeypatch, case):
    s = SC.sph_handle(dsr, case)
    units = SC.units_of(case["grid"])
    nT, nP = s.gridN()
    assert nT * nP == units and (SC.GRIDS[case["grid"]] is None or (nT, nP) == SC.GRIDS[case["grid"]][2:]), (nT, nP)
    want = fused_cell(units, case["maxOrder"] ** 2, case["C"])
    assert want == case["expect"], (case["name"], want)
    monkeypatch.setenv(_PATH, "fused")
    got, lds = s.cell()
    assert got == (0,) + case["expect"], "%s: the fused launch is k_sph_srp<%d, %d> staging %d bins, %d K steps" % ((case["name"],) + got[1:])
    assert lds == lds_bytes(case["C"], want[2]) <= 64 * 1024
    monkeypatch.setenv(_PATH, "folded")
    got, lds = s.cell()
    lin = linear_cell(units, case["C"])
    assert got == (1, lin[0], 0, lin[1], lin[2]) and lds == lds_bytes(case["C"], lin[1])
    if case in SC.SPH_CASES:
        tg, dt = case["name"].split("_")[0][1:].split("d")
        assert (int(tg), int(dt)) == want[:2] and case["name"].split("_")[1] == "c%d" % case["C"] and case["name"].endswith("dim%d" % case["maxOrder"] ** 2)


@pytest.mark.parametrize("case", SC.DOA_CASES, **_ID)
def test_doa_case_reaches_the_cell_it_names(dsr, case):
    d = SC.doa_handle(dsr, case)
    assert d.thetaN() == case["nTheta"]
    want = linear_cell(case["nTheta"], case["C"])
    assert want == case["expect"], (case["name"], want)
    got, lds = d.cell()
    assert got == case["expect"], "%s: the launch is k_doa_srp<%d> staging %d bins, %d K steps" % ((case["name"],) + got)
    assert lds == lds_bytes(case["C"], want[1]) <= 64 * 1024


@pytest.mark.parametrize("row", SC.BEAM_CASES, ids=lambda r: "c%d_nb%d_%s" % r[:3])
def test_beam_case_reaches_the_cell_it_names(dsr, monkeypatch, row):
    Cn, NB, kernel, kind, mo, T, expect = row
    monkeypatch.delenv("DSR_SPH_BEAMS_PATH", raising=False)
    want, lds = beams_cell(NB, Cn, SC.F)
    assert want == expect and ("valu", "mfma")[want[0]] == kernel
    assert dsr.sph_beams_cell(NB, Cn, SC.F) == (expect, lds)
    assert ("valu", "mfma")[dsr.load().dsr_sph_beams_path(NB)] == kernel


def test_every_fused_cell_has_a_case():
    cells = {c["expect"][:2] for c in SC.SPH_CASES}
    assert cells == {(tg, dt) for tg in (8, 4, 2, 1) for dt in (1, 2, 4)}
    for tg, ragged in ((2, {3}), (4, {5}), (8, {14, 21})):
        nts = {tiles(SC.units_of(c["grid"])) for c in SC.SPH_CASES if c["expect"][0] == tg}
        assert nts & ragged and all(nt % tg for nt in nts & ragged), (tg, nts)
    for tg in (8, 4, 2, 1):
        assert any(SC.units_of(c["grid"]) % 16 for c in SC.SPH_CASES if c["expect"][0] == tg), tg
    assert any(SC.units_of(c["grid"]) % 16 == 0 for c in SC.SPH_CASES)                       # and one grid of full tiles
    assert {c["maxOrder"] for c in SC.SPH_CASES} == {3, 4, 5, 6, 7, 8}
    assert {c["maxOrder"] for c in SC.SPH_CASES if c["expect"][1] == 4} == {6, 7, 8}          # DT 4: third tile partial / fourth partial / full
    assert {c["kind"] for c in SC.SPH_CASES} == {"EB", "DS"}
    assert max(c["C"] * SC.units_of(c["grid"]) for c in SC.SPH_CASES) == 128 * 210
    # k_sph_frame: ranks beyond the units (1-unit grid) and 5 ranks of 15 units
    assert [(c["nBest"], SC.units_of(c["grid"])) for c in SC.FRAME_CASES] == [(3, 1), (5, 15)]


def test_linear_and_beam_cells_have_cases():
    assert {c["C"] for c in SC.DOA_CASES} == {5, 13, 25, 27, 66, 128}
    by = {}
    for c in SC.DOA_CASES:
        by.setdefault(c["expect"][0], set()).add(tiles(c["nTheta"]))
    assert by == {2: {2, 3}, 4: {7}}                                                         # TG 2 with NT 3, TG 4 with NT 7: ragged
    assert {c["nTheta"] for c in SC.DOA_CASES} == {17, 40, 100} and all(c["nTheta"] % 16 for c in SC.DOA_CASES)
    assert {c["expect"][2] for c in SC.DOA_CASES} >= {2, 4, 7, 17, 32}                        # KS 7 = 4 + 2 + 1, KS 17 = 4 x 4 + 1
    mfma = [r for r in SC.BEAM_CASES if r[2] == "mfma"]
    assert {r[6][1] for r in mfma} == {4, 1} and {r[1] for r in mfma} >= {5, 16} and {r[0] for r in mfma} >= {66, 128}
    assert {r[0] for r in mfma if r[6][1] == 4} & {16, 25}
    assert all(r[5] % 16 for r in SC.BEAM_CASES if r[5] < 64) and any(r[5] < 64 for r in SC.BEAM_CASES)
    valu = [r for r in SC.BEAM_CASES if r[2] == "valu"]
    assert [(r[0], r[1]) for r in valu] == [(66, 4)] and valu[0][0] % valu[0][6][2] and valu[0][0] > 2 * valu[0][6][2]   # chunks 23, 23, 20
    # with tests/sph2_cases.py (BCT 8 and 2) every instantiation of k_sph_beams_mfma has a case
    from tests.sph2_cases import BEAM_SHAPES
    assert {min(8, bin_chunk(r[0])) for r in BEAM_SHAPES if r[2] == "mfma"} | {r[6][1] for r in mfma} == {8, 4, 2, 1}
    assert {(k, c, mo * mo) for k, c, mo in SC.APPLY_CASES} >= {("DS", 13, 25), ("EB", 66, 49)} and {c for _, c, _ in SC.APPLY_CASES} == {13, 66}
    assert {mo * mo for _, _, mo in SC.APPLY_CASES} == {25, 49}


def test_every_bin_chunk_class_has_a_ragged_channel_count(dsr):
    """C 5 (BC 16, KS 2), 13 (8, 4), 25 (4, 7), 27 (2, 7), 66 (1, 17), 128 (1, LDS 65 536); the class boundaries for every C through the query"""
    want = {5: (16, 2), 13: (8, 4), 25: (4, 7), 27: (2, 7), 66: (1, 17), 128: (1, 32)}
    for cases in (SC.SPH_CASES, SC.DOA_CASES):
        seen = {c["C"]: c["expect"][-2:] for c in cases}
        for C, cell in want.items():
            assert seen[C] == cell, (C, seen[C])
        for BC in (16, 8, 4, 2, 1):
            assert any(c["expect"][-2] == BC and c["C"] % 4 for c in cases), BC
    assert lds_bytes(128, 1) == 65536 == max(lds_bytes(C, bin_chunk(C)) for C in range(1, 129))
    got = {}
    for C in range(1, 129):
        d = dsr.DoaSRP(1, SC.FS, SC.M, C); d.setArrayGeometry(SC.doa_positions(C)); d.setSearchParam(0.0, np.pi, np.pi / 17)
        cell, lds = d.cell()
        assert cell == linear_cell(17, C) and lds == lds_bytes(C, cell[1]) <= 64 * 1024, C
        assert dsr.sph_beams_cell(5, C, SC.F) == ((SC.MFMA, min(8, cell[1]), cell[2]), lds_bytes(C, min(8, cell[1]))), C
        got[C] = cell[1]
    for lo, hi, a, b in ((7, 8, 16, 8), (14, 15, 8, 4), (25, 26, 4, 2), (64, 65, 2, 1)):
        assert (got[lo], got[hi]) == (a, b), (lo, hi)
    assert [got[C] for C in range(1, 129)] == sorted(got.values(), reverse=True) and got[1] == 16 and got[128] == 1
    for C in (0, 129):
        with pytest.raises(dsr.DsrError):
            dsr.sph_beams_cell(5, C, SC.F)
    with pytest.raises(dsr.DsrError):
        dsr.sph_beams_cell(17, 8, SC.F)


def test_frequency_ranges():
    for cases in (SC.SPH_CASES, SC.DOA_CASES):
        for BC in (16, 8, 4, 2, 1):
            rs = [c["rng"] for c in cases if c["expect"][-2] == BC]
            assert any(a > 0 and b < SC.M // 2 and (BC == 1 or (b - a + 1) % BC) for a, b in rs), (BC, rs)   # (every length is a multiple of 1)
        assert any(c["rng"] == (0, SC.M // 2) for c in cases)
    assert all(0 <= a <= b <= SC.M // 2 for c in SC.SPH_CASES + SC.FRAME_CASES + SC.DOA_CASES for a, b in [c["rng"]])


def test_batches_are_ragged_as_named():
    assert (SC.M, SC.T, SC.U) == (64, 70, 3) and len(SC.NFRAMES) == SC.U
    full, short, one = SC.NFRAMES
    assert full == SC.T and 64 < SC.T < 128 and SC.T % 16 and 1 < short < 64 and one == 1      # two frame tiles, the second partial; an early exit; one frame
    p, l = SC.planted(), SC.live()
    assert p.sum() == 16 and not (p & ~l).any() and p[0].any() and p[1].any() and not p[2].any()


@pytest.mark.parametrize("case", SC.SPH_CASES + SC.FRAME_CASES + SC.DOA_CASES, **_ID)
def test_restatement_gates_exactly_the_planted_frames(case):
    X = SC.snapshots(case)
    assert X.shape == (SC.U, case["C"], SC.T, SC.F) and X.dtype == np.complex64
    thr, e = SC.gate_threshold(X, *case["rng"])
    p, l = SC.planted(), SC.live()
    gated = (e < np.float32(thr)) & l
    assert np.array_equal(gated, p), (case["name"], int(gated.sum()))
    assert e[p].max() * 100 < e[l & ~p].min()                                               # the threshold sits in a wide gap
