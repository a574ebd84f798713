"""CPU tests of the adaptive subband beamformers' test inputs (tests/abf_cases.py) and restatement (tests/abf_np.py); no kernel is involved.

  * the dispatch query dsr_abf_path returns the cell each case names, the same cell follows from the rules DESIGN 4.4t states
    (abf_cases.cell_formula), and every cell and every reachable side of a gate has a case;
  * every Griffiths-Jim case takes and leaves each of its three decisions (gate, norm constraint, floor) at least 5 times, and no compared value
    lies within 1e-6 (relative) of its threshold -- so a device that rounds differently decides the same;
  * the matrix every sample-matrix case factorises is Hermitian positive definite at every adapted frame;
  * the host helpers equal the restatement to 1e-13 and B^H conj(vs) = 0 to 1e-12;
  * the two evaluations of each case differ by the yardstick the GPU test's tolerance is built from (printed with -s), and the device's
    formulation (fp64 Cholesky; MPDR with R and L averaged directly), evaluated in numpy, stays inside that tolerance;
  * argument errors."""
import numpy as np
import pytest

from tests import abf_cases as AC
from tests import abf_np as A
from tests import synth

_ID = dict(ids=lambda c: c["name"])
ALL = AC.CASES + AC.CROSS_CASES


def _set_env(monkeypatch, env):
    for k in AC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def abf(dsr):
    from dsr import _abf
    return _abf


@pytest.mark.parametrize("case", ALL, **_ID)
def test_query_returns_the_cell_the_case_names(abf, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    path, lds = abf.abf_path(case["kind"], case["C"])
    assert path == case["expect"] == AC.cell_formula(case["kind"], case["C"], case["env"])
    sN, fN = AC.state_entries(case["kind"], case["C"])
    assert lds[0] == (sN + fN) * 16 * 64
    assert lds[1] == {AC.REGS: fN * 16 * 64, AC.LDS: lds[0], AC.MEM: 0}[path[2]] and lds[1] <= 160 * 1024
    if "lds" in case["gates"]:
        assert case["gates"]["lds"] == (lds[0] <= AC.LDS_GATE) and case["gates"]["cap16"] == (case["C"] <= 16)
        assert not case["env"]                                                  # a gate case sits on its side without a switch


def test_every_cell_and_every_gate_side_has_a_case():
    envs = ({}, AC.NOREGS, AC.BOTH, AC.MEMSTATE)
    have = {(c["kind"], c["expect"]) for c in AC.CASES}
    for kind in ("gj", "mvdr", "mpdr"):
        cells = {AC.cell_formula(kind, C, e) for C in range(2, 65) for e in envs}
        assert cells == {e for k, e in have if k == kind}, (kind, sorted(cells - {e for k, e in have if k == kind}))
        gate = {(c["C"], c["gates"]["lds"]) for c in AC.CASES if c["kind"] == kind and "lds" in c["gates"]}
        fits = [C for C in range(2, 65) if sum(AC.state_entries(kind, C)) * 1024 <= AC.LDS_GATE]
        assert (max(fits), True) in gate or max(fits) == 64 and (64, True) in gate      # the last channel count inside the gate
        if max(fits) < 64:
            assert (max(fits) + 1, False) in gate                                # and the first one past it
        else:
            assert kind == "gj"                                                 # n + 1 entries: every supported C fits, memory only by the switch
        caps = {c["C"] for c in AC.CASES if c["kind"] == kind}
        assert {2, 16, 17, 64} <= caps                                          # order-1 matrix, both sides of the capacity gate, the largest C
    for kind in ("mvdr", "mpdr"):
        ends = {c["params"]["end"] for c in AC.CASES if c["kind"] == kind}
        assert 0 in ends and 20 in ends and any(e >= 40 for e in ends)
        assert any(c["scale"] == 1.0e3 for c in AC.CASES if c["kind"] == kind)
    assert any(c["wp"] for c in AC.CASES if c["kind"] == "mvdr") and any(not c["wp"] for c in AC.CASES if c["kind"] == "mvdr")
    for c in AC.CASES:
        if c["kind"] == "gj":
            assert 0 < c["params"]["staticAfter"] < c["T"] and c["wp"] < c["T"]
        if c["kind"] == "mvdr" and c["wp"]:
            assert c["wp"] >= c["T"]
    assert any(c["wp"] for c in AC.CASES if c["kind"] == "gj")


@pytest.mark.parametrize("case", [c for c in ALL if c["kind"] == "gj"], **_ID)
def test_griffiths_jim_cases_take_and_leave_every_decision(case):
    r = AC.reference(case)
    for k in ("gate", "norm", "floor"):
        taken = sum(ref["counts"][k][0] for ref, _ in r["runs"]); idle = sum(ref["counts"][k][1] for ref, _ in r["runs"])
        margin = min(ref["margins"][k] for ref, _ in r["runs"])
        print("%s %s: taken %d, idle %d, smallest relative distance from the threshold %.2e" % (case["name"], k, taken, idle, margin))
        assert taken >= 5 and idle >= 5, (case["name"], k, taken, idle)
        assert margin > 1.0e-6, (case["name"], k, margin)
        assert [sum(a["counts"][k][i] for _, a in r["runs"]) for i in (0, 1)] == [taken, idle]      # the second evaluation decides the same


@pytest.mark.parametrize("case", [c for c in ALL if c["kind"] != "gj"], **_ID)
def test_sample_matrices_are_hermitian_positive_definite(case):
    r = AC.reference(case)
    stats = [ref["stat"] for (ref, _), n in zip(r["runs"], AC.lens_of(case)) if n]
    print("%s: smallest eigenvalue %.3e, condition number up to %.2e" % (case["name"], min(s["min_eig"] for s in stats), max(s["cond"] for s in stats)))
    assert min(s["min_eig"] for s in stats) >= 0.5 * case["params"]["diagLoad"]
    assert max(s["herm"] for s in stats) <= 1.0e-14


@pytest.mark.parametrize("case", ALL, **_ID)
def test_the_two_evaluations_differ_by_the_yardstick(case):
    r = AC.reference(case)
    print("%s: yardstick %.2e of the output RMS (%.3g), %.2e of the weight RMS (%.3g)" % (case["name"], r["yard_y"], r["rms_y"], r["yard_w"], r["rms_w"]))
    assert np.isfinite(r["yard_y"]) and np.isfinite(r["yard_w"]) and r["rms_y"] > 0 and r["rms_w"] > 0
    if case["kind"] == "gj":
        return
    # the device's formulation, in numpy: inside the GPU test's tolerance (8 x the yardstick, floored at 1e-14)
    ey = ew = 0.0
    for u, n in enumerate(AC.lens_of(case)):
        if n:
            Xu, p = r["X"][u][:, :n], case["params"]
            d = A.mvdr_device_order(Xu, r["wq"], **p) if case["kind"] == "mvdr" else A.smi_mpdr(Xu, r["wq"], r["B"], form="rl", **p)
            Y = d["Y"]
            if r["wp"] is not None:
                Y = Y * r["wp"][u][:n].astype(np.float64)
            ey = max(ey, np.abs(Y - r["runs"][u][0]["Y"]).max()); ew = max(ew, np.abs(d["w"] - r["runs"][u][0]["w"]).max())
    ty, tw = 8 * max(r["yard_y"], 1e-14) * r["rms_y"], 8 * max(r["yard_w"], 1e-14) * r["rms_w"]
    print("%s: Cholesky formulation at %.2f of the output tolerance, %.2f of the weight tolerance" % (case["name"], ey / ty, ew / tw))
    assert ey <= ty and ew <= tw


@pytest.mark.parametrize("C", [2, 3, 4, 8, 13, 64])
def test_host_helpers_equal_the_restatement(abf, C):
    delays, wq, B = AC.design(C)
    d2 = A.calcDelays(-300.0, 1200.0, 100.0, synth.linear_array(C, 25.0))
    for f in (0, 1, 7, AC.M // 2, AC.M // 2 + 1, AC.M - 1):
        for norm in (True, False):
            v = A.calcArrayManifold_f(f, AC.M, C, 16000.0, delays, norm=norm)
            assert np.abs(abf.manifold(f, AC.M, C, 16000.0, delays, False, norm) - v).max() <= 1e-13
    for f in (0, 1, 7, AC.M // 2):
        Bd = abf.blocking_matrix(wq[f], 1)
        assert Bd.shape == (C, C - 1) and np.abs(Bd - B[f]).max() <= 1e-13
        assert np.abs(Bd.conj().T @ np.conj(wq[f])).max() <= 1e-12 if C > 1 else True
        assert np.abs(Bd.conj().T @ Bd - np.eye(C - 1)).max() <= 1e-12
        if C >= 3:
            w1 = A.calcArrayManifold_f(f, AC.M, C, 16000.0, delays, norm=False); w2 = A.calcArrayManifold_f(f, AC.M, C, 16000.0, d2, norm=False)
            wn = A.calcNullBeamformer(w1, w2, 2)
            assert np.abs(abf.null_beamformer(w1, w2, 2) - wn).max() <= 1e-13 * max(1.0, np.abs(wn).max())
            B2 = abf.blocking_matrix(wn, 2)
            assert B2.shape == (C, C - 2) and np.abs(B2 - A.calcBlockingMatrix(wn, 2)).max() <= 1e-13
    from dsr.btk import subbandBeamforming as SB
    assert np.abs(SB.calcDelays(800.0, 1500.0, 300.0, synth.linear_array(C, 25.0)) - delays).max() <= 1e-18


def test_argument_errors(dsr, abf):
    for kind in ("ds", "gj", "mvdr", "mpdr"):
        with pytest.raises(dsr.DsrError) as e:
            abf.AdaptiveBeamformer(kind, 32, 4, NC=2)
        assert e.value.status == dsr.E_CONSISTENCY
        with pytest.raises(dsr.DsrError) as e:
            abf.AdaptiveBeamformer(kind, 32, 4, halfBandShift=True)
        assert e.value.status == dsr.E_CONSISTENCY
    g = abf.AdaptiveBeamformer("gsc", 32, 4, NC=2)                               # two constraints: the static GSC only
    assert (g.C, g.NC, g.outN) == (4, 2, 3)
    with pytest.raises(dsr.DsrError) as e:
        abf.AdaptiveBeamformer("gsc", 32, 4, NC=3)
    assert e.value.status == dsr.E_CONSISTENCY
    for kind in ("mvdr", "mpdr"):
        for dl in (0.0, -1.0e-3):
            with pytest.raises(dsr.DsrError) as e:
                abf.AdaptiveBeamformer(kind, 32, 4, diagLoad=dl)
            assert e.value.status == dsr.E_PARAMETER
    with pytest.raises(dsr.DsrError) as e:
        abf.AdaptiveBeamformer("gj", 32, 65)
    assert e.value.status == dsr.E_DIMENSION
    with pytest.raises(dsr.DsrError) as e:
        abf.manifold(3, 32, 4, 16000.0, np.zeros(4), True)
    assert e.value.status == dsr.E_CONSISTENCY
    with pytest.raises(dsr.DsrError) as e:
        abf.null_beamformer(np.ones(4), np.ones(4), 1)
    assert e.value.status == dsr.E_CONSISTENCY
    with pytest.raises(dsr.DsrError) as e:
        abf.abf_path("gsc", 4)                                                  # the fixed-weight kinds have no dispatch
    assert e.value.status == dsr.E_PARAMETER
    assert dsr.AdaptiveBeamformer is abf.AdaptiveBeamformer                      # the binding's name


def test_facade_refuses_what_the_library_refuses(dsr):
    from dsr.btk import subbandBeamforming as SB
    X = np.zeros((4, 12, 17), np.complex64)
    for cls in (SB.SubbandBeamformerMVDR, SB.SubbandBeamformerMPDR):
        with pytest.raises(dsr.DsrError) as e:
            cls(X)                                                              # the reference's default halfBandShift=True
        assert e.value.status == dsr.E_CONSISTENCY
        with pytest.raises(dsr.DsrError) as e:
            cls(X, diagLoad=0.0, halfBandShift=False)
        assert e.value.status == dsr.E_PARAMETER
    with pytest.raises(dsr.DsrError) as e:
        SB.SubbandBeamformerGriffithsJim(X, halfBandShift=True)
    assert e.value.status == dsr.E_CONSISTENCY
    with pytest.raises(dsr.DsrError) as e:
        SB.SubbandBeamformerGSC(X, NC=3)
    assert e.value.status == dsr.E_CONSISTENCY
    # a wp1L shorter than the utterance: refused before anything is computed
    bf = SB.SubbandBeamformerMVDR(X, halfBandShift=False, wp1L=[np.ones(17)] * 11)
    bf.calcArrayManifoldVectors(16000.0, np.linspace(0.0, 1.0e-4, 4))
    with pytest.raises(dsr.DsrError) as e:
        next(iter(bf))
    assert e.value.status == dsr.E_CONSISTENCY and "wp1L" in str(e.value)
