"""CPU tests of the multichannel cross-correlation localiser: the numpy restatement (tests/mcc_np.py) against independent forms, the
properties of the two search grids, the host side of the C-ABI (include/dsr.h section 2f) without a GPU, and the conditions on the inputs
that tests/test_gpu_mcc.py relies on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mcc_cases as K
from tests import mcc_np as M
from tests.conftest import PKG

LIB = os.path.join(PKG, "lib", "libdsr_hip.so")


def _case_id(i):
    c = K.CASES[i]
    return "%s-C%d-L%s-S%d" % (c["kind"], c["C"], c["L"] or "2D", c["S"])


ALL = pytest.mark.parametrize("i", range(len(K.CASES)), ids=_case_id)
_memo = {}


def _setup(i):
    if i not in _memo:
        case = K.CASES[i]; g = K.np_grid(case); pos, dl, tau = g.enumerate(); D = g.D()
        b = K.build(case, tau, D)
        _memo[i] = (case, g, pos, dl, tau, D, b, K.reference(case, b, tau, D))
    return _memo[i]


# ---- the restatement against independent forms ------------------------------------------------------------------------------------------------
def test_covariance_against_a_double_loop():
    rng = np.random.default_rng(3); Cn, L, D = 3, 12, 4
    x = rng.standard_normal((Cn, L)).astype(np.float32); tau = np.array([0, -3, 4])
    R = np.zeros((Cn, Cn))
    for n in range(L - D):
        v = []
        for c in range(Cn):
            y = n + tau[c]
            v.append(float(x[c, y]) if y >= 0 else float(x[c, L + y]))          # the holder has the last D samples of this block
        for i in range(Cn):
            for j in range(i + 1):
                R[i, j] += v[i] * v[j]
    R /= (L - D)
    got = M.covariance(x, tau, D)
    assert np.abs(got - R).max() < 1e-14 and not np.triu(got, 1).any()
    with pytest.raises(ValueError):
        M.covariance(x[:, :7], tau, D)


def test_cost_against_slogdet_and_hadamard():
    rng = np.random.default_rng(4)
    for Cn in (2, 5, 16):
        x = rng.standard_normal((Cn, 400)).astype(np.float32); x[1] += 0.8 * x[0]
        R = M.covariance(x, np.zeros(Cn, int), 5); Rs = np.tril(R) + np.tril(R, -1).T
        c, ev = M.cost_of(R); sign, ld = np.linalg.slogdet(Rs)
        assert sign > 0 and abs(c - (ld - np.log(np.diag(Rs)).sum())) < 1e-11
        assert c <= 0.0                                                          # Hadamard: det R <= prod R_ii
        c2, _ = M.cost_of(R, normalizeVariance=False)
        assert abs(c2 - ld) < 1e-11
    assert M.cost_of(np.zeros((3, 3)))[0] == 0.0                                 # an exactly zero eigenvalue
    with np.errstate(invalid="ignore"):
        c, ev = M.cost_of(np.diag([1.0, -2.0]))                                      # a negative one is negated (the diagonal's log is then nan there too)
    assert ev.tolist() == [2.0, 1.0]


def test_two_channels_give_the_squared_normalised_cross_correlation():
    rng = np.random.default_rng(5); L, D = 300, 6
    s = rng.standard_normal(L + 20); x = np.stack([s[10:10 + L], s[7:7 + L] + 0.5 * rng.standard_normal(L)]).astype(np.float32)
    for lag in (-3, 0, 3, 5):
        tau = np.array([0, lag]); R = M.covariance(x, tau, D); c, _ = M.cost_of(R)
        n = np.arange(L - D); a = x[0, n].astype(np.float64); bb = x[1, (n + lag) % L].astype(np.float64)
        rho2 = (a @ bb) ** 2 / ((a @ a) * (bb @ bb))
        assert abs((1.0 - np.exp(c)) - rho2) < 1e-12


def test_nbest_insertion_keeps_the_earlier_grid_point():
    assert M.nbest([-1.0, -3.0, -3.0, -2.0, -3.0], 3) == [(-3.0, 1), (-3.0, 2), (-3.0, 4)]
    assert M.nbest([-1.0], 2) == [(-1.0, 0), (100000.0, -1)]
    assert M.nbest([0.0, 0.0, 0.0], 2) == [(0.0, 0), (0.0, 1)]


@ALL
def test_planted_direction_is_found(i):
    case, g, pos, dl, tau, D, b, ref = _setup(i)
    for (u, k), r in ref.items():
        p = b["planted"][u, k]
        if p < 0:
            assert not r["costs"].any() and [x[1] for x in r["best"]] == list(range(case["S"]))     # the all-zero block: the first grid points
            continue
        best = r["best"][0][1]
        assert np.array_equal(tau[best], tau[p]), (u, k, best, p)
        assert np.all(r["costs"] <= 0.0)


# ---- grid properties ------------------------------------------------------------------------------------------------------------------------
@ALL
def test_grid_properties(i):
    case, g, pos, dl, tau, D, b, ref = _setup(i)
    G = pos.shape[0]
    assert not pos[0].any() and 2 <= G < 65536                                   # the first candidate is the origin; the walk ends
    assert np.abs(tau).max() <= D and D >= 4
    if case["kind"] == "linear":
        az = pos[:, 1]; first = az < 3 * np.pi / 2
        s1 = np.sin(az[first].astype(np.float32)).astype(np.float64); s2 = np.sin(az[~first].astype(np.float32)).astype(np.float64)
        assert np.all(np.diff(s1) > 0) and np.all(np.diff(s2) > 0) and s1[-1] == 1.0 and s2[0] == -1.0 and s2[-1] < 0
        for s in (s1[:-1], s2):                                                  # equal steps in sin(azimuth) (the last step of the first half is cut at 1)
            assert np.abs(np.diff(s) - float(g.constV)).max() < 1e-6
        assert np.all(tau[first] <= 0) and np.all(tau[~first] >= 0)
    else:
        assert np.all(np.diff(pos[:, 1]) >= 0) and pos[:, 1].max() < 2 * np.pi and pos[:, 2].min() >= 0 and pos[:, 2].max() < np.pi
        assert len(np.unique(pos[:, 1])) >= 2                                    # polar angle first, then azimuth


# ---- the host side of the C-ABI, no GPU needed ------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_classes_import(dsr):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = set(re.findall(r" T (dsr_[a-z0-9_]+)", out))
    protos = dsr.header_prototypes()
    mine = {n for n in protos if n.startswith(("dsr_sgb_", "dsr_mcc_", "dsr_mcccalc_"))}
    need = {"dsr_sgb_create", "dsr_sgb_set_distance", "dsr_sgb_set_positions", "dsr_sgb_set_radius", "dsr_sgb_reset", "dsr_sgb_next", "dsr_sgb_position",
            "dsr_sgb_time_delays", "dsr_sgb_max_time_delay", "dsr_sgb_enumerate", "dsr_mcc_create", "dsr_mcc_run", "dsr_mcc_calc", "dsr_mcc_channel_delays",
            "dsr_mcc_destroy", "dsr_sgb_destroy", "dsr_mcc_stream_create", "dsr_mcccalc_stream_create"}
    assert need <= mine and mine <= exported, sorted(mine - exported)
    from dsr.btk.localization import SearchGridBuilderPtr, SGB4LinearArrayPtr, SGB4CircularArrayPtr, MCCLocalizerPtr, MCCCalculatorPtr  # noqa: F401
    assert dsr.SearchGrid and dsr.MccLocalizer and dsr.MccCalculator


@ALL
def test_enumerate_matches_the_restatement(dsr, i):
    case, g, pos, dl, tau, D, b, ref = _setup(i)
    sg = K.configure(dsr.SearchGrid(case["kind"], case["C"], True, K.FS), case)
    assert abs(sg.maxTimeDelay() - float(g.maxTimeDelay)) == 0.0 and np.abs(sg.microphonePositions() - g.mpos).max() <= 1e-4
    p2, d2, t2 = sg.enumerate()
    assert p2.shape == pos.shape, (p2.shape, pos.shape)
    assert np.abs(p2 - pos).max() <= 1e-6
    frac = np.abs(K.FS * dl - np.round(K.FS * dl)); safe = frac > 1e-4           # elsewhere sinf of two libraries may differ in the last bit
    safe |= np.abs(K.FS * dl) < 0.5                                              # truncation toward zero: everything near 0 gives 0
    assert np.array_equal(t2[safe], tau[safe])
    assert (~safe).mean() <= 0.02, (~safe).mean()
    # the step-by-step walk gives the same points as enumerate()
    sg.reset(); n = 1
    assert not sg.getSearchPosition().any()
    while sg.nextSearchGrid():
        assert np.array_equal(sg.getSearchPosition(), p2[n]) and np.array_equal(sg.getTimeDelays(), d2[n]); n += 1
    assert n == p2.shape[0]
    dsr.mcc_check(sg, case["S"], b["L"])


def test_refusals(dsr):
    sg = dsr.SearchGrid("linear", 4, True, K.FS)
    with pytest.raises(dsr.DsrError) as e:                                       # no geometry: the reference casts maxTimeDelay = -1 to size_t
        dsr.mcc_check(sg, 1, 0)
    assert e.value.status == 7
    with pytest.raises(dsr.DsrError) as e:
        sg.enumerate()
    assert e.value.status == 7
    with pytest.raises(dsr.DsrError) as e:
        sg.setRadius(100.0)
    assert e.value.status == 13
    sg.setDistanceBtwMicrophones(50.0)
    dsr.mcc_check(sg, 1, 12)
    with pytest.raises(dsr.DsrError) as e:                                       # D = 6: 11 samples are fewer than 2 D
        dsr.mcc_check(sg, 1, 11)
    assert e.value.status == 1 and "Data samples are insufficient" in str(e.value)
    with pytest.raises(dsr.DsrError) as e:
        dsr.mcc_check(sg, 0, 0)
    assert e.value.status == 5
    nf = dsr.SearchGrid("circular", 8, False, K.FS); nf.setRadius(100.0)
    with pytest.raises(dsr.DsrError) as e:                                       # the near-field grid: "need to be implemented"
        nf.enumerate()
    assert e.value.status == 7 and "need to be implemented" in str(e.value)
    with pytest.raises(dsr.DsrError) as e:
        dsr.mcc_check(nf, 1, 0)
    assert e.value.status == 7
    assert nf.nextSearchGrid() is False
    big = dsr.SearchGrid("linear", 65, True, K.FS); big.setDistanceBtwMicrophones(10.0)
    with pytest.raises(dsr.DsrError) as e:
        dsr.mcc_check(big, 1, 0)
    assert e.value.status == 5
    with pytest.raises(dsr.DsrError) as e:
        sg.setPositionsOfMicrophones(np.zeros((3, 3)))
    assert e.value.status == 5


def test_localizer_needs_a_device(dsr):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    sg = dsr.SearchGrid("linear", 4, True, K.FS); sg.setDistanceBtwMicrophones(50.0)
    with pytest.raises(dsr.DsrError) as e:
        dsr.MccLocalizer(sg, 1)
    assert e.value.status == 7
    from dsr.btk.localization import SGB4LinearArrayPtr, MCCLocalizerPtr
    s2 = SGB4LinearArrayPtr(4, True); s2.setDistanceBtwMicrophones(50.0)
    with pytest.raises(dsr.DsrError) as e:
        MCCLocalizerPtr(s2)
    assert e.value.status == 7


# ---- what the GPU test relies on ---------------------------------------------------------------------------------------------------------------
@ALL
def test_inputs_satisfy_the_gpu_tests_conditions(i):
    case, g, pos, dl, tau, D, b, ref = _setup(i)
    v = K.valid_blocks(case, b)
    assert v[0].all() and not v[1:, -1].any() and v[:, :-1].all()                # ragged: the later utterances lose their last block
    items = left = 0
    for (u, k), r in ref.items():
        if (u, k) == b["zero"]:
            continue
        assert r["kappa"].max() <= K.KAPPA_MAX, (u, k, r["kappa"].max())
        items += 1
        srt = np.sort(r["costs"]); distinct = srt[srt > srt[0]]
        tol = K.tolerance(case["C"], r["kappa"].max())
        if distinct.size and distinct[0] - srt[0] < 2 * tol:
            left += 1
        if not all(K.comparable_entries(r, tau, case["C"])):
            left += 1
    assert items > 0 and left <= 0.02 * items, (items, left)


def test_cpp_classes_walk_the_grid_and_map_refusals(tmp_path):
    """host/dsr_streams.hpp: SGB4LinearArray, SGB4CircularArray, MCCLocalizer and MCCCalculator under plain g++ -std=c++11 -- the walk gives the
    restatement's number of grid points, and the constructors' refusals arrive as the reference's exception types."""
    src = tmp_path / "m.cpp"
    src.write_text(r"""
#include "dsr_streams.hpp"
#include <cstdio>
int main() {
  SGB4LinearArray* lin = new SGB4LinearArray(4, true); lin->setDistanceBtwMicrophones(50.0f); SearchGridBuilderPtr l(lin);
  int n = 1; while (l->nextSearchGrid()) n++;
  printf("linear %d %d %g\n", n, (int) l->chanN(), l->getSearchPosition()[1] > 4.7 ? 1.0 : 0.0);
  SGB4CircularArray* cir = new SGB4CircularArray(8, true); cir->setRadius(100.0f); SearchGridBuilderPtr c(cir);
  n = 1; while (c->nextSearchGrid()) n++;
  c->reset(); printf("circular %d %g\n", n, c->getTimeDelays()[0]);
  try { SearchGridBuilderPtr bare(new SGB4LinearArray(4, true)); MCCLocalizerPtr m(new MCCLocalizer(bare)); printf("no refusal\n"); }
  catch (jinitialization_error& e) { printf("bare %d\n", (int) e.getCode()); }
  try { SGB4CircularArray* nf = new SGB4CircularArray(8, false); nf->setRadius(100.0f); SearchGridBuilderPtr f(nf); MCCCalculatorPtr m(new MCCCalculator(f)); printf("no refusal\n"); }
  catch (jinitialization_error& e) { printf("nearfield %d\n", (int) e.getCode()); }
  try { MCCLocalizerPtr m(new MCCLocalizer(l, 2)); MCCCalculatorPtr k(new MCCCalculator(c, false)); printf("made %u %s\n", m->size(), k->name().c_str()); }
  catch (jinitialization_error& e) { printf("nodevice %d\n", (int) e.getCode()); }
  return 0;
}
""")
    exe = tmp_path / "m"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    gl = M.Grid("linear", 4, K.FS); gl.setDistanceBtwMicrophones(50.0); gc = M.Grid("circular", 8, K.FS); gc.setRadius(100.0)
    assert lines[0] == "linear %d 4 1" % gl.enumerate()[0].shape[0]
    assert lines[1] == "circular %d 0" % gc.enumerate()[0].shape[0] or lines[1] == "circular %d -0" % gc.enumerate()[0].shape[0]
    assert lines[2] == "bare 6" and lines[3] == "nearfield 6"
    assert lines[4] in ("nodevice 6", "made 3 MCCCalculator")                    # without a GPU the plan is refused (JINITIALIZATION)
