"""The fp64-MFMA steered-response-power kernels and the multi-beam apply in every cell their dispatches can select, on the cases of
tests/srp_cases.py (tests/test_srp_cases_cpu.py shows without a GPU that the cases are what they are named for).  fftLen 64, 70 frames (two
64-frame workgroup tiles, the second partial), three utterances: full, one that ends inside the first tile, one frame.

Every case first asserts its cell through the library's query (dsr_sph_srp_cell, dsr_doa_srp_cell, dsr_sph_beams_cell), which the launch itself
switches on.  What is compared, under the project's standing bounds:
  * k_sph_srp<TG, DT> (DSR_SPH_SRP_PATH=fused) and, on the same case, the folded table through k_doa_srp<TG> (folded), each with tests/sph_np.py
    in complex128 on the handle's own tables, as tests/test_gpu_sph.py::_run_case does: energy bit for bit, the gate equal, rp and acc within 1e-12
    of the frame's / the utterance's largest value, the N-best by _check_nbest, the last unit's y within 2e-7 of the frame maximum, sentinels
    untouched past nframes (and in y outside the frequency range); the two paths' energy and gate equal;
  * k_doa_srp<TG> with tests/doa_srp_np.py under the assertions of tests/test_gpu_doa.py::test_srp_matches_restatement;
  * k_sph_beams_mfma<4 | 1> and the VALU kernel over several channel chunks with tests/sph2_np.py under _check of tests/test_gpu_sph2.py;
  * k_sph_apply at dim 25 and 49 under the bounds of tests/test_gpu_sph.py::test_apply_matches_restatement;
  * k_sph_frame with more ranks than units: the ranks beyond the units are (-10e10, -1) on ungated frames, the others copies of rp.

Template instance -> the case that launches it (tests/srp_cases.py):
  k_sph_srp<1, 1 | 2 | 4>   [t1d1_c5_dim9] [t1d2_c13_dim25] [t1d4_c25_dim36], the two frame cases
  k_sph_srp<2, 1 | 2 | 4>   [t2d1_c27_dim16] [t2d2_c66_dim25] (NT 3) [t2d4_c128_dim49] (LDS 65 536)
  k_sph_srp<4, 1 | 2 | 4>   [t4d1_c32_dim9] (NT 5) [t4d2_c5_dim25] [t4d4_c13_dim64] (NT 5)
  k_sph_srp<8, 1 | 2 | 4>   [t8d1_c25_dim16] [t8d2_c27_dim25] [t8d4_c66_dim36] [t8d4_c128_dim49] (NT 14)
  k_doa_srp<1>              the folded runs of the 15-unit and 1-unit cases
  k_doa_srp<2>              [c5_n40] [c27_n40] (NT 3) [c13_n17] [c128_n17], the folded runs of the 18-, 32- and 40-unit cases
  k_doa_srp<4>              [c25_n100] [c66_n100] [c128_n100] (NT 7), the folded runs from 50 units up
  k_sph_beams_mfma<4>       [c25_nb5] [c16_nb16];  k_sph_beams_mfma<1>  [c66_nb16] [c128_nb5]  (<8> and <2>: tests/test_gpu_sph2.py)
  k_sph_beams_valu<4, 4>    [c66_nb4]: channel chunks of 23, 23, 20
Run with -s for the measured error of every case; the closing test prints the largest seen per quantity (recorded in DESIGN.md)."""
import ctypes as C

import numpy as np
import pytest

from tests import doa_srp_np as D
from tests import sph2_np as S2
from tests import sph_np as S
from tests import srp_cases as SC
from tests.sph2_cases import beam_dirs, geom_of, handle
from tests.test_gpu_doa import _check_nbest, _snapshots

pytestmark = pytest.mark.gpu

_ID = dict(ids=lambda c: c["name"])
_REF = {}                                                                      # case -> snapshots, tables and the restatement's run, computed once
WORST = {"sph rp": 0.0, "sph acc": 0.0, "sph y": 0.0, "doa rp": 0.0, "doa acc": 0.0, "doa y": 0.0, "beams y": 0.0, "apply y": 0.0, "apply F": 0.0}
_M, _T, _U = SC.M, SC.T, SC.U


def _note(key, v):
    WORST[key] = max(WORST[key], float(v))


def _freeze(ref):
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _srp_call(dsr, cuda, entry, h, X, nBest, nU):
    """the C entry on sentinel-filled outputs -> ({energy, rp, nbr, nbi, y, g} on the host, acc [U][units])"""
    import torch
    p = lambda t: C.c_void_p(t.data_ptr())
    sent = dict(energy=torch.full((_U, _T), -7.0, dtype=torch.float32, device=cuda), rp=torch.full((_U, _T, nU), -7.0, dtype=torch.float64, device=cuda),
                nbr=torch.full((_U, _T, nBest), -7.0, dtype=torch.float64, device=cuda), nbi=torch.full((_U, _T, nBest), -7, dtype=torch.int32, device=cuda),
                y=torch.full((_U, _T, SC.F, 2), -7.0, dtype=torch.float32, device=cuda), g=torch.full((_U, _T), -7, dtype=torch.int32, device=cuda))
    acc = torch.zeros((_U, nU), dtype=torch.float64, device=cuda)
    Xd = torch.from_numpy(np.array(X)).to(cuda)
    nf = torch.tensor(SC.NFRAMES, dtype=torch.int32, device=cuda)
    dsr.check(entry(h, p(torch.view_as_real(Xd)), p(nf), _U, _T, p(sent["energy"]), p(sent["rp"]), p(sent["nbr"]), p(sent["nbi"]), p(acc), p(sent["y"]),
                    p(sent["g"]), dsr.cur_stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in sent.items()}, acc.cpu().numpy()


def _compare_common(h, accd, ref, what, tag):
    """what test_gpu_sph.py::_run_case and test_gpu_doa.py::test_srp_matches_restatement share: sentinels, energy, gate, rp, N-best, acc"""
    for u, N in enumerate(SC.NFRAMES):
        for k, v in h.items():
            assert np.all(v[u, N:] == -7), (tag, k, u)                       # frames past nframes untouched
        assert np.array_equal(h["energy"][u, :N], ref["energy"][u, :N]), (tag, u)   # bit for bit
        assert np.array_equal(h["g"][u, :N], ref["gated"][u, :N]), (tag, u)
        rr = ref["rp"][u, :N]
        e = (np.abs(h["rp"][u, :N] - rr) / rr.max(axis=1, keepdims=True)).max(); _note(what + " rp", e)
        assert e <= 1e-12, (tag, u, e)
        _check_nbest(h["nbr"][u, :N], h["nbi"][u, :N], ref["nbest_rp"][u, :N], ref["nbest_idx"][u, :N])
    e = (np.abs(accd - ref["acc"]) / np.abs(ref["acc"]).max(axis=1, keepdims=True)).max(); _note(what + " acc", e)
    assert e <= 1e-12, (tag, e)
    return e


def _sph_ref(s, case):
    if case["name"] not in _REF:
        fmin, fmax = case["rng"]
        nU = s.units()
        X = SC.snapshots(case)
        W = np.stack([s.steering(k)[:fmax + 1] for k in range(nU)], axis=1)   # [f][unit][dim], the handle's own table
        Sh = s.harmonics()
        thr, e = SC.gate_threshold(X, fmin, fmax)
        ref = S.run(X, SC.NFRAMES, Sh, W, _M, case["nBest"], fmin, fmax, thr)
        assert np.array_equal(ref["gated"].astype(bool), SC.planted()) and np.array_equal(ref["energy"], np.where(SC.live(), e, 0).astype(np.float32))
        X.setflags(write=False)
        _REF[case["name"]] = (X, thr, _freeze(ref))
    return _REF[case["name"]]


def _run_sph(dsr, cuda, case, path, monkeypatch):
    fmin, fmax = case["rng"]
    s = SC.sph_handle(dsr, case)
    assert s.frequencyRange() == (fmin, fmax)
    nU, nBest = s.units(), case["nBest"]
    X, thr, ref = _sph_ref(s, case)
    s.setEnergyThreshold(thr)
    monkeypatch.setenv("DSR_SPH_SRP_PATH", path)
    assert s.path() == path
    cell, lds = s.cell()                                                     # the launch the call below makes
    if path == "fused":
        assert cell == (0,) + case["expect"], "%s: the fused launch is k_sph_srp<%d, %d> (BC %d, KS %d), the case is there for %s" % (
            (case["name"],) + cell[1:] + (case["expect"],))
    else:
        assert cell[0] == 1 and cell[2] == 0 and cell[3:] == case["expect"][2:]
    h, accd = _srp_call(dsr, cuda, dsr._lib.dsr_sph_srp, s.h, X, nBest, nU)
    tag = "%s %s" % (case["name"], path)
    _compare_common(h, accd, ref, "sph", tag)
    worst_y = 0.0
    for u, N in enumerate(SC.NFRAMES):
        yd = h["y"][u, :N, :, 0] + 1j * h["y"][u, :N, :, 1]
        yr = ref["y"][u, :N, fmin:fmax + 1]
        scale = np.maximum(np.abs(yr).max(axis=1, keepdims=True), 1e-300)
        err = np.abs(yd[:, fmin:fmax + 1] - yr)
        worst_y = max(worst_y, float((err / scale).max()))
        assert np.all(err <= 2e-7 * scale), (tag, u)
        assert np.all(h["y"][u, :N, :fmin] == -7) and np.all(h["y"][u, :N, fmax + 1:] == -7), (tag, u)   # bins outside the range: never written
    _note("sph y", worst_y)
    Rf, If = s.finalNBest(accd)
    for u in range(_U):
        Rr, Ir = S.D.nbest(ref["acc"][u], nBest)
        _check_nbest(Rf[u][None], If[u][None], Rr[None], Ir[None])
    print("%s: k_%s cell %s, LDS %d: rp %.2e, acc %.2e, y %.2e" % (tag, "sph_srp" if path == "fused" else "doa_srp", cell[1:], lds, WORST["sph rp"],
                                                                     WORST["sph acc"], worst_y))
    return h


@pytest.mark.parametrize("case", SC.SPH_CASES, **_ID)
def test_sph_srp_fused_and_folded(dsr, cuda, monkeypatch, case):
    h1 = _run_sph(dsr, cuda, case, "fused", monkeypatch)
    h2 = _run_sph(dsr, cuda, case, "folded", monkeypatch)
    assert np.array_equal(h1["energy"], h2["energy"]) and np.array_equal(h1["g"], h2["g"])


@pytest.mark.parametrize("case", SC.FRAME_CASES, **_ID)
def test_frame_nbest_with_ranks_beyond_the_units(dsr, cuda, monkeypatch, case):
    """k_sph_frame's wave arg-max runs out of units before it runs out of ranks: those ranks are empty, (-10e10, -1), on ungated frames too"""
    nU, nBest = SC.units_of(case["grid"]), case["nBest"]
    ungated = SC.live() & ~SC.planted()
    for path in ("fused", "folded"):
        h = _run_sph(dsr, cuda, case, path, monkeypatch)
        filled = min(nU, nBest)
        assert np.all(h["nbr"][ungated][:, filled:] == -10e10) and np.all(h["nbi"][ungated][:, filled:] == -1)
        idx = h["nbi"][ungated][:, :filled]
        assert idx.min() >= 0 and idx.max() < nU and all(len(set(r)) == filled for r in idx)
        assert np.array_equal(h["nbr"][ungated][:, :filled], np.take_along_axis(h["rp"][ungated], idx.astype(np.int64), axis=1))   # copies of rp
        assert np.all(np.diff(h["nbr"][ungated][:, :filled], axis=1) <= 0)
        assert np.all(h["nbr"][SC.planted()] == -10e10) and np.all(h["nbi"][SC.planted()] == -1)                                  # the gate
    assert (nU < nBest) == (case["name"] == "frame_1unit_nbest3")


@pytest.mark.parametrize("case", SC.DOA_CASES, **_ID)
def test_doa_srp_matches_restatement(dsr, cuda, case):
    Cn, nBest = case["C"], case["nBest"]
    fmin, fmax = case["rng"]
    d = SC.doa_handle(dsr, case)
    cell, lds = d.cell()
    assert cell == case["expect"], "%s: the launch is k_doa_srp<%d> (BC %d, KS %d), the case is there for %s" % ((case["name"],) + cell + (case["expect"],))
    thetas = d.thetas()
    assert len(thetas) == case["nTheta"] and d.frequencyRange() == (fmin, fmax)
    X = SC.snapshots(case)
    x = SC.doa_positions(Cn)
    thr, _ = SC.gate_threshold(X, fmin, fmax)
    d.setEnergyThreshold(thr)
    ref = D.run(X, SC.NFRAMES, x, SC.FS, _M, nBest, thetas, fmin, fmax, thr)
    assert np.array_equal(ref["gated"].astype(bool), SC.planted())
    h, accd = _srp_call(dsr, cuda, dsr._lib.dsr_doa_srp, d.h, X, nBest, len(thetas))
    _compare_common(h, accd, ref, "doa", case["name"])
    worst_y = 0.0
    for u, N in enumerate(SC.NFRAMES):
        yd = h["y"][u, :N, :, 0] + 1j * h["y"][u, :N, :, 1]
        yr = ref["y"][u, :N]
        rms = np.maximum(np.sqrt((np.abs(yr[:, fmin:fmax + 1]) ** 2).mean(axis=1, keepdims=True)), 1e-30)
        err = np.abs(yd[:, fmin:fmax + 1] - yr[:, fmin:fmax + 1])
        worst_y = max(worst_y, float((err / rms).max()))
        assert np.all(err <= 2e-6 * rms), (case["name"], u)
        assert np.all(h["y"][u, :N, :fmin] == -7) and np.all(h["y"][u, :N, fmax + 1:] == -7), (case["name"], u)
    _note("doa y", worst_y)
    Rf, If = d.finalNBest(accd)
    for u in range(_U):
        Rr, Ir = D.nbest(ref["acc"][u], nBest)
        _check_nbest(Rf[u][None], If[u][None], Rr[None], Ir[None])
    print("%s: k_doa_srp cell %s, LDS %d: y %.2e of the frame's rms" % (case["name"], cell, lds, worst_y))


def _check_beams(y, ref, nframes, tag):
    """_check of tests/test_gpu_sph2.py, with the worst error kept"""
    for u, N in enumerate(nframes):
        assert np.all(y[u, :, N:] == 0), (tag, u)                            # rows beyond nframes are exactly 0
        scale = np.abs(ref[u, :, :N]).max(axis=2, keepdims=True)
        err = np.abs(y[u, :, :N] - ref[u, :, :N])
        _note("beams y", (err / scale).max())
        print("%s u %d: max err / frame max = %.3e" % (tag, u, float((err / scale).max())))
        assert np.all(err <= 2e-7 * scale), (tag, u)


@pytest.mark.parametrize("row", SC.BEAM_CASES, ids=lambda r: "c%d_nb%d_%s" % r[:3])
def test_beams_match_restatement(dsr, cuda, monkeypatch, row):
    import torch
    Cn, NB, kernel, kind, mo, T, expect = row
    monkeypatch.delenv("DSR_SPH_BEAMS_PATH", raising=False)
    cell, lds = dsr.sph_beams_cell(NB, Cn, SC.F)
    assert cell == expect and ("valu", "mfma")[cell[0]] == kernel, (cell, expect)
    s = handle(dsr, kind, _M, geom_of(Cn), mo, NC=1, ratio=0.3 if kind.startswith("HWNC") else None)
    dirs = beam_dirs(NB)
    s.setLookDirection(*dirs[0])
    for b in range(1, NB):
        s.setBeam(b, *dirs[b])
    X = _snapshots(_U, Cn, T, _M, seed=Cn + NB)
    nf = [T, 23, 1]                                                          # full, inside the first tile (not on a 16-frame boundary), one frame
    y = s.beams(torch.from_numpy(X).to(cuda), torch.tensor(nf, dtype=torch.int32, device=cuda), NB).cpu().numpy()
    assert y.shape == (_U, NB, T, SC.F)
    _check_beams(y, S2.beams(X, nf, s.beamWeights(NB)), nf, "c%d nb%d %s cell %s LDS %d" % (Cn, NB, kernel, cell, lds))


@pytest.mark.parametrize("kind,Cn,maxOrder", SC.APPLY_CASES)
def test_apply_matches_restatement(dsr, cuda, kind, Cn, maxOrder):
    """k_sph_apply at dim 25 and 49: three and six full groups of 8 eigenbeams, then a group of one"""
    import torch
    T, nf = 40, [40, 23, 1]
    s = dsr.SphDoaSRP(kind, 1, SC.FS, _M, Cn, maxOrder); s.setArrayGeometry(*SC.geometry(Cn))
    assert s.dim == maxOrder * maxOrder and s.dim % 8 == 1
    s.setLookDirection(1.0, 0.3)
    X = _snapshots(_U, Cn, T, _M, seed=Cn + maxOrder)
    y, Fo = s.apply(torch.from_numpy(X).to(cuda), torch.tensor(nf, dtype=torch.int32, device=cuda), want_F=True)
    y, Fo = y.cpu().numpy(), Fo.cpu().numpy()
    yr, Fr = S.apply(X, nf, s.harmonics(), s.lookWeights())
    for u, N in enumerate(nf):
        assert np.all(y[u, N:] == 0) and np.all(Fo[u, N:] == 0)
        sy = np.abs(yr[u, :N]).max(axis=1, keepdims=True); sf = np.abs(Fr[u, :N]).max(axis=(1, 2), keepdims=True)
        ey = np.abs(y[u, :N] - yr[u, :N]); ef = np.abs(Fo[u, :N] - Fr[u, :N])
        _note("apply y", (ey / sy).max()); _note("apply F", (ef / sf).max())
        assert np.all(ey <= 2e-7 * sy)
        assert np.all(ef <= 2e-7 * sf)
    print("%s C %d dim %d: y %.2e, F %.2e of the frame maximum" % (kind, Cn, s.dim, WORST["apply y"], WORST["apply F"]))


def test_zz_report_worst_errors():
    print("worst errors seen: " + ", ".join("%s %.2e" % kv for kv in WORST.items()))
