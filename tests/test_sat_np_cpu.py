"""CPU tests of speaker-adaptive training: the numpy restatement (tests/sat_np.py) on the recipes of tests/sat_cases.py, and the library's
host side through the C-ABI where no device is needed (include/dsr.h section 14: dsr_sat_check, dsr_speaker_list_read, the null refusals).
A dsr_sat is created over a trainer, which needs a device: its slot tables and the refusals of accumulate are in tests/test_gpu_sat.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import adapt_np as A
from tests import sat_cases as Cs
from tests import sat_np as N
from tests.conftest import PKG

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("S", Cs.RECIPE_S)
@pytest.mark.parametrize("D", Cs.RECIPE_D)
def test_recipe_is_far_from_every_tie_and_the_restatement_recovers_the_model(D, S):
    p = Cs.Problem(D, 1, [2, 3], [4, 3], S, seed=10 * D + S); acc = p.mean_accus()
    for g in range(p.G):
        M, v = acc.mat[g, 0], acc.vec[g, 0]
        q, kept, s = N.solve(M, v)
        assert kept == D and (s / s[0]).min() >= 0.2
        assert np.abs(np.linalg.lstsq(M, v, rcond=None)[0] - p.muStar[g]).max() <= 3e-14 * max(1.0, np.abs(p.muStar[g]).max())
    r = N.update_means(acc.mat, acc.vec, acc.scalar, acc.occ, acc.has, p.m.mean, 1.0)               # the counts are >= 5
    assert (r["auxNew"] <= r["auxOld"]).all() and (r["decision"] == N.UPDATED).all()               # the auxiliary function does not go up
    assert r["info"] == [p.G, p.G, p.G * D, p.G * D] and r["totals"] == [p.G, p.G]
    assert (np.abs(r["mean"].astype(f64) - p.muStar) <= 2.0 ** -23 * np.abs(p.muStar) + 1e-10).all()
    assert r["aux"] == sum(r["auxNew"].ravel().tolist())                                            # the model-order sum
    # the variances, with the model at mu*
    va = N.VarAccus(p.G, D)
    for s in range(S):
        va.accumulate(p.classes, p.muStar.astype(f32), p.c[s], p.sumO[s], p.sumOsq[s], p.xf[s], exact=p.y[s])
    cv, tot = N.update_variances(va.vec, va.occ, p.m.cv, 1.0)
    tol = 2.0 ** -23 * p.sigma2 + (va.model + 4 * S * 2.0 ** -53 * va.bound) / va.occ[:, None]
    assert tot == [p.G, p.G] and (np.abs(cv.astype(f64) - p.sigma2) <= tol).all()


@pytest.mark.parametrize("D,k", Cs.DEFICIENT)
def test_deficient_speaker_has_an_unambiguous_rank(D, k):
    p = Cs.Problem(D, 1, [1], [5], 1, seed=D, deficient=k); acc = p.mean_accus()
    for g in range(p.G):
        q, kept, s = N.solve(acc.mat[g, 0], acc.vec[g, 0]); r = s / s[0]
        assert kept == D - k and r[:D - k].min() >= 0.2 and r[D - k:].max() <= 1e-16
    r = N.update_means(acc.mat, acc.vec, acc.scalar, acc.occ, acc.has, p.m.mean, 1.0)
    assert (r["auxNew"] <= r["auxOld"]).all() and r["info"][3] == p.G * (D - k) and r["info"][2] == p.G * D


def test_thresholds_zero_occupancy_and_the_keep_old_branch():
    D = 3; p = Cs.Problem(D, 1, [1], [4], 2, seed=5)
    # Gaussian 0: below the threshold; 1: counts +5 and -5 (occ == 0 with blocks); 2: never a count (no blocks); 3: indefinite, occ 15
    p.c[0][:] = [4.0, 5.0, 0.0, 30.0]; p.c[1][:] = [3.0, -5.0, 0.0, -15.0]
    p.xf[0][1] = N.Xform(N.MLLR, 0.1 * np.eye(D), np.zeros(D)); p.xf[1][1] = N.Xform(N.MLLR, np.eye(D), np.zeros(D))
    acc = p.mean_accus()
    assert acc.occ.tolist() == [7.0, 0.0, 0.0, 15.0] and acc.has.tolist() == [True, True, False, True]
    r = N.update_means(acc.mat, acc.vec, acc.scalar, acc.occ, acc.has, p.m.mean, -1.0)           # every occupancy reaches the threshold
    assert r["decision"][:, 0].tolist() == [N.UPDATED, N.ZEROED, N.LEFT, N.KEPT_OLD]
    assert (r["mean"][1] == 0).all() and np.array_equal(r["mean"][2], p.m.mean[2]) and np.array_equal(r["mean"][3], p.m.mean[3])
    assert r["auxOld"][3, 0] < r["auxNew"][3, 0] - 1.0                                            # by a wide margin
    assert r["info"] == [2, 1, D, D] and r["totals"] == [4, 4]
    r = N.update_means(acc.mat, acc.vec, acc.scalar, acc.occ, acc.has, p.m.mean, 0.0)            # massThreshold 0 means 10
    assert r["decision"][:, 0].tolist() == [N.LEFT, N.LEFT, N.LEFT, N.KEPT_OLD] and r["totals"] == [4, 1]
    cv, tot = N.update_variances(np.ones((4, D)), np.array([7.0, 0.0, 12.0, np.nan]), np.full((4, D), 4.0, f32), -1.0, gs=[0, 1, 2])
    assert cv[:3, 0].tolist() == [f32(1.0 / 7.0), 0.0, f32(1.0 / 12.0)] and tot == [3, 3]
    cv, tot = N.update_variances(np.ones((4, D)), np.array([7.0, 0.0, 12.0, 1.0]), np.full((4, D), 4.0, f32), 0.0)
    assert cv[:, 0].tolist() == [0.25, 0.25, f32(1.0 / 12.0), 0.25] and tot == [4, 1]            # below the threshold: fixup, 1 / var
    with pytest.raises(N.NumericError):
        N.update_variances(np.full((1, D), np.nan), np.array([20.0]), np.ones((1, D), f32), 0.0)


def test_transformer_lookup_and_block_counts():
    x = N.Xform(N.MLLR, np.eye(2), np.zeros(2)); xf = {2: x, 3: x, 6: x}
    assert N.transformer(xf, 2) is x and N.transformer(xf, 6) is x
    with pytest.raises(A.ConsistencyError):
        N.transformer(xf, 3)                                                                      # 6 is below 3: not a leaf
    with pytest.raises(A.KeyError_):
        N.transformer(xf, 5)                                                                      # the exact node, no ancestor
    with pytest.raises(A.IndexError_):
        N.transformer(xf, 0)
    a = N.MeanAccus(1, 4); one = np.ones((1, 4))
    a.accumulate([1], one, [0.0], one, {1: N.Xform(N.MLLR, np.eye(4), np.zeros(4))})
    assert not a.has[0] and a.occ[0] == 0.0                                                       # a zero count: nothing, not even the blocks' shape
    a = N.MeanAccus(1, 4)
    a.accumulate([1], one, [2.0], one, {1: N.Xform(N.APT, np.stack([np.eye(2)] * 2), np.zeros(4))})
    with pytest.raises(N.DimensionError):
        a.accumulate([1], one, [2.0], one, {1: N.Xform(N.MLLR, np.eye(4), np.zeros(4))})          # a second batch with another block count
    with pytest.raises(N.DimensionError):
        N.MeanAccus(1, 4).accumulate([1], one, [2.0], one, {1: N.Xform(N.APT, np.zeros((3, 1, 1)), None)})


def test_transform_restatements_agree_with_the_adaptation_modules():
    from tests import apt_np as P
    rng = np.random.default_rng(3); D = 6; mu = rng.standard_normal((5, D)).astype(f32); W = rng.standard_normal((D, D + 1))
    assert np.array_equal(N.transform_mean(N.Xform(N.MLLR, W[:, :D], W[:, D]), mu), A.transform_means(W, mu))
    M = P.matrix(1, [0.2], 3); bias = rng.standard_normal(3).astype(f32)
    assert np.array_equal(N.transform_mean(N.apt_xform(M, 2, bias), mu), P.transform(M, mu, 2, bias))
    assert np.array_equal(N.transform_mean(N.apt_xform(M, 2), mu), P.transform(M, mu, 2))


def test_speaker_list_and_file_names(dsr, tmp_path):
    long_label = "x" * 150
    data = ("spk1\nB02\n%s\nlast" % long_label).encode()
    want = ["spk1", "B02", "x" * 127, "x" * 23, "last"]                                           # fgets(buffer, 128): a longer line arrives in pieces
    assert N.speaker_list(data) == want
    f = tmp_path / "list.txt"; f.write_bytes(data)
    assert dsr.speaker_list_read(str(f)) == want
    from dsr.asr.sat import SpeakerListPtr
    assert list(SpeakerListPtr(str(f))) == want and len(SpeakerListPtr(str(f))) == 5
    (tmp_path / "bad.txt").write_bytes(b"a\n\nb\n")
    with pytest.raises(N.ParseError):
        N.speaker_list(b"a\n\nb\n")
    with pytest.raises(dsr.DsrError) as e:
        dsr.speaker_list_read(str(tmp_path / "bad.txt"))
    assert e.value.status == dsr.E_PARSE
    with pytest.raises(dsr.DsrError) as e:
        dsr.speaker_list_read(str(tmp_path / "missing.txt"))
    assert e.value.status == dsr.E_IO
    assert N.accu_file("accus/", "spk1") == "accus/spk1.cbs.accu" and N.param_file("params/", "spk1") == "params/spk1"
    assert N.param_file("params", "spk1") == "paramsspk1"                                         # no separator, sat:1890
    assert N.estimate_return([f32(-10.5), f32(-20.25)], [100, 200]) == -30.75 / 300


def test_refusals_that_need_no_device(dsr):
    L = dsr.load()
    dsr.sat_check(0, 39); dsr.sat_check(39, 39, 0.0, 1)
    for args, status in (((42, 39, 0.0, 0), dsr.E_DIMENSION), ((39, 39, 0.5, 0), dsr.E_PARAMETER), ((39, 39, 0.0, 2), dsr.E_PARAMETER),
                         ((39, 39, 0.0, 3), dsr.E_PARAMETER), ((39, 39, 0.0, 4), dsr.E_PARAMETER)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.sat_check(*args)
        assert e.value.status == status, args
    h = C.c_void_p()
    assert L.dsr_sat_create(None, 1, 0.0, 1, 1, C.byref(h)) == dsr.E_PARAMETER and not h.value
    assert L.dsr_sat_accumulate(None, 1, 1, None) == dsr.E_PARAMETER and L.dsr_sat_zero(None) == dsr.E_PARAMETER
    assert L.dsr_sat_gaussian_status(None, 0) == dsr.E_INDEX and L.dsr_sat_num_slots(None) == 0
    import dsr._capi as K
    assert K.Sat.__module__ == "dsr._sat" and K.SAT_MEAN == 1 and K.SAT_VARIANCE == 2


def test_cpp_facade_names_compile(tmp_path):
    src = tmp_path / "s.cpp"
    src.write_text('#include "dsr_streams.hpp"\n#include <cstdio>\nint main(int argc, char** argv) {\n'
                   '  SpeakerListPtr s(new SpeakerList(argv[1])); printf("%d %s\\n", (int) s->speakers().size(), s->speakers()[1].c_str());\n'
                   '  try { SpeakerList t("/nonexistent/list"); } catch (jio_error& e) { printf("io %d\\n", (int) e.getCode()); }\n'
                   '  MeanSATPtr m; VarianceSATPtr v; return (m || v) ? 1 : 0; }\n')
    lst = tmp_path / "l.txt"; lst.write_text("a1\nb2\n")
    exe = tmp_path / "s"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(lst)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split("\n")[:2] == ["2 b2", "io 7"], out.stdout + out.stderr
