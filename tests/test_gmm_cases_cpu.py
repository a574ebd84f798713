"""The near-tie inputs of tests/gmm_cases.py do what tests/test_gpu_gmm_shapes.py relies on -- conditions on the INPUTS, checked without a GPU against the
oracle's _scoreOpt and a numpy emulation of the expanded form's fp32 arithmetic (the kernel is not involved):
  * among the frames placed within 1e-7 S of a tie, the expanded form evaluated in fp32 picks another Gaussian than the reference's own arithmetic
    on at least 30 % (measured 40-52 %): a kernel that trusts the expanded form there is wrong every second time;
  * the placed pair is the codebook's two nearest on at least 90 % of the frames, so the tie is the one that decides the argmin;
  * the 'negative' family's distances are negative, the 'straddle' family's come with both signs.
Run with -s for the measured shares of every (family, dimN, R)."""
import numpy as np
import pytest

from tests import gmm_cases as GC

N_TIE = 3000            # (about 1400 of them within 1e-7 S: the share is measured to +-0.013)


def _measure(oracle, family, D, R):
    K = 37 if R == 4 else dict(GC.WIDE_R)[R]
    m = GC.model(family, K, R, D, seed=3)
    x, info = GC.near_tie_frames(m, N_TIE, seed=100 + D + R)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    _, arg = oracle.gmm_score_opt(cb, m["val"], x)
    n = np.arange(N_TIE); k = info["k"]
    ref = arg[n, k]                                                            # the reference's nearest Gaussian of the frame's own codebook
    g = (k * R)[:, None] + np.arange(R)[None, :]
    emu = GC.emulate_expanded(m, x, g).argmin(1)                               # (argmin: the first of equals, as the reference's strict '<')
    d64 = GC.dist64(m, x, g)
    two = np.sort(np.argsort(d64, 1)[:, :2], 1)
    pair = np.sort(np.stack([info["a"], info["b"]], 1), 1)
    close = info["g"] <= 1e-7
    best = d64.min(1)
    return dict(flip=float((emu != ref)[close].mean()), nclose=int(close.sum()), top2=float((two == pair).all(1).mean()),
                inpair=float(((ref == info["a"]) | (ref == info["b"])).mean()), neg=float((best < 0).mean()))


@pytest.mark.parametrize("family,D,R", GC.tie_shapes())
def test_near_tie_inputs_have_teeth(oracle, family, D, R):
    r = _measure(oracle, family, D, R)
    print("%-9s D=%2d R=%2d: flip share %.2f of %d frames within 1e-7 S, placed pair top two %.2f, reference argmin in the pair %.2f, negative %.2f"
          % (family, D, R, r["flip"], r["nclose"], r["top2"], r["inpair"], r["neg"]))
    assert r["nclose"] >= 1000
    assert r["flip"] >= 0.30
    assert r["top2"] >= 0.90 and r["inpair"] >= 0.90
    if family == "negative":
        assert r["neg"] >= 0.99
    elif family == "straddle":
        assert 0.1 <= r["neg"] <= 0.9
    elif family == "unit":
        assert r["neg"] == 0.0
    if GC.FAMILIES[family][2]:                                                 # "everything is re-scored" holds for the mix the GPU tests score
        K = 37 if R == 4 else dict(GC.WIDE_R)[R]
        m = GC.model(family, K, R, D, seed=3)
        assert GC.best_over_S(m, GC.frames(family, m, 1431, seed=10 + D)[0]) < 1e-3


def test_emulation_agrees_with_reference_away_from_ties(oracle):
    """the emulated expanded form is the same function as the oracle's distance: on plain frames (no ties) both pick the same Gaussian, and the
    emulated best distance lies within the header's bound (2 dimN + 3) 2^-24 S of the float64 one"""
    D, R, K = 39, 4, 37
    m = GC.model("unit", K, R, D, seed=3)
    x = GC.plain_frames("unit", 300, D, seed=5)
    cb = oracle.Codebooks(m["refN"], m["mean"], m["ivar"], m["det"])
    _, arg = oracle.gmm_score_opt(cb, m["val"], x)
    S = GC.frame_S(m, x)
    for k in (0, 17, 36):
        g = np.tile(k * R + np.arange(R), (x.shape[0], 1))
        e = GC.emulate_expanded(m, x, g)
        d = GC.dist64(m, x, g)
        assert np.array_equal(e.argmin(1), arg[:, k])
        assert (np.abs(e - d) <= (2 * D + 3) * 2.0 ** -24 * S[:, None]).all()


def test_frames_mix_and_sizes():
    m = GC.model("unit", 5, 4, 13, seed=3)
    for N in (1, 129, 515):
        x, tie, info = GC.frames("unit", m, N, seed=9)
        assert x.shape == (N, 13) and x.dtype == np.float32 and tie.sum() == (N + 1) // 2 and tie[info["row"]].all()
    r = GC.model("unit", 3, 0, 13, seed=3, refN=[3, 7, 33])
    x, info = GC.near_tie_frames(r, 50, seed=2)
    assert (info["a"] < np.asarray([3, 7, 33])[info["k"]]).all() and (info["a"] != info["b"]).all()
