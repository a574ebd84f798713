"""Inputs shared by tests/test_pf_dispatch_cases_cpu.py and tests/test_gpu_postfilter_kernels.py: one case or more for every cell the dispatch of the
Zelinski / McCowan / Lefkimmiatis post-filters (zelinski_apply_impl, dsr_zelinski_apply_bf, csrc/k_postfilter.hip) can select, on both sides of its
gates, and the ragged batch each runs on.

A case is a dict:
  name       its id, after the cell
  kind       0 Zelinski, 1 McCowan, 2 Lefkimmiatis
  C          channels
  env        the switches the case sets (monkeypatch)
  expect     (cell, template argument) it is there to launch: the values dsr_zelinski_path returns (dsr.h: DSR_PF_*)
  inset      True / False where the case sits next to the gate "C in {2, 3, 4, 6, 8}" (the register instances)
  bf         None, or the beamformer the filter sits behind ("ds" / "mvdr"): dsr_zelinski_apply_bf
  family     "aligned": X_c = s d_c C + 0.8 noise, a source from the look direction (the filters time-align with conj(d_c) x_c, postfilter.cc:30-43);
             "incoherent": noise only; "edge": aligned without noise (a Zelinski weight of 1 up to rounding)
  alpha, type, minFrames   the filter's parameters
  lens       frames per utterance (9 utterances), Tmax = max(lens)
  blocks     [lo, hi) of the carried blocks: a first block of 1 frame, a later cut inside a stretch
Shapes: fftLen 32 (17 bins), 9 utterances: 153 (utterance, bin) series = three workgroups of 64 series (k_zelinski_reg, k_zel_recur), two of 128
(k_mccowan), 153 wavefronts (k_pf_wave); utterance boundaries inside workgroups.
Time axis of the sum kernels: k_zel_recur cuts Tmax into 16 stretches of L = ceil(Tmax / 16) frames and prefetches 8 frames at a time, k_zel_pairs
gives a thread the frames t and t + H, H = ceil(Tmax / 2)."""
import numpy as np

from tests import synth

ZEL_REG, ZEL_SUM, ZEL_SUM_BF, MCCOWAN_REG, MCCOWAN_MEM, WAVE = 0, 1, 2, 3, 4, 5      # dsr.h: DSR_PF_*
CELL_NAMES = ("k_zelinski_reg<C>", "k_zel_pairs<false> + k_zel_recur", "k_zel_pairs<true> + k_zel_recur", "k_mccowan<C>", "k_mccowan<0>", "k_pf_wave<kind>")
M, U = 32, 9
F = M // 2 + 1
REG_SET = (2, 3, 4, 6, 8)
SWITCHES = ("DSR_PF_SUM", "DSR_PF_NOFUSE", "DSR_PF_WAVE", "DSR_PF_MEMSTATE")
# the reference keeps _thresholdOfRij as a float (postfilter.h:163), so does the library; the oracle takes a double, and a clipped pair divides by
# 1 - threshold: 0.99 as a double there would move the weights by 1e-6 relative on the 6-12 % of pairs x bins this geometry clips
THRESHOLD, LOADING, MIN_SV, FBINX1 = float(np.float32(0.99)), 0.05, 1e-8, 3
LADDER = (1, 2, 15, 16, 17, 31, 33, 129, 272)                  # Tmax of the sum kernels: 129 and 272 give stretches of 9 and 17 frames (2 and 3 prefetch batches)


def stretch(Tmax):
    return (Tmax + 15) // 16


def ragged(Tmax):
    """the ragged lengths of a batch of Tmax frames: Tmax, the end inside a stretch, on a stretch edge, at H = ceil(Tmax / 2) and either side of it, 0, 1"""
    L = stretch(Tmax); H = (Tmax + 1) // 2
    k = max(1, min(15, Tmax // L) - 2)                          # a stretch well inside the batch
    inside = k * L + L // 2 if L >= 2 else k * L                # (L = 1: every length ends on an edge)
    lens = [Tmax, inside, k * L, H - 1, H, H + 1, 0, 1, Tmax]
    return [int(min(max(n, 0), Tmax)) for n in lens]


def carried_blocks(Tmax):
    """a first block of 1 frame; a second one whose own Tmax leaves k_zel_recur's last stretch empty while state is carried in (1, 17 or 33 frames);
    the rest in two blocks, cut inside a stretch"""
    if Tmax == 1:
        return [(0, 1)]
    if Tmax == 2:
        return [(0, 1), (1, 2)]
    b2 = 33 if Tmax > 200 else 17 if Tmax > 20 else 1
    c3 = 1 + b2 + (Tmax - 1 - b2) // 2                           # a third cut, inside a stretch of the whole batch
    if stretch(Tmax) >= 2 and c3 % stretch(Tmax) == 0:
        c3 += 1
    return [(0, 1), (1, 1 + b2), (1 + b2, c3), (c3, Tmax)]


def block_lens(lens, lo, hi):
    return [int(min(max(n - lo, 0), hi - lo)) for n in lens]


def _case(name, kind, C, expect, Tmax=40, env=None, inset=None, bf=None, family="aligned", alpha=0.7, type=2, minFrames=0):
    return dict(name=name, kind=kind, C=C, env=dict(env or {}), expect=tuple(expect), inset=inset, bf=bf, family=family, alpha=alpha, type=type,
                minFrames=minFrames, lens=ragged(Tmax), Tmax=Tmax, blocks=carried_blocks(Tmax))


SUM, NOFUSE, WAVE_ENV, MEMSTATE = {"DSR_PF_SUM": "1"}, {"DSR_PF_NOFUSE": "1"}, {"DSR_PF_WAVE": "1"}, {"DSR_PF_MEMSTATE": "1"}

# ------------------------------------------------------------------------------------------------ Zelinski
ZEL_REG_CASES = [
    _case("zreg2", 0, 2, (ZEL_REG, 2), inset=True, type=1, minFrames=5),
    _case("zreg3", 0, 3, (ZEL_REG, 3), inset=True, alpha=0.0),
    _case("zreg4", 0, 4, (ZEL_REG, 4), inset=True, family="incoherent", type=1),
    _case("zreg6", 0, 6, (ZEL_REG, 6), inset=True, minFrames=5),
    _case("zreg8", 0, 8, (ZEL_REG, 8), inset=True, family="edge", type=1),
]
_S = (ZEL_SUM, 0)
# the ladder of Tmax at 5 channels (the first size out of the set), parameters varied along it; then the other sizes and the switch
ZEL_SUM_CASES = [
    _case("zsum5_T1", 0, 5, _S, 1, inset=False),
    _case("zsum5_T2", 0, 5, _S, 2, inset=False, type=1),
    _case("zsum5_T15", 0, 5, _S, 15, inset=False, minFrames=5),
    _case("zsum5_T16", 0, 5, _S, 16, inset=False, alpha=0.0, type=1),
    _case("zsum5_T17", 0, 5, _S, 17, inset=False, family="incoherent", type=1),
    _case("zsum5_T31", 0, 5, _S, 31, inset=False, family="edge"),
    _case("zsum5_T33", 0, 5, _S, 33, inset=False, type=1, minFrames=5),
    _case("zsum5_T129", 0, 5, _S, 129, inset=False, minFrames=5),
    _case("zsum5_T272", 0, 5, _S, 272, inset=False, type=1),
    _case("zsum16_T17", 0, 16, _S, 17, type=1),
    _case("zsum16_T272", 0, 16, _S, 272, alpha=0.0),
    _case("zsum17_T33", 0, 17, _S, 33, minFrames=5),
    _case("zsum17_T129", 0, 17, _S, 129, family="incoherent", type=1),
    _case("zsum64_T31", 0, 64, _S, 31, type=1),
    _case("zsum64_T129", 0, 64, _S, 129, minFrames=5),
    _case("zsum2_switch_T16", 0, 2, _S, 16, SUM, inset=True, minFrames=5),
    _case("zsum2_switch_T129", 0, 2, _S, 129, SUM, inset=True, type=1),
    _case("zsum8_switch_T33", 0, 8, _S, 33, SUM, inset=True, family="edge", type=1),
    _case("zsum8_switch_T272", 0, 8, _S, 272, SUM, inset=True),
]
_B = (ZEL_SUM_BF, 0)
# behind a beamformer of fixed weights (manifold: the beamformer's own); each has a twin with DSR_PF_NOFUSE in the GPU test
ZEL_BF_CASES = [
    _case("zbf5_ds_T33", 0, 5, _B, 33, bf="ds", inset=False, minFrames=5),
    _case("zbf5_mvdr_T129", 0, 5, _B, 129, bf="mvdr", inset=False, type=1),
    _case("zbf17_ds_T129", 0, 17, _B, 129, bf="ds", type=1, minFrames=5),
    _case("zbf17_mvdr_T17", 0, 17, _B, 17, bf="mvdr"),
]
ZEL_WAVE_CASES = [
    _case("zwave3", 0, 3, (WAVE, 0), env=WAVE_ENV, inset=True, type=1, minFrames=5),
    _case("zwave8", 0, 8, (WAVE, 0), env=WAVE_ENV, inset=True),
]


# ------------------------------------------------------------------------------------------------ McCowan, Lefkimmiatis
def _mc(tag, kind):
    def T(C):
        return 18 if C == 64 else 40
    par = {2: dict(type=1), 3: dict(minFrames=5), 4: dict(alpha=0.0, type=1), 5: dict(type=1, minFrames=5), 6: dict(), 7: dict(alpha=0.0),
           8: dict(type=1, minFrames=5), 16: dict(type=1), 17: dict(minFrames=5), 64: dict(type=1)}
    reg = [_case("%sreg%d" % (tag, C), kind, C, (MCCOWAN_REG, C), T(C), inset=True, **par[C]) for C in REG_SET]
    mem = [_case("%smem%d" % (tag, C), kind, C, (MCCOWAN_MEM, 0), T(C), inset=False, **par[C]) for C in (5, 7, 16)]
    mem += [_case("%smem%d_switch" % (tag, C), kind, C, (MCCOWAN_MEM, 0), T(C), MEMSTATE, inset=True, **par[C]) for C in (4, 8)]
    wave = [_case("%swave%d" % (tag, C), kind, C, (WAVE, kind), T(C), **par[C]) for C in (17, 64)]
    wave += [_case("%swave%d_switch" % (tag, C), kind, C, (WAVE, kind), T(C), WAVE_ENV, inset=True, **par[C]) for C in (4, 8)]
    return reg, mem, wave


MC_REG_CASES, MC_MEM_CASES, MC_WAVE_CASES = _mc("mc", 1)
LF_REG_CASES, LF_MEM_CASES, LF_WAVE_CASES = _mc("lf", 2)

ZEL_CASES = ZEL_REG_CASES + ZEL_SUM_CASES + ZEL_BF_CASES + ZEL_WAVE_CASES
NOISE_CASES = MC_REG_CASES + MC_MEM_CASES + MC_WAVE_CASES + LF_REG_CASES + LF_MEM_CASES + LF_WAVE_CASES
ALL_CASES = ZEL_CASES + NOISE_CASES
assert len({c["name"] for c in ALL_CASES}) == len(ALL_CASES)


# ------------------------------------------------------------------------------------------------ inputs
def geometry(case):
    return synth.linear_array(case["C"], 15.0)


def look_delays(oracle, case):
    return oracle.calc_delays_polar2(np.float32(0.5), np.float32(np.pi / 2), geometry(case))


def manifold(oracle, case):
    """[F][C]: the time-alignment vector d / C.  Behind a beamformer it is the beamformer's own (calcArrayManifoldVectors); else random phases"""
    if case["bf"]:
        return oracle.calc_mainlobe(16000.0, look_delays(oracle, case), M)[:F]
    rng = np.random.default_rng(600 + 10 * case["C"] + case["kind"])
    return (np.exp(-1j * rng.uniform(0, 6, (F, case["C"]))) / case["C"]).astype(np.complex128)


def _seed(case):
    return 700 + 13 * case["C"] + case["Tmax"] + 1000 * case["kind"] + 50 * ALL_NAMES.index(case["name"])


ALL_NAMES = [c["name"] for c in ALL_CASES]


def snapshots(case, wq):
    """-> X complex64 [U][C][Tmax][F], rows past an utterance's length zero"""
    Cn, T = case["C"], case["Tmax"]
    rng = np.random.default_rng(_seed(case))
    s = rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))
    sigma = {"aligned": 0.8, "incoherent": 1.0, "edge": 0.0}[case["family"]]
    X = np.zeros((U, Cn, T, F), np.complex64)
    for c in range(Cn):
        x = 0.0 if case["family"] == "incoherent" else s * wq[:, c] * Cn
        if sigma:
            x = x + sigma * (rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F)))
        X[:, c] = x
    for u, n in enumerate(case["lens"]):
        X[u, :, n:] = 0
    return X


def coherence(oracle, case):
    """[F][C][C]: the diffuse-noise coherence of the array with diagonal loading (setDiffuseNoiseModel + setAllLevelsOfDiagonalLoading)"""
    R = oracle.pf_diffuse_noise_model(geometry(case), M, 16000.0)
    R[:, np.eye(case["C"], dtype=bool)] += np.float32(LOADING)
    return R


def beamformed(X, w):
    """Y [U][T][F] = sum_c conj(w[f][c]) X[u][c][t][f] in fp64, rounded to complex64 (what the filter gets from its beamformer)"""
    return np.einsum("fc,uctf->utf", np.conj(w), X.astype(np.complex128)).astype(np.complex64)


def oracle_run(oracle, case, X, Y, wq, u, n, R=None, lam=None):
    """the matching oracle function on the first n frames of utterance u -> (out [n][F], weights [n][F])"""
    Xu = X[u][:, :n].astype(np.complex128); Yu = Y[u][:n].astype(np.complex128)
    a = (case["alpha"], case["type"], case["minFrames"])
    if case["kind"] == 0:
        return oracle.zelinski_postfilter(Xu, Yu, wq, *a)
    if case["kind"] == 1:
        return oracle.mccowan_postfilter(Xu, Yu, wq, R, *a, THRESHOLD)
    return oracle.lefkimmiatis_postfilter(Xu, Yu, wq, R, lam, *a, THRESHOLD, FBINX1)
