"""Inputs shared by tests/test_rls_cases_cpu.py and tests/test_gpu_rls_kernels.py: one case for every cell the dispatch of SubbandGSCRLS
(bf_launch_rls, csrc/k_beamform.hip) can select, on both sides of its two gates, and the ragged batch each runs on.

A case is a dict:
  name     its id, after the cell: where the state lives, the channel count
  C        channels (n = C - 1 active weights, an n x n precision matrix per (utterance, bin))
  env      the switches the case sets (monkeypatch)
  expect   (CT, CAP, residence) of the k_gsc_rls<CT, REG, CAP> it is there to launch: the values dsr_bf_rls_path returns (dsr.h: DSR_RLS_STATE_*)
  gates    {"lds": True (the 64 lanes' state fits 150 KB) / False, "cap16": True (C <= 16) / False} where the case sits next to a gate
  T        frames of the longest utterance
  qc, alpha  setQuadraticConstraint(alpha, qc); qc 0: none
  mode     "gsc" or "gsc_norm"
  adapt    updateActiveWeightVecotrs
  p0       "init": initPrecisionMatrix(SIGMA2_INIT); "set": setPrecisionMatrix with precision_start() on every bin
Shapes: fftLen 32 (17 bins), 9 utterances: 153 (utterance, bin) series = three workgroups of 64 threads, the last one partial, utterance
boundaries inside workgroups; frame counts full, shorter, 1 and 0."""
import numpy as np

from tests import synth

REGS, LDS, MEM = 0, 1, 2                                        # dsr.h: DSR_RLS_STATE_*
M, U = 32, 9
F = M // 2 + 1
MYU, SIGMA2, SIGMA2_INIT = 0.95, 0.01, 0.01
LDS_GATE = 150 * 1024

NOREGS = {"DSR_RLS_NOREGS": "1"}
BOTH = {"DSR_RLS_NOREGS": "1", "DSR_RLS_MEMSTATE": "1"}
MEMSTATE = {"DSR_RLS_MEMSTATE": "1"}
SWITCHES = ("DSR_RLS_NOREGS", "DSR_RLS_MEMSTATE")


def _case(name, C, expect, env=None, gates=None, T=40, qc=0, alpha=-1.0, mode="gsc", adapt=True, p0="init"):
    return dict(name=name, C=C, env=dict(env or {}), expect=tuple(expect), gates=dict(gates or {}), T=T, qc=qc, alpha=alpha, mode=mode,
                adapt=adapt, p0=p0)


# alpha of the qc = 2 cases: chosen per case so that the threshold constraint is both taken and not taken (test_rls_cases_cpu.py counts them)
CASES = [
    _case("regs4", 4, (4, 16, REGS), qc=2, alpha=0.4),
    _case("regs6", 6, (6, 16, REGS), qc=1, alpha=0.3, mode="gsc_norm", p0="set"),
    _case("regs8", 8, (8, 16, REGS)),
    _case("lds4_noregs", 4, (4, 16, LDS), NOREGS, mode="gsc_norm"),
    _case("lds6_noregs", 6, (6, 16, LDS), NOREGS, qc=2, alpha=0.4, p0="set"),
    _case("lds8_noregs", 8, (8, 16, LDS), NOREGS, qc=1, alpha=0.3),
    _case("mem4_both", 4, (4, 16, MEM), BOTH, qc=1, alpha=0.3),
    _case("mem6_both", 6, (6, 16, MEM), BOTH, mode="gsc_norm", p0="set"),
    _case("mem8_both", 8, (8, 16, MEM), BOTH, qc=2, alpha=0.4),
    _case("lds2", 2, (0, 16, LDS), qc=2, alpha=0.4),                                            # a 1 x 1 precision matrix
    _case("lds5", 5, (0, 16, LDS), qc=1, alpha=0.3, mode="gsc_norm"),
    _case("lds12", 12, (0, 16, LDS), gates={"lds": True, "cap16": True}, p0="set"),             # 135 168 bytes: the largest LDS state
    _case("mem5_memstate", 5, (0, 16, MEM), MEMSTATE, qc=2, alpha=0.4, mode="gsc_norm"),
    _case("mem13", 13, (0, 16, MEM), gates={"lds": False, "cap16": True}, qc=1, alpha=0.3, p0="set"),   # 159 744 bytes: past the 153 600 of the gate
    _case("mem16", 16, (0, 16, MEM), gates={"lds": False, "cap16": True}, qc=2, alpha=0.4),
    _case("mem17_cap64", 17, (0, 64, MEM), gates={"lds": False, "cap16": False}, mode="gsc_norm", p0="set"),
    _case("mem64_cap64", 64, (0, 64, MEM), gates={"lds": False, "cap16": False}, T=18, qc=2, alpha=0.02),
    # adaptation off: the fixed GSC through each residence
    _case("regs4_fixed", 4, (4, 16, REGS), adapt=False),
    _case("lds5_fixed", 5, (0, 16, LDS), adapt=False, mode="gsc_norm"),
    _case("mem13_fixed", 13, (0, 16, MEM), adapt=False),
]
assert len({c["name"] for c in CASES}) == len(CASES)
# block 1 in registers, block 2 in LDS, block 3 in memory: the carried layout is documented as common to the three residences
CROSS_CASE = _case("cross6", 6, (6, 16, REGS), qc=2, alpha=0.4)
CROSS_ENVS = [({}, REGS), (NOREGS, LDS), (BOTH, MEM)]


def lens_of(case):
    """frames per utterance: full, shorter, 1, 0, ..."""
    T = case["T"]
    return [T, T - 11, 1, 0, T, T - 5, T // 2 - 3, T, 5]


def blocks_of(case):
    """three carried blocks [lo, hi): one frame, then a cut inside the stream; the utterance of 1 frame gets 0 frames in the middle block"""
    T = case["T"]
    return [(0, 1), (1, T // 3), (T // 3, T)]


def block_lens(lens, lo, hi):
    return [int(min(max(n - lo, 0), hi - lo)) for n in lens]


def design(oracle, C):
    """-> (microphone positions, delays, wq [M][C], B [F][C][C - 1]) as the reference computes them (calcGSCWeights)"""
    mp = synth.linear_array(C, 25.0)
    delays = oracle.calc_delays_polar2(np.float32(0.4), np.float32(1.2), mp)
    wq = oracle.calc_mainlobe(16000.0, delays, M)
    B = np.array([oracle.blocking_matrix(wq[f])[0] for f in range(F)])
    return mp, delays, wq, B


def precision_start(C):
    """[F][n][n]: a Hermitian positive definite start that is no multiple of the identity (setPrecisionMatrix)"""
    n = C - 1
    rng = np.random.default_rng(77 + C)
    A = rng.standard_normal((F, n, n)) + 1j * rng.standard_normal((F, n, n))
    return 60.0 * np.eye(n)[None] + 20.0 * (A @ np.conj(np.swapaxes(A, 1, 2))) / n


def snapshots(case, wq):
    """-> X complex64 [U][C][T][F], rows past an utterance's length zero: a source from the look direction (s d_c, d = C wq) + noise"""
    Cn, T = case["C"], case["T"]
    rng = np.random.default_rng(900 + Cn + (7 if case["name"].startswith("cross") else 0))
    s = rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))
    X = np.stack([s * wq[:F, c] * Cn + 0.7 * (rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))) for c in range(Cn)], axis=1)
    X = X.astype(np.complex64)
    for u, n in enumerate(lens_of(case)):
        X[u, :, n:] = 0
    return X


def full(a):
    """[...][F] unique bins -> [...][M] with the conjugate mirror (what the reference's vectors hold)"""
    f = np.zeros(a.shape[:-1] + (M,), np.complex128); f[..., :F] = a; f[..., F:] = np.conj(a[..., 1:F - 1][..., ::-1])
    return f


def oracle_run(oracle, case, X, wq, B, u, n):
    """the oracle on the first n frames of utterance u -> (Y [n][F], final active weights [F][C - 1])"""
    P0 = precision_start(case["C"]) if case["p0"] == "set" else None
    Y, wa = oracle.gsc_rls(full(X[u][:, :n]), wq, B, MYU, SIGMA2, SIGMA2_INIT, case["alpha"], case["qc"], case["adapt"], case["mode"] == "gsc_norm", P0=P0)
    return Y[:, :F], wa


def rls_numpy(case, Xu, wq, B):
    """the restatement of tests/test_oracle_cpu.py::test_gsc_rls_against_numpy (numpy matrix algebra, another summation order) on one utterance
    Xu [C][n][F] -> (final active weights [F][C - 1], steps with the threshold constraint taken, steps with it idle)"""
    Cn = case["C"]; n = Cn - 1; T = Xu.shape[1]
    muf, s2f, af = float(np.float32(MYU)), float(np.float32(SIGMA2)), float(np.float32(case["alpha"]))
    if case["p0"] == "set":
        P = [p.copy() for p in precision_start(Cn)]
    else:
        P = [np.eye(n, dtype=complex) * float(np.float32(1.0) / np.float32(SIGMA2_INIT)) for _ in range(F)]
    wa = np.zeros((F, n), complex); taken = idle = 0
    for t in range(T):
        for f in range(1, F):
            x = Xu[:, t, f].astype(np.complex128)
            w = wq[f] - B[f] @ wa[f]
            if case["mode"] == "gsc_norm":
                w = w / (np.linalg.norm(w) * Cn)
            y = np.vdot(w, x)
            Z = B[f].conj().T @ x
            PZ = P[f] @ Z; PH = P[f].conj().T @ Z
            g = (PZ / muf) / (np.vdot(PH, Z) / muf + 1.0)
            P[f] = (P[f] - np.outer(g, PH.conj())) / muf
            w2 = (np.eye(n) - s2f * P[f]) @ wa[f] + g * np.conj(y)
            nr = np.linalg.norm(w2)
            if case["qc"] == 1 or (case["qc"] == 2 and nr * nr >= af):
                w2 = w2 * (af / nr); taken += 1
            else:
                idle += 1
            wa[f] = w2
    return wa, taken, idle
