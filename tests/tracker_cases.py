"""The cases of the tracker tests (tests/test_tracker_np_cpu.py, tests/test_gpu_tracker.py) and their shared references.

Small by default: M = 32 (17 bins), EigenMike, U = 3 utterances of 12, 7 and 1 frames.  The input is a random source spectrum through the restated
PlaneWaveSimulator, steered at a direction that drifts about 0.02 rad a frame from near (0.6, 0.2), plus noise at -30 dB, cast to complex64.
reference(case) runs the restatement (tests/tracker_np.py) once per case in float64 and in the second precision and keeps both.

A case may carry its own fftLen, batch and frame counts (keys M, U, frames; dims(case) gives the derived sizes): k_trk_run is one workgroup of
256 threads per utterance, and the cases at the end of CASES are there for what M = 32 cannot reach (the table is in tests/test_gpu_tracker.py).
Their source spectrum is shaped (key loud: a band of bins scaled up; key only: every other bin zero and no noise), so that the bins the
tracker keeps are the ones the case is about; tests/test_tracker_np_cpu.py checks that they are."""
import functools

import numpy as np

from tests import tracker_np as T

M, F, U, TMAX = 32, 17, 3, 12
NFRAMES = [12, 7, 1]
A_MM, FS = 42.0, 16000.0
SIM_ORDER = 3
SIGMA2_U, SIGMA2_V, SIGMA2_INIT = 0.01, 0.1, 1.0


def _case(name, kind, orderN, useSubbandsN, maxLocalN, seed, setV=False, init=None, start=(0.6, 0.2), mid=None, M=M, U=U, frames=None, loud=None, only=None):
    """loud: (first bin, last bin, factor) on the source's amplitude; only: the source's non-zero bins, and no noise is added"""
    frames = list(NFRAMES if frames is None else frames)
    assert len(frames) == U
    return dict(name=name, kind=kind, orderN=orderN, useSubbandsN=useSubbandsN, maxLocalN=maxLocalN, seed=seed, setV=setV, init=init, start=start, mid=mid,
                M=M, U=U, frames=frames, loud=loud, only=only)


def dims(case):
    """(M, F, U, TMAX, frames) of a case"""
    return case["M"], case["M"] // 2 + 1, case["U"], max(case["frames"]), case["frames"]


CASES = []
for _kind, _order, _use in (("modal", 2, 4), ("modal", 3, 0), ("spatial", 2, 4), ("spatial", 3, 6)):
    for _local in (1, 4):
        CASES.append(_case("%s-o%d-s%d-l%d" % (_kind, _order, _use, _local), _kind, _order, _use, _local, seed=11))
CASES += [
    _case("modal-setV", "modal", 2, 4, 2, seed=12, setV=True),
    _case("spatial-setV", "spatial", 2, 4, 2, seed=13, setV=True),
    _case("modal-clamp", "modal", 2, 4, 2, seed=14, init=(0.02, 0.0), start=(0.005, 0.2)),          # the source above the clamp: theta < 0.01 is limited
    _case("spatial-mid", "spatial", 2, 4, 2, seed=15, mid=(5, (0.7, 0.1))),                           # nextSpeaker + setInitialPosition before frame 5
]
OLD_CASES = len(CASES)                                                                              # the cases above keep their inputs bit for bit
CASES += [
    # more bins than the workgroup has threads: every per-bin loop wraps, and the loud band puts bin 256 (thread 0's second bin) among the kept ones
    _case("modal-F257", "modal", 2, 4, 2, seed=21, M=512, U=2, frames=[4, 2], loud=(250, 256, 4.0)),
    _case("spatial-F257", "spatial", 2, 4, 2, seed=22, M=512, U=2, frames=[4, 2], loud=(250, 256, 4.0)),     # F L = 8224 observation entries
    # 2N = 2 x 41 x 32 = 2624 rows: 70 824 bytes of LDS, above the 64 KiB a kernel gets without asking
    _case("spatial-lds64k", "spatial", 2, 41, 1, seed=23, M=128, U=2, frames=[3, 1]),
    # |B| is exactly zero in all bins but two: the ties among the zeros go to the lowest bins
    _case("modal-ties", "modal", 2, 4, 1, seed=24, M=512, U=1, frames=[3], only=(200, 256)),
]
BY_NAME = {c["name"]: c for c in CASES}

# where long double is no wider than double the second opinion is a float64 run with every dot product summed in reverse
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def second_precision():
    return dict(dtype=np.longdouble) if WIDE else dict(dtype=np.float64, reverse=True)


def directions(case):
    """[U][TMAX][2]: the true direction of every frame"""
    _, _, U, TMAX, _ = dims(case)
    d = np.zeros((U, TMAX, 2))
    for u in range(U):
        t = np.arange(TMAX)
        d[u, :, 0] = case["start"][0] + (0.012 if case["start"][0] > 0.1 else 0.0) * t + 0.01 * u
        d[u, :, 1] = case["start"][1] + 0.016 * t - 0.02 * u
    return d


@functools.lru_cache(maxsize=None)
def sim_decomposition(M=M):
    return T.Decomposition(False, SIM_ORDER, M, A_MM, FS)


def pws_coefficients(dec, theta, phi):
    """[32][F]: PlaneWaveSimulator's coefficients of every channel, the restated sums vectorised over channels and bins (same order of terms)"""
    Y = np.array([T.harmonic(n, m, theta, phi) for n, m in dec.modes])
    coef = np.zeros((T.CHAN, dec.F), np.complex128)
    for n in range(dec.orderN + 1):
        coeff_n = np.zeros(T.CHAN, np.complex128)
        for m in range(-n, n + 1):
            idx = n * n + n + m
            coeff_n = coeff_n + dec.sc[idx] * Y[idx]
        coef = coef + dec.bn[None, :, n] * coeff_n[:, None]
    return coef


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = BY_NAME[name]
    M, F, U, TMAX, NFRAMES = dims(case)
    rng = np.random.default_rng(case["seed"])
    src = (rng.standard_normal((U, TMAX, F)) + 1j * rng.standard_normal((U, TMAX, F))) / np.sqrt(2.0)
    if case["loud"]:
        src[:, :, case["loud"][0]:case["loud"][1] + 1] *= case["loud"][2]
    if case["only"]:
        keep = np.zeros(F, bool); keep[list(case["only"])] = True
        src[:, :, ~keep] = 0.0
    d = directions(case)
    dec = sim_decomposition(M)
    X = np.zeros((U, T.CHAN, TMAX, F), np.complex128)
    for u in range(U):
        for t in range(TMAX):
            X[u, :, t, :] = pws_coefficients(dec, d[u, t, 0], d[u, t, 1]) * src[u, t][None, :]
    p = np.mean(np.abs(X) ** 2)
    noise = (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)) * np.sqrt(p * 1e-3 / 2.0)
    if case["only"]:
        noise[:] = 0.0
    X = (X + noise).astype(np.complex64)
    for u in range(U):
        X[u, :, NFRAMES[u]:, :] = 0
    Vs = None
    if case["setV"]:
        L = T.CHAN if case["kind"] == "spatial" else (case["orderN"] + 1) ** 2
        Vs = np.zeros((F, L, L), np.complex128)
        for f in range(F):
            A = (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / np.sqrt(2.0 * L)
            Vs[f] = 0.02 * (A @ A.conj().T) + 0.1 * np.eye(L)            # Hermitian, positive definite and diagonally dominant
    return src, X, Vs


def inputs(case):
    """(source [U][TMAX][F] complex128, X [U][32][TMAX][F] complex64, V blocks [F][L][L] or None)"""
    return _inputs(case["name"])


def make_tracker(case, **prec):
    M, F = dims(case)[:2]
    dec = T.Decomposition(case["kind"] == "spatial", case["orderN"], M, A_MM, FS, case["useSubbandsN"], **prec)
    trk = T.Tracker(dec, SIGMA2_U, SIGMA2_V, SIGMA2_INIT, case["maxLocalN"])
    Vs = inputs(case)[2]
    if Vs is not None:
        for f in range(F):
            trk.setV(Vs[f], f)
    return trk


def run_restatement(case, **prec):
    """-> dict(pos64 [U][TMAX][2], pos [U][TMAX][2] float32, info [U][TMAX] int32, logs [U] lists)"""
    _, X, _ = inputs(case)
    _, _, U, TMAX, NFRAMES = dims(case)
    trk = make_tracker(case, **prec)
    rt = trk.rt
    pos64 = np.zeros((U, TMAX, 2), rt)
    pos = np.zeros((U, TMAX, 2), np.float32)
    info = np.zeros((U, TMAX), np.int32)
    logs = []
    for u in range(U):
        trk.nextSpeaker()
        if case["init"]:
            trk.setInitialPosition(*case["init"])
        trk.log = []
        for t in range(NFRAMES[u]):
            if case["mid"] and t == case["mid"][0]:
                trk.nextSpeaker()
                trk.setInitialPosition(*case["mid"][1])
            pos[u, t] = trk.next(X[u, :, t, :].T)
            pos64[u, t] = trk.log[-1]["pos64"]
            info[u, t] = T.info_word(trk.log[-1])
        logs.append(trk.log)
    return dict(pos64=pos64, pos=pos, info=info, logs=logs)


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = BY_NAME[name]
    a = run_restatement(case)
    b = run_restatement(case, **second_precision())
    s_case = float(np.abs(a["pos64"].astype(np.longdouble) - b["pos64"].astype(np.longdouble)).max())
    return dict(ref=a, second=b, s_case=s_case)


def reference(case):
    """the float64 run, the second-precision run and s_case = the largest difference of their pos64: the restatement's own rounding sensitivity"""
    return _reference(case["name"])
