"""Inputs shared by tests/test_abf_np_cpu.py and tests/test_gpu_abf.py: one case for every cell the dispatch of the adaptive subband beamformers
(abf_launch, csrc/abf_kernels.hip) can select, for each of the three adaptive kinds, on both sides of its gates, and the ragged batch each runs on.

A case is a dict:
  name     its id: the kind, then the cell (where the state lives, the channel count)
  kind     "gj", "mvdr" or "mpdr"
  C        channels
  env      the switches the case sets (monkeypatch)
  expect   (CT, CAP, residence): the values dsr_abf_path returns (dsr.h: DSR_ABF_STATE_*)
  gates    {"lds": the 64 lanes' state and factor fit 150 KB, "cap16": C <= 16} where the case sits next to a gate
  T        frames of the longest utterance
  params   the reference constructor's parameters
  scale    factor on the snapshots (1e3: filter-bank amplitudes)
  wp       frames of post-filter weights (0: none); Griffiths-Jim cases use fewer than T, MVDR's wp1L covers every frame
Shapes as tests/rls_cases.py: fftLen 32 (17 bins), 9 utterances: 153 (utterance, bin) series = three workgroups of 64 threads, the last one partial,
utterance boundaries inside workgroups; frame counts full, shorter, 1 and 0.  Snapshots as rls_cases.snapshots with an on/off envelope over the
frames, so that the Griffiths-Jim gate closes."""
import numpy as np

from tests import abf_np as A
from tests import synth
from tests.rls_cases import lens_of, blocks_of, block_lens      # noqa: F401  (the ragged batch and the three carried blocks)

REGS, LDS, MEM = 0, 1, 2                                        # dsr.h: DSR_ABF_STATE_*
M, U = 32, 9
F = M // 2 + 1
LDS_GATE = 150 * 1024
NOREGS = {"DSR_ABF_NOREGS": "1"}
BOTH = {"DSR_ABF_NOREGS": "1", "DSR_ABF_MEMSTATE": "1"}
MEMSTATE = {"DSR_ABF_MEMSTATE": "1"}
SWITCHES = ("DSR_ABF_NOREGS", "DSR_ABF_MEMSTATE")
CT_LIST = (4, 6, 8)

# Griffiths-Jim: the gate, the norm constraint and the floor are each taken and left (test_abf_np_cpu.py counts them)
GJ = dict(beta=0.9, gamma=0.05, initDiagLoad=3.0, floorSubBandSigmaK=None, silThresh=30.0, alpha2=None, staticAfter=None)
SMI = dict(diagLoad=0.001, forgetFactor=0.95, end=20)


def state_entries(kind, C):
    """(state, factor) complex fp64 entries of a thread, as DESIGN 4.4t states them"""
    n = C - 1
    if kind == "gj":
        return n + 1, 0
    m = C if kind == "mvdr" else n
    return m * (m + 1) // 2 + (m if kind == "mvdr" else 2 * m), m * (m + 1) // 2


def cell_formula(kind, C, env):
    """the cell DESIGN 4.4t's rules give, without the library"""
    sN, fN = state_entries(kind, C)
    ct = C if C in CT_LIST else 0
    regs = ct != 0 and "DSR_ABF_NOREGS" not in env
    lds = (sN + fN) * 16 * 64 <= LDS_GATE and "DSR_ABF_MEMSTATE" not in env
    return (ct, 16 if C <= 16 else 64, REGS if regs else LDS if lds else MEM)


def _case(kind, name, C, expect, env=None, gates=None, T=40, scale=1.0, wp=0, **params):
    p = dict(GJ if kind == "gj" else SMI); p.update(params)
    if kind == "gj":
        if p["staticAfter"] is None:
            p["staticAfter"] = T // 2                           # inside the utterance
        if p["floorSubBandSigmaK"] is None:
            p["floorSubBandSigmaK"] = 1.15 * C                   # about the median of the smoothed |x|^2 of these snapshots
        if p["alpha2"] is None:
            p["alpha2"] = 0.05 if C <= 5 else 0.08 / C           # |wa|^2 of these snapshots falls with the channel count
    return dict(name="%s_%s" % (kind, name), kind=kind, C=C, env=dict(env or {}), expect=tuple(expect), gates=dict(gates or {}), T=T, scale=scale,
                wp=wp, params=p)


CASES = [
    # ---- Griffiths-Jim: n + 1 entries, so the 64 lanes' state always fits LDS (64 channels: 65 536 bytes); memory only through the switch
    _case("gj", "regs4", 4, (4, 16, REGS)),
    _case("gj", "regs6", 6, (6, 16, REGS), wp=25),
    _case("gj", "regs8", 8, (8, 16, REGS)),
    _case("gj", "lds4_noregs", 4, (4, 16, LDS), NOREGS, wp=25),
    _case("gj", "lds6_noregs", 6, (6, 16, LDS), NOREGS),
    _case("gj", "lds8_noregs", 8, (8, 16, LDS), NOREGS),
    _case("gj", "mem4_both", 4, (4, 16, MEM), BOTH),
    _case("gj", "mem6_both", 6, (6, 16, MEM), BOTH),
    _case("gj", "mem8_both", 8, (8, 16, MEM), BOTH, wp=25),
    _case("gj", "lds2", 2, (0, 16, LDS)),
    _case("gj", "lds5", 5, (0, 16, LDS), wp=25),
    _case("gj", "lds16", 16, (0, 16, LDS), gates={"lds": True, "cap16": True}),
    _case("gj", "lds17_cap64", 17, (0, 64, LDS), gates={"lds": True, "cap16": False}),
    _case("gj", "lds64_cap64", 64, (0, 64, LDS), gates={"lds": True, "cap16": False}, T=18, alpha2=3.0e-4),
    _case("gj", "mem5_memstate", 5, (0, 16, MEM), MEMSTATE),
    _case("gj", "mem17_memstate", 17, (0, 64, MEM), MEMSTATE, wp=25),
    # ---- MVDR: C (C + 1) + C entries with the factor: 11 channels 146 432 bytes (inside the gate), 12 channels 172 032
    _case("mvdr", "regs4", 4, (4, 16, REGS), end=0),
    _case("mvdr", "regs6", 6, (6, 16, REGS), wp=40),
    _case("mvdr", "regs8", 8, (8, 16, REGS), end=100),
    _case("mvdr", "regs8_scale", 8, (8, 16, REGS), scale=1.0e3),
    _case("mvdr", "lds4_noregs", 4, (4, 16, LDS), NOREGS, end=100, wp=40),
    _case("mvdr", "lds6_noregs", 6, (6, 16, LDS), NOREGS, end=0),
    _case("mvdr", "lds8_noregs", 8, (8, 16, LDS), NOREGS),
    _case("mvdr", "mem4_both", 4, (4, 16, MEM), BOTH),
    _case("mvdr", "mem6_both", 6, (6, 16, MEM), BOTH, end=100),
    _case("mvdr", "mem8_both", 8, (8, 16, MEM), BOTH, end=0, wp=40),
    _case("mvdr", "lds2", 2, (0, 16, LDS), end=100),
    _case("mvdr", "lds5", 5, (0, 16, LDS)),
    _case("mvdr", "lds11", 11, (0, 16, LDS), gates={"lds": True, "cap16": True}),
    _case("mvdr", "mem12", 12, (0, 16, MEM), gates={"lds": False, "cap16": True}, end=100),
    _case("mvdr", "mem16", 16, (0, 16, MEM), gates={"lds": False, "cap16": True}),
    _case("mvdr", "mem17_cap64", 17, (0, 64, MEM), gates={"lds": False, "cap16": False}),
    _case("mvdr", "mem64_cap64", 64, (0, 64, MEM), gates={"lds": False, "cap16": False}, T=18, end=100),
    _case("mvdr", "mem5_memstate", 5, (0, 16, MEM), MEMSTATE, wp=40),
    # ---- MPDR: n (n + 1) + 2 n entries with the factor (n = C - 1): 11 channels 133 120 bytes, 12 channels 157 696
    _case("mpdr", "regs4", 4, (4, 16, REGS)),
    _case("mpdr", "regs6", 6, (6, 16, REGS), end=100),
    _case("mpdr", "regs8", 8, (8, 16, REGS), end=0),
    _case("mpdr", "lds4_noregs", 4, (4, 16, LDS), NOREGS, end=0),
    _case("mpdr", "lds6_noregs", 6, (6, 16, LDS), NOREGS),
    _case("mpdr", "lds8_noregs", 8, (8, 16, LDS), NOREGS, end=100),
    _case("mpdr", "lds8_noregs_scale", 8, (8, 16, LDS), NOREGS, scale=1.0e3),
    _case("mpdr", "mem4_both", 4, (4, 16, MEM), BOTH, end=100),
    _case("mpdr", "mem6_both", 6, (6, 16, MEM), BOTH, end=0),
    _case("mpdr", "mem8_both", 8, (8, 16, MEM), BOTH),
    _case("mpdr", "lds2", 2, (0, 16, LDS)),                                                       # an order-1 matrix
    _case("mpdr", "lds5", 5, (0, 16, LDS), end=100),
    _case("mpdr", "lds11", 11, (0, 16, LDS), gates={"lds": True, "cap16": True}),
    _case("mpdr", "mem12", 12, (0, 16, MEM), gates={"lds": False, "cap16": True}),
    _case("mpdr", "mem16", 16, (0, 16, MEM), gates={"lds": False, "cap16": True}, end=100),
    _case("mpdr", "mem17_cap64", 17, (0, 64, MEM), gates={"lds": False, "cap16": False}),
    _case("mpdr", "mem64_cap64", 64, (0, 64, MEM), gates={"lds": False, "cap16": False}, T=18),
    _case("mpdr", "mem5_memstate", 5, (0, 16, MEM), MEMSTATE),
]
assert len({c["name"] for c in CASES}) == len(CASES)
# block 1 in registers, block 2 in LDS, block 3 in memory: the carried layout is common to the three residences
CROSS_CASES = [_case("gj", "cross6", 6, (6, 16, REGS)), _case("mvdr", "cross6", 6, (6, 16, REGS), end=100), _case("mpdr", "cross6", 6, (6, 16, REGS), end=100)]
CROSS_ENVS = [({}, REGS), (NOREGS, LDS), (BOTH, MEM)]


def design(C):
    """-> (delays, wq [F][C], B [F][C][C - 1]) as the restatement computes them (calcDelays, calcArrayManifoldVectors of the GSC)"""
    mp = synth.linear_array(C, 25.0)
    delays = A.calcDelays(800.0, 1500.0, 300.0, mp)
    wq, B = A.design(M, C, 16000.0, delays)
    return delays, wq, B


def envelope(T):
    """the on/off envelope over the frames: speech, a pause, speech, a pause"""
    e = np.ones(T); e[T // 4: T // 4 + max(T // 6, 2)] = 0.04; e[(3 * T) // 4:(3 * T) // 4 + max(T // 8, 2)] = 0.04
    return e


def snapshots(case, wq):
    """-> X complex64 [U][C][T][F], rows past an utterance's length zero: a source from the look direction + noise, under the envelope"""
    Cn, T = case["C"], case["T"]
    rng = np.random.default_rng(1900 + Cn + {"gj": 0, "mvdr": 100, "mpdr": 200}[case["kind"]] + (7 if "cross" in case["name"] else 0))
    s = rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))
    d = wq[:F] * Cn                                                               # the look direction: wq^H d = 1
    X = np.stack([s * d[:, c] + 0.7 * (rng.standard_normal((U, T, F)) + 1j * rng.standard_normal((U, T, F))) for c in range(Cn)], axis=1)
    X = (X * envelope(T)[None, None, :, None] * case["scale"]).astype(np.complex64)
    for u, n in enumerate(lens_of(case)):
        X[u, :, n:] = 0
    return X


def post_filter(case):
    """wp [U][wp][F] float32 in (0.2, 1): the post-filter weights of the case's first `wp` frames; None without"""
    if not case["wp"]:
        return None
    return np.random.default_rng(5 + case["C"]).uniform(0.2, 1.0, (U, case["wp"], F)).astype(np.float32)


def run_np(case, Xu, wq, B, wp=None, **kw):
    """the restatement on one utterance Xu [C][n][F]"""
    p = case["params"]
    if case["kind"] == "gj":
        return A.griffiths_jim(Xu, wq, B, M, wp=wp, **p, **kw)
    if case["kind"] == "mvdr":
        return A.smi_mvdr(Xu, wq, wp1L=wp, **p, **kw)
    return A.smi_mpdr(Xu, wq, B, **p, **kw)


_REF = {}


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def reference(case):
    """design, snapshots, post-filter weights and, per utterance on its own length, the restatement and its second evaluation; computed once.
    -> dict(wq, B, X, wp, runs [(ref, alt)], yard_y, yard_w): the yardsticks are the largest difference of the two evaluations over the batch,
    relative to the RMS of the restatement's outputs / final weights"""
    if case["name"] not in _REF:
        _, wq, B = design(case["C"])
        X = snapshots(case, wq); wp = post_filter(case)
        runs = []
        for u, n in enumerate(lens_of(case)):
            w = None if wp is None else wp[u].astype(np.float64)
            runs.append((run_np(case, X[u][:, :n], wq, B, w), run_np(case, X[u][:, :n], wq, B, w, alt=True)))
        Yr = np.concatenate([r["Y"].ravel() for r, _ in runs]); Wr = np.concatenate([r["w"].ravel() for r, _ in runs if len(r["Y"])])
        dy = max([np.abs(r["Y"] - a["Y"]).max() for r, a in runs if len(r["Y"])])
        dw = max([np.abs(r["w"] - a["w"]).max() for r, a in runs if len(r["Y"])])
        X.setflags(write=False)
        _REF[case["name"]] = dict(wq=wq, B=B, X=X, wp=wp, runs=runs, rms_y=rms(Yr), rms_w=rms(Wr), yard_y=dy / rms(Yr), yard_w=dw / rms(Wr))
    return _REF[case["name"]]
