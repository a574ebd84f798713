"""Shapes and synthetic inputs of the maximum-kurtosis beamformer tests (tests/test_mk_np_cpu.py, tests/test_gpu_mk.py).

Inputs: a super-Gaussian target on the look direction, a Gaussian interferer off it and a little sensor noise, seeded, built per bin in the
subband domain: X[c] = d_look[c] s + d_int[c] v + 0.05 e with d[c] = exp(-2 pi i f fs tau_c / fftLen), so that the delay-and-sum vector
wq = d_look / C passes the target with gain 1.  s is a complex Gaussian times a Rayleigh amplitude, v a complex Gaussian of the same power.

The blocking matrix of this toolkit (Gram-Schmidt on I - conj(d) d^T / |d|^2, the reference's) is orthogonal to conj(wq); only where wq is real
-- a broadside look direction -- does it block the target exactly.  The cases look at 70 degrees (the general situation: the active weights
also change the target's gain); the test of the interferer's power looks broadside, where the target's gain stays 1."""
import numpy as np

from tests import mk_np

FS = 16000.0
LOOK_DEG, INTERFERER_DEG = 70.0, 130.0


def delays(C, deg):
    return np.arange(C) * 0.04 * np.cos(np.deg2rad(deg)) / 343.0


def steering(fftLen, C, deg):
    """[F][C]"""
    F = fftLen // 2 + 1
    return np.exp(-2j * np.pi * np.arange(F)[:, None] * FS * delays(C, deg)[None, :] / fftLen)


def fixed_weights(fftLen, C, look=LOOK_DEG):
    """wq [F][C] (delay and sum on the look direction), B [F][C][C-1]"""
    wq = steering(fftLen, C, look) / C
    B = np.stack([mk_np.blocking_matrix([complex(w) for w in wq[f]]) for f in range(wq.shape[0])])
    return np.ascontiguousarray(wq), np.ascontiguousarray(B)


def observations(U, C, T, fftLen, seed, parts=False, look=LOOK_DEG):
    """X [U][C][T][F] complex64 (with parts: the target and interferer images too, same shape, complex128)"""
    rng = np.random.default_rng(seed); F = fftLen // 2 + 1

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    s = cn(U, T, F) * np.abs(cn(U, T, F))                            # a Gaussian with a Rayleigh amplitude on top: heavier tails than a Gaussian
    v = cn(U, T, F)
    dl, di = steering(fftLen, C, look), steering(fftLen, C, INTERFERER_DEG)
    tgt = s[:, None, :, :] * dl.T[None, :, None, :]; itf = v[:, None, :, :] * di.T[None, :, None, :]
    X = (tgt + itf + 0.05 * cn(U, C, T, F)).astype(np.complex64)
    return (X, tgt, itf) if parts else X


# name: (fftLen, C, T, sFrame, eFrame, R); every case has U = 3 with nframes (T, 0, (T + 1) // 2).  T = 63, 64, 65 sit on the edge of the 64
# partial sums, C = 4, 6, 8 are the compile-time instantiations, 2, 3 and 64 run the run-time one (64: the largest, gradient in eight passes).
CASES = {
    "c2_t1":     (8, 2, 1, 0, 1000, 1),
    "c4_t63":    (8, 4, 63, 0, 1000, 1),
    "c8_t64":    (32, 8, 64, 0, 1000, 1),
    "c8_t65":    (8, 8, 65, 0, 1000, 1),
    "c4_t200_r2": (32, 4, 200, 3, 190, 2),
    "c6_t200":   (8, 6, 200, 5, 1000, 1),
    "c2_t200_r2": (8, 2, 200, 1, 1000, 2),
    "c3_t65":    (8, 3, 65, 0, 1000, 1),
    "c64_t65":   (8, 64, 65, 0, 1000, 1),
}
STEP5_CASES = ("c4_t63", "c8_t65", "c4_t200_r2", "c3_t65")          # STEPSIZE 5.0: the first trial fails
U = 3


# cases named for a branch of the minimisers: name -> (case, kind, u, f, start, settings, branch or None, exit reason or None).  start: "zero",
# "rand" (0.1 x seeded normal), "big" (3 x seeded normal: beyond |gamma|), "nan"; "zeroX" as the case means all-zero observations.
BRANCH_CASES = {
    "failed_trial":         ("c4_t63", mk_np.NRM, 0, 0, "zero", dict(STEPSIZE=5.0), "failed_trial", None),
    "intermediate_retry":   ("c4_t63", mk_np.PR, 0, 0, "zero", dict(STEPSIZE=5.0), "intermediate_retry", None),
    "conjugate_restart":    ("c2_t200_r2", mk_np.PR, 0, 1, "rand", dict(DIFFSTOPTOLERANCE=0.0, STOPTOLERANCE=0.0, MAXITNS=4), "restart", mk_np.MAXIT),
    "norm_clipping":        ("c8_t65", mk_np.NRM, 0, 3, "big", dict(), "clip", None),
    "exit_max_iterations":  ("c4_t63", mk_np.NRM, 0, 1, "zero", dict(MAXITNS=2), None, mk_np.MAXIT),
    "exit_gradient":        ("c4_t63", mk_np.PR, 0, 1, "zero", dict(STOPTOLERANCE=1.0e3), None, mk_np.GRADIENT),
    "exit_difference":      ("c4_t63", mk_np.NRM, 0, 1, "zero", dict(DIFFSTOPTOLERANCE=1.0e-2, STOPTOLERANCE=0.0), None, mk_np.DIFFERENCE),
    "exit_no_progress":     ("zeroX", mk_np.PR, 0, 1, "zero", dict(), None, mk_np.NO_PROGRESS),
    "exit_skipped_empty":   ("c4_t63", mk_np.PR, 1, 1, "zero", dict(), None, mk_np.SKIPPED),
    "exit_skipped_nan":     ("c4_t63", mk_np.NRM, 0, 1, "nan", dict(), None, mk_np.SKIPPED),
}


def branch_inputs(name):
    case, kind, u, f, start, settings, branch, reason = BRANCH_CASES[name]
    inp = case_inputs("c4_t63" if case == "zeroX" else case)
    if case == "zeroX":
        inp["X"] = np.zeros_like(inp["X"])
    n2 = 2 * (inp["C"] - 1); rng = np.random.default_rng(77)
    x0 = {"zero": np.zeros(n2), "rand": 0.1 * rng.standard_normal(n2), "big": 3.0 * rng.standard_normal(n2), "nan": np.full(n2, np.nan)}[start]
    return inp, kind, u, f, x0, settings, branch, reason


def nframes_of(T):
    return np.array([T, 0, (T + 1) // 2], np.int32)


def case_inputs(name):
    fftLen, C, T, sF, eF, R = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    X = observations(U, C, T, fftLen, seed)
    wq, B = fixed_weights(fftLen, C)
    return dict(fftLen=fftLen, C=C, T=T, sFrame=sF, eFrame=eF, R=R, X=X, wq=wq, B=B, nframes=nframes_of(T), F=fftLen // 2 + 1)


def problem(cls, kind, inp, u, f, prev=(0.0, 0.0, 0.0), X=None, **over):
    """the (u, f) problem of a case as a mk_np problem object of class cls"""
    X = inp["X"] if X is None else X
    sel = mk_np.select_frames(inp["sFrame"], inp["eFrame"], inp["R"], int(inp["nframes"][u]), X.shape[2])
    d = dict(mk_np.DEFAULTS[kind]); d.update(over)
    Xf = np.ascontiguousarray(X[u][:, sel, :][:, :, f].T) if sel else np.zeros((0, inp["C"]), X.dtype)      # [Tsel][C]
    return cls(kind, Xf, inp["wq"][f], inp["B"][f], d["alpha"], d["beta"], d["gamma"], prev)
