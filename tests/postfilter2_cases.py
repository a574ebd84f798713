"""Cases shared by test_postfilter2_np_cpu.py and test_gpu_postfilter2.py (as gcc_cases.py does for the GCC family): the inputs, the block
structure of the carried runs, and the restatement driven through them."""
import numpy as np

from tests import postfilter2_np as P


def snapshots(seed, shape, scale=1.0):
    """complex64 snapshots with a speech-like spread of magnitudes over frames; a few exact zeros (a zero bin has a defined output, :119)"""
    r = np.random.default_rng(seed)
    x = (r.standard_normal(shape) + 1j * r.standard_normal(shape)) * scale * (0.2 + r.random(shape[:-1] + (1,)) * 2.0)
    x = x.astype(np.complex64)
    x.reshape(-1)[r.integers(0, x.size, size=3)] = 0
    return x


# --- spectral subtraction: three blocks.  1: training, no subtraction.  stopTraining + startNoiseSubtraction.  2: subtraction only.
#     startTraining.  3: both at once (the recursive channels go on learning, and the current frame is inside the estimate subtracted from it).
#     nframes per block and utterance: ragged, with 0 and 1 (block 1 keeps >= 1 frame where a channel averages, or stopTraining would refuse).
SS_CASES = [
    dict(name="M64_c1_avg", M=64, alphas=[-1.0], ft=1.0, floor=0.001, T=6, nframes=[[6, 1], [6, 0], [3, 6]], seed=1),
    dict(name="M256_c3_mixed", M=256, alphas=[-1.0, 0.9, 0.5], ft=1.5, floor=0.01, T=7, nframes=[[7, 2, 1], [0, 7, 1], [7, 7, 0]], seed=2),
    dict(name="M512_c8_rec", M=512, alphas=[0.8] * 8, ft=0.7, floor=0.001, T=5, nframes=[[5, 0], [1, 5], [5, 5]], seed=3),
    dict(name="M256_c2_over", M=256, alphas=[-1.0, -1.0], ft=4.0, floor=0.5, T=8, nframes=[[8], [8], [8]], seed=4),
]


def ss_input(c):
    U = len(c["nframes"][0])
    return [snapshots(c["seed"] * 100 + b, (U, len(c["alphas"]), c["T"], c["M"] // 2 + 1)) for b in range(3)]


def ss_reference(c, full=False):
    """-> per block the outputs [U][T][F or M] (rows past nframes zero) and, at the end, the estimates [U][C][F]"""
    X = ss_input(c); U = X[0].shape[0]; M = c["M"]; nb = M if full else M // 2 + 1
    outs = [np.zeros((U, c["T"], nb), np.complex128) for _ in range(3)]; est = []
    for u in range(U):
        s = P.SpectralSubtractor(M, c["ft"], c["floor"])
        for a in c["alphas"]:
            s.setChannel(a)
        for b in range(3):
            if b == 1:
                s.stopTraining(); s.subtract = True
            if b == 2:
                s.training = True
            n = c["nframes"][b][u]
            if n:
                outs[b][u, :n] = s.run(X[b][u][:, :n].astype(np.complex128), full)
        est.append(np.array([p.est for p in s.psd]))
    return outs, np.array(est)


# --- Wiener: blocks with the noise update switched; block 2 runs with updating stopped
WIENER_CASES = [
    dict(name="M64_a0", M=64, alpha=0.0, floor=0.001, beta=1.0, T=5, nframes=[[5, 1], [5, 0], [2, 5]], seed=11),
    dict(name="M256_a06", M=256, alpha=0.6, floor=0.01, beta=2.5, T=6, nframes=[[6, 1, 0], [3, 6, 6], [6, 0, 1]], seed=12),
    dict(name="M512_a09", M=512, alpha=0.9, floor=0.001, beta=0.3, T=4, nframes=[[1], [4], [4]], seed=13),
]


def wiener_input(c):
    U = len(c["nframes"][0]); F = c["M"] // 2 + 1
    return [(snapshots(c["seed"] * 100 + b, (U, c["T"], F)), snapshots(c["seed"] * 100 + 50 + b, (U, c["T"], F), 0.3)) for b in range(3)]


def wiener_reference(c):
    """carried over the three blocks -> outputs per block [U][T][F], final (PSDs, PSDn, frames) per utterance"""
    X = wiener_input(c); U = X[0][0].shape[0]; F = c["M"] // 2 + 1
    outs = [np.zeros((U, c["T"], F), np.complex128) for _ in range(3)]; fin = []
    for u in range(U):
        w = P.WienerFilter(c["M"], c["alpha"], c["floor"], c["beta"])
        for b in range(3):
            w.update = b != 1
            n = c["nframes"][b][u]
            if n:
                outs[b][u, :n] = w.run(X[b][0][u, :n], X[b][1][u, :n])
        fin.append((w.PSDs.copy(), w.PSDn.copy(), w.frames))
    return outs, fin


# --- masks: two blocks, carried; per-bin thresholds are set (twice: the first call only allocates) before block 2 where perbin is on
MASK_CASES = [
    dict(name="kim_M64_L", kind=1, chanX=0, M=64, threshold=2.0, alpha=0.0, dEta=0.01, perbin=False, T=6, nframes=[[6, 1], [0, 6]], seed=21),
    dict(name="kim_M256_R", kind=1, chanX=1, M=256, threshold=5.0, alpha=0.7, dEta=0.05, perbin=True, T=7, nframes=[[7, 0, 1], [7, 7, 3]], seed=22),
    dict(name="iid_M512_L", kind=2, chanX=0, M=512, threshold=0.2, alpha=0.5, dEta=0.01, perbin=False, T=5, nframes=[[5, 1], [5, 0]], seed=23),
    dict(name="iid_M256_R_bins", kind=2, chanX=1, M=256, threshold=-0.1, alpha=0.3, dEta=0.1, perbin=True, T=6, nframes=[[6, 2], [1, 6]], seed=24),
    dict(name="base_M64", kind=0, chanX=0, M=64, threshold=0.0, alpha=0.0, dEta=0.01, perbin=False, T=3, nframes=[[3], [3]], seed=25),
]


def mask_input(c):
    U = len(c["nframes"][0]); F = c["M"] // 2 + 1
    return [(snapshots(c["seed"] * 100 + b, (U, c["T"], F)), snapshots(c["seed"] * 100 + 50 + b, (U, c["T"], F), 0.8)) for b in range(2)]


def mask_thresholds(c):
    return np.linspace(-0.3, 0.4, c["M"] // 2 + 1) + 1.0 / 3.0


def mask_reference(c, full=False):
    """-> per block (out, mu, sideA, sideB) with [U][T][...] arrays, final prevMu [U][F]"""
    X = mask_input(c); U = X[0][0].shape[0]; M = c["M"]; F = M // 2 + 1; nb = M if full else F
    res = [dict(out=np.zeros((U, c["T"], nb), np.complex128), mu=np.zeros((U, c["T"], F), np.float32), a=np.zeros((U, c["T"], F)), b=np.ones((U, c["T"], F)))
           for _ in range(2)]
    prev = []
    for u in range(U):
        m = P.MaskFilter(c["kind"], c["chanX"], M, c["threshold"], c["alpha"], c["dEta"])
        for b in range(2):
            if b == 1 and c["perbin"]:
                m.setThresholds(mask_thresholds(c)); m.setThresholds(mask_thresholds(c))
            n = c["nframes"][b][u]
            if n:
                o, mu, (A, B) = m.run(X[b][0][u, :n], X[b][1][u, :n], full)
                res[b]["out"][u, :n] = o; res[b]["mu"][u, :n] = mu; res[b]["a"][u, :n] = A; res[b]["b"][u, :n] = B
        prev.append(m.prevMu.copy())
    return res, np.array(prev)


# --- estimators: two blocks added into the same accumulators.  scale: IID/FDIID magnitudes comparable with the threshold range.
EST_CASES = [
    dict(name="kim_builtin_M256", kind=0, M=256, rng=(0.0, 0.0, 0.02), band=(-1, -1, -1), dEta=0.01, pc=1.0 / 15, T=6, nframes=[[6, 1], [0, 6]], scale=1.0, seed=31),
    dict(name="kim_explicit_M64_band", kind=0, M=64, rng=(0.5, 20.0, 0.25), band=(1000.0, 6000.0, 16000), dEta=0.05, pc=0.5, T=8, nframes=[[8, 3], [8, 8]], scale=1.0, seed=32),
    dict(name="kim_degenerate_M64", kind=0, M=64, rng=(0.5, 8.0, 0.5), band=(-1, -1, -1), dEta=0.01, pc=0.0, T=4, nframes=[[4], [4]], scale=1.0, seed=33),
    dict(name="iid_builtin_M256", kind=1, M=256, rng=(0.0, 0.0, 0.02), band=(-1, -1, -1), dEta=0.01, pc=1.0 / 15, T=5, nframes=[[5, 1], [5, 0]], scale=4.0, seed=34),
    dict(name="iid_explicit_M512_band", kind=1, M=512, rng=(-3.0, 3.0, 0.125), band=(500.0, 4000.0, 16000), dEta=0.1, pc=0.5, T=6, nframes=[[6], [2]], scale=2.0, seed=35),
    dict(name="iid_degenerate_M64", kind=1, M=64, rng=(-1.0, 1.0, 0.25), band=(-1, -1, -1), dEta=0.01, pc=0.0, T=3, nframes=[[3], [3]], scale=1.0, seed=36),
    dict(name="fdiid_builtin_M64", kind=2, M=64, rng=(0.0, 0.0, 1000.0), band=(-1, -1, -1), dEta=0.01, pc=1.0 / 15, T=40, nframes=[[40, 1], [0, 40]], scale=3000.0, seed=37),
    dict(name="fdiid_explicit_M256", kind=2, M=256, rng=(-2.0, 2.0, 0.01), band=(-1, -1, -1), dEta=0.05, pc=0.5, T=30, nframes=[[30], [7]], scale=1.5, seed=38),
]


def est_input(c):
    U = len(c["nframes"][0]); F = c["M"] // 2 + 1
    return [(snapshots(c["seed"] * 100 + b, (U, c["T"], F), c["scale"]), snapshots(c["seed"] * 100 + 50 + b, (U, c["T"], F), 0.8 * c["scale"])) for b in range(2)]


def est_new(c):
    return P.ThresholdEstimator(c["kind"], c["M"], c["rng"][0], c["rng"][1], c["rng"][2], c["band"][0], c["band"][1], c["band"][2], c["dEta"], c["pc"])


_EST_CACHE = {}


def est_reference(c):
    """-> list over utterances of the restatement's estimator after both blocks (cached: the literal loops are slow)"""
    if c["name"] not in _EST_CACHE:
        X = est_input(c); U = X[0][0].shape[0]; out = []
        for u in range(U):
            e = est_new(c)
            for b in range(2):
                n = c["nframes"][b][u]
                e.run(X[b][0][u, :n].astype(np.complex128), X[b][1][u, :n].astype(np.complex128))
            out.append(e)
        _EST_CACHE[c["name"]] = out
    return _EST_CACHE[c["name"]]


def est_terms(c, e):
    """n of the accumulator bound: the (frame, bin) terms behind one accumulator entry.  Kim: every entry sums one R per frame, each R from a
    sum over the band's bins.  IID: every entry belongs to one side and sums one term per band bin and frame.  FDIID: an entry belongs to one
    bin and sums the T and the I term of every frame."""
    return 2 * e.nSamples if c["kind"] == 2 else (e.f1 - e.f0) * e.nSamples


# The pow() term of the accumulator bound.  Measured on the first GPU run: an accumulator entry that is a single term (one bin, one frame)
# differs from numpy's by at most 1.37e-15 = 12.3 x 2^-53 (terms up to the fourth power of a pow() result), and the largest accumulator error of
# the cases below was 1.08e-15 against a smallest 4 n 2^-53 of 3.3e-14.  The pow() difference disappears inside the summation bound of every
# case, so no term is added for it.
POW_DIFF = 0.0


def acc_bound(n):
    """sums of n non-negative fp64 terms in another order: 4 n 2^-53 relative, plus the measured pow() difference"""
    return 4.0 * n * 2.0 ** -53 + POW_DIFF
