#!/usr/bin/env python3
"""Maximum-negentropy beamformer micro benchmark: --shape U,C,T,fftLen (default 8,8,500,512), both reference classes (beta 0.5 and 1.0) at the
reference's defaults, per-bin shape parameters spread over [0.2, 1.2].
Reports ms per estimate (prepare + minimise kernels), ms of a call that prepares and evaluates once, their difference (the minimiser proper),
evaluations per second and the share of problems per exit reason.
Yardstick: the same number of cost-and-gradient evaluations per problem (the mean over the problems) as ONE batched fp64 torch expression
(torch.pow / torch.log) over all U x F problems on the same device, y0 and Z prepared once outside the timed part.
For ggd_accumulate: ms of one pass over the beamformed output [U][T][F] and GB/s on its samples (8 bytes each)."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "distantspeechrecognition-mirror_amd"))
import torch
import dsr._capi as dsr
import dsr._mn as mn
from tests import mk_cases
ap = argparse.ArgumentParser(); ap.add_argument("--shape", default="8,8,500,512"); ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
U, Cn, T, fftLen = [int(v) for v in a.shape.split(",")]; F = fftLen // 2 + 1; n = Cn - 1
dsr.load(); dev = torch.device("cuda:0")
X = torch.from_numpy(mk_cases.observations(U, Cn, T, fftLen, seed=1)).to(dev)
bf = dsr.Beamformer(fftLen, Cn); bf.calcGSCWeights(mk_cases.FS, mk_cases.delays(Cn, mk_cases.LOOK_DEG))
NAMES = ["max_iterations", "gradient", "difference", "no_progress", "eval_cap", "skipped"]
shape = np.linspace(0.2, 1.2, F)


def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps


out = dict(shape=[U, Cn, T, fftLen], path=dsr.mk_path(Cn, T))
for beta, name in ((mn.MN_BETA_PR, "pr"), (mn.MN_BETA_NRM, "nrm")):
    b = mn.MnBeamformer(fftLen, Cn, shape, beta=beta); b.setFixedWeightsFromBeamformer(bf)
    wa, info, cost = b.estimate(X); info = info.cpu().numpy()
    ms = timed(lambda: b.estimate(X))
    zero = torch.zeros((U, F, n), dtype=torch.complex128, device=dev)
    ms_one = timed(lambda: b.eval(X, zero))
    evals = int(info[..., 1].sum()); mean_evals = evals / (U * F)
    # the yardstick: one evaluation of every problem as a batched fp64 expression
    wq, B = [torch.from_numpy(v).to(dev) for v in b.getFixedWeights()]
    Bc, Ng, lB = [torch.from_numpy(v).to(dev)[None, :] for v in b.getConstants()]
    fs = torch.from_numpy(shape).to(dev)[None, :]
    Xd = X.to(torch.complex128)
    y0 = torch.einsum("fc,uctf->uft", wq.conj(), Xd); Z = torch.einsum("fcj,uctf->uftj", B.conj(), Xd)
    w = wa.clone()

    def sweep():
        Y = y0 - torch.einsum("ufj,uftj->uft", w.conj(), Z)
        y2 = (Y.real * Y.real + Y.imag * Y.imag)
        p = torch.pow(y2, fs[..., None])
        s2 = y2.mean(-1); sf = p.mean(-1)
        q = Z * Y.conj()[..., None]
        costv = -((torch.log(s2) + 2.1447298858494) - beta * (Ng + torch.log(fs * sf) / fs - lB)) + b.alpha * (w.real ** 2 + w.imag ** 2).sum(-1)
        dJ = -q.mean(2) / s2[..., None] + beta * ((p / y2)[..., None] * q).mean(2) / sf[..., None]
        return costv, -dJ + b.alpha * w
    ms_sweep = timed(sweep)
    share = {NAMES[r]: float((info[..., 3] == r).mean()) for r in range(6) if (info[..., 3] == r).any()}
    out[name] = dict(ms_estimate=ms, ms_prepare_and_one_evaluation=ms_one, ms_minimise=ms - ms_one, evaluations=evals, evaluations_per_problem=mean_evals,
                     evaluations_per_second=evals / (ms * 1e-3), exit_share=share, torch_ms_per_batched_evaluation=ms_sweep,
                     torch_ms_same_evaluations=ms_sweep * mean_evals, ratio_torch_over_device=ms_sweep * mean_evals / ms)
Y = b.apply(X, wa)
p0, sa0 = np.full(F, 0.7), np.full(F, 1.0)
ms_acc = timed(lambda: mn.ggd_accumulate(Y, p0, sa0))
out["ggd_accumulate"] = dict(ms=ms_acc, samples=U * T * F, GBps=U * T * F * 8 / (ms_acc * 1e-3) / 1e9)
print(json.dumps(out))
