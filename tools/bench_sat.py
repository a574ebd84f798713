#!/usr/bin/env python
"""Time speaker-adaptive training on the GPU: tools/bench_sat.py [--shape S,G,D,leaves]... [--steps 5] [--warmup 2] [--out FILE]

One JSON line per shape (S speaker slots in one batch, G Gaussians of dimension D spread evenly over `leaves` regression classes, a power of
two: the classes are the nodes leaves .. 2 leaves - 1 of a complete tree; every slot holds one MLLR transform per class, one block D x D):
  ms_mean_call / ms_var_call   the whole dsr_sat_accumulate (tables built and uploaded, kernel, synchronised), median of --steps calls
  ms_mean_acc    k_sat_mean_acc (events inside the library);  ms_var_acc: k_sat_var_acc;  ms_solve: k_sat_solve;  ms_update: the whole mean
                 update (occupancies pulled, solve, records and means pulled, the model's device copies rebuilt)
  tflops_mean    2 D (D (D + 1) / 2 + D) G S fp64 flop over ms_mean_acc: the useful flop of the contraction (the upper triangle of mat, and
                 vec); the scalar and occupancy sums are in the time, not in the count
  solves_per_s   G symmetric eigen-solves of order D over ms_solve
  ms_torch_mean / ms_torch_solve   the same mat and vec by torch.einsum in fp64 (full matrices, class by class) and the solves by
                 torch.linalg.pinv(rcond = 1e-7, hermitian) @ vec -- yardsticks, not reference results"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import torch
    import dsr._capi as dsr
    from tests import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="S,G,D,leaves")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in (a.shape or ["1,4096,39,1", "32,4096,39,4", "128,4096,39,8"])]
    dsr.load(); dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]                                            # noqa: E731
    lines = []
    for S, G, D, L in shapes:
        assert L >= 1 and L & (L - 1) == 0 and G % 16 == 0
        gm = synth.gmm_model(G // 16, 16, D, seed=12); g = dsr.Gmm(**gm)
        classes = (L + np.arange(G) % L).astype(np.uint16); g.set_reg_classes(classes)
        rng = np.random.default_rng(3)
        A = np.eye(D)[None, None] + 0.1 * rng.standard_normal((S, L, D, D)) / np.sqrt(D); b = 0.3 * rng.standard_normal((S, L, D))
        c = rng.uniform(5.0, 50.0, (S, G)).astype(np.float32).astype(np.float64)
        mu = gm["mean"].astype(np.float64)
        tr = dsr.Trainer(g); h = dsr.Sat(tr, S, 1.0); h.set_timing(True)
        sumO = np.empty((S, G, D))
        for s in range(S):
            y = np.einsum("gpq,gq->gp", A[s][classes - L], mu) + b[s][classes - L]; sumO[s] = c[s][:, None] * y
            for l in range(L):
                h.set_transform(s, L + l, dsr.SAT_MLLR, A[s, l], b[s, l])
            h.set_stats(s, c=c[s], sumO=sumO[s], sumOsq=c[s][:, None] * (1.0 + y * y))
        wm, wv, wu, km, kv, ks = [], [], [], [], [], []
        for i in range(a.warmup + a.steps):
            h.zero(); torch.cuda.synchronize()
            t0 = time.perf_counter(); h.accumulate(dsr.SAT_MEAN, S); dm = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter(); h.accumulate(dsr.SAT_VARIANCE, S); dv = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter(); r = h.update(dsr.SAT_MEAN); du = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                ms = h.kernel_ms(); wm.append(dm); wv.append(dv); wu.append(du); km.append(ms[0]); kv.append(ms[1]); ks.append(ms[2])
        mat, vec, scalar, occ, has = h.mean_accus(); ms_update, ms_solve = med(wu), med(ks)
        recovered = float(np.abs(g.params()["mean"].astype(np.float64) - mu).max())
        # torch yardsticks
        cd = torch.from_numpy(c).to(dev); iv = torch.from_numpy(gm["ivar"]).to(dev).double(); Ad = torch.from_numpy(A).to(dev)
        v1 = torch.from_numpy(sumO - c[:, :, None] * b[:, classes - L]).to(dev)
        sel = [torch.from_numpy(np.nonzero(classes == L + l)[0]).to(dev) for l in range(L)]

        def torch_mean():
            Ms, Vs = [], []
            for l, ix in enumerate(sel):
                w = cd[:, ix, None] * iv[None, ix]                                     # [S][g][D]
                Ms.append(torch.einsum("sgm,smp,smq->gpq", w, Ad[:, l], Ad[:, l])); Vs.append(torch.einsum("sgm,smp->gp", v1[:, ix] * iv[None, ix], Ad[:, l]))
            return Ms, Vs

        def torch_solve(Ms, Vs):
            return [(torch.linalg.pinv(M, rcond=1e-7, hermitian=True) @ V[..., None])[..., 0] for M, V in zip(Ms, Vs)]
        Ms, Vs = torch_mean(); torch_solve(Ms, Vs); torch.cuda.synchronize()
        t1, t2 = [], []
        for _ in range(max(2, a.steps // 2)):
            t0 = time.perf_counter(); Ms, Vs = torch_mean(); torch.cuda.synchronize(); t1.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); X = torch_solve(Ms, Vs); torch.cuda.synchronize(); t2.append((time.perf_counter() - t0) * 1e3)
        ix0 = sel[0].cpu().numpy(); M0 = Ms[0].cpu().numpy()
        mat_vs_torch = float(np.abs(mat[ix0, 0] - M0).max() / np.abs(M0).max())
        flop = 2.0 * D * (D * (D + 1) / 2 + D) * G * S
        lines.append(dict(tool="bench_sat", S=S, G=G, dimN=D, leaves=L, ms_mean_call=round(med(wm), 3), ms_var_call=round(med(wv), 3), ms_mean_acc=round(med(km), 3),
                          ms_var_acc=round(med(kv), 3), ms_update=round(ms_update, 3), ms_solve=round(ms_solve, 3),
                          tflops_mean=round(flop / (med(km) * 1e-3) / 1e12, 3), solves_per_s=round(G / (ms_solve * 1e-3)),
                          ms_torch_mean=round(med(t1), 3), ms_torch_solve=round(med(t2), 3), rel_mat_diff_vs_torch=mat_vs_torch,
                          max_abs_mean_error=recovered, updated=r["totals"][1]))
        del h, tr, g, cd, v1, Ms, Vs, X, Ad
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
