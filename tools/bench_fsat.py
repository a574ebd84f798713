#!/usr/bin/env python
"""Time fast speaker-adaptive training on the GPU: tools/bench_fsat.py [--shape S,G,D,leaves]... [--steps 5] [--warmup 2] [--out FILE]

One JSON line per shape, the shapes of tools/bench_sat.py (S speaker slots in one batch, G Gaussians of dimension D spread evenly over `leaves`
regression classes, every slot one MLLR transform per class, one block D x D):
  ms_norm_call / ms_acc_call   the whole dsr_fsat_norm / dsr_fsat_accumulate (tables built and uploaded, kernel, synchronised), median of --steps
  ms_norm        k_fsat_norm (events inside the library);  gbs_norm: the 2 S G D doubles of sumO and sumOsq, which it reads once, over ms_norm
  ms_mat_acc     the matrix-only k_sat_mean_acc;  tflops_mat: 2 D (D (D + 1) / 2) G S useful fp64 flop (the upper triangle of mat) over it
  ms_solve       k_fsat_solve;  solves_per_s: G eigen-solves of order D over it;  ms_update: the whole dsr_fsat_update
  ms_two_pass_acc / ms_two_pass_update   what this replaces, on the same shape: k_sat_mean_acc + k_sat_var_acc, and the mean update of
                 dsr_sat_update(1) -- reported as the yardstick, not asserted (the variance update of the two-pass path is host arithmetic)"""
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
    dsr.load()
    med = lambda v: sorted(v)[len(v) // 2]                                            # noqa: E731
    lines = []
    for S, G, D, L in shapes:
        assert L >= 1 and L & (L - 1) == 0 and G % 16 == 0
        gm = synth.gmm_model(G // 16, 16, D, seed=12)
        classes = (L + np.arange(G) % L).astype(np.uint16)
        rng = np.random.default_rng(3)
        A = np.eye(D)[None, None] + 0.1 * rng.standard_normal((S, L, D, D)) / np.sqrt(D); b = 0.3 * rng.standard_normal((S, L, D))
        c = rng.uniform(5.0, 50.0, (S, G)).astype(np.float32).astype(np.float64)
        mu = gm["mean"].astype(np.float64)

        def handle(cls, *args):
            g = dsr.Gmm(**gm); g.set_reg_classes(classes); tr = dsr.Trainer(g); h = cls(tr, S, *args); h.set_timing(True)
            return g, tr, h
        g, tr, h = handle(dsr.FastSat, 0.0, 1.0); g2, tr2, h2 = handle(dsr.Sat, 1.0)
        for s in range(S):
            y = np.einsum("gpq,gq->gp", A[s][classes - L], mu) + b[s][classes - L]; sumO = c[s][:, None] * y; sumOsq = c[s][:, None] * (1.0 + y * y)
            for l in range(L):
                h.set_transform(s, L + l, dsr.SAT_MLLR, A[s, l], b[s, l]); h2.set_transform(s, L + l, dsr.SAT_MLLR, A[s, l], b[s, l])
            h.set_stats(s, count=c[s], den=np.zeros(G), sumO=sumO, sumOsq=sumOsq); h2.set_stats(s, c=c[s], sumO=sumO, sumOsq=sumOsq)
        wn, wa, wu, kn, ka, ks, k2, u2 = [], [], [], [], [], [], [], []
        for i in range(a.warmup + a.steps):
            h.zero(); h.zero_fast(); torch.cuda.synchronize()
            t0 = time.perf_counter(); h.norm(S); dn = (time.perf_counter() - t0) * 1e3
            h.add_fast()
            t0 = time.perf_counter(); h.accumulate(S); da = (time.perf_counter() - t0) * 1e3
            ms = h.kernel_ms()
            if i == a.warmup + a.steps - 1:                                                   # one update: it changes the model the next fold would read
                t0 = time.perf_counter(); r = h.update(); du = (time.perf_counter() - t0) * 1e3; wu.append(du); ks.append(h.kernel_ms()[2])
            h2.zero(); h2.accumulate(dsr.SAT_MEAN, S); h2.accumulate(dsr.SAT_VARIANCE, S); m2 = h2.kernel_ms()
            if i >= a.warmup:
                wn.append(dn); wa.append(da); kn.append(ms[0]); ka.append(ms[1]); k2.append(m2[0] + m2[1])
        t0 = time.perf_counter(); h2.update(dsr.SAT_MEAN); u2.append((time.perf_counter() - t0) * 1e3)
        recovered = float(np.abs(g.params()["mean"].astype(np.float64) - mu).max())
        lines.append(dict(tool="bench_fsat", S=S, G=G, dimN=D, leaves=L, ms_norm_call=round(med(wn), 3), ms_acc_call=round(med(wa), 3), ms_norm=round(med(kn), 3),
                          gbs_norm=round(2.0 * S * G * D * 8 / (med(kn) * 1e-3) / 1e9, 1), ms_mat_acc=round(med(ka), 3),
                          tflops_mat=round(2.0 * D * (D * (D + 1) / 2) * G * S / (med(ka) * 1e-3) / 1e12, 3), ms_solve=round(med(ks), 3),
                          solves_per_s=round(G / (med(ks) * 1e-3)), ms_update=round(med(wu), 3), ms_two_pass_acc=round(med(k2), 3),
                          ms_two_pass_update=round(med(u2), 3), max_abs_mean_error=recovered, updated=r["totals"][1]))
        del h, tr, g, h2, tr2, g2
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
