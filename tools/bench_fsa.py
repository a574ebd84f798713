#!/usr/bin/env python
"""Time feature-space adaptation on the GPU: tools/bench_fsa.py [--shape S,T,D]... [--iterN 10] [--steps 5] [--warmup 2] [--out FILE]

One JSON line per shape (S speakers, one accumulator and one transformation each, T frames of dimension D per speaker, every frame one item;
the model has 64 codebooks of 16 Gaussians):
  ms_accumulate  the whole dsr_fsa_accumulate of the S T items (host sort, uploads, kernels, the sums added on the host), median of --steps calls
  ms_nearest     k_fsa_nearest (events inside the library);  ms_stats: k_fsa_stats + k_fsa_reduce;  ms_eig: k_fsa_eig;  ms_rows: k_fsa_rows
                 of one dsr_fsa_estimate over the S pairs with --iterN sweeps;  ms_apply: k_fsa_apply over the S T frames with per-row transforms
  tflops_stats   2 D ((D + 1)(D + 2) / 2 + D + 1) S T fp64 flop over ms_stats (the useful flop of the contraction)
  estimates_per_s  S over ms_eig + ms_rows
  apply_gbps     S T D (4 + 4) bytes of frames read and written over ms_apply (the transforms stay in cache)
  ms_torch_stats the same statistics by torch.einsum in fp64 given the Gaussian of every item -- a yardstick, not a reference result"""
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
    from tests import fsa_np
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="S,T,D")
    ap.add_argument("--iterN", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in (a.shape or ["1,2000,39", "8,2000,39", "32,2000,39"])]
    dsr.load(); dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]                                            # noqa: E731
    lines = []
    for S, T, D in shapes:
        K, R = 64, 16
        m = fsa_np.synth_model(K, R, D, seed=12); g = dsr.Gmm(**m)
        xs, ds = [], []
        for s in range(S):
            x, dist, _ = fsa_np.synth_speaker(m, T, seed=100 + s); xs.append(x); ds.append(dist)
        x = np.concatenate(xs); dist = np.concatenate(ds); N = S * T
        frame = np.arange(N, dtype=np.int32); accu = np.repeat(np.arange(S, dtype=np.int32), T); gamma = np.ones(N, np.float32)
        xd = torch.from_numpy(x).to(dev); trd = torch.from_numpy(accu).to(dev)
        h = dsr.Fsa(g, nAccu=S, nTran=S); h.add_all(); h.set_timing(True)
        wall, near, st, eig, rows, app = [], [], [], [], [], []
        pairs = list(range(S))
        for i in range(a.warmup + a.steps):
            for s in range(S):
                h.zero(s); h.clear(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); h.accumulate(xd, frame, dist, gamma, accu); dt = (time.perf_counter() - t0) * 1e3
            h.estimate(a.iterN, pairs, pairs)
            out = h.apply(xd, trd); torch.cuda.synchronize()
            if i >= a.warmup:
                ms = h.kernel_ms(); wall.append(dt); near.append(ms[0]); st.append(ms[1]); eig.append(ms[2]); rows.append(ms[3]); app.append(ms[4])
        # torch yardstick: the statistics given every item's Gaussian
        am = g.score(xd, mode=0, want_argmin=True)[1].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(m["refN"])])[:-1]
        gi = torch.from_numpy((off[dist] + am[frame, dist]).astype(np.int64)).to(dev)
        iv = torch.from_numpy(m["ivar"]).to(dev)[gi].double(); mi = torch.from_numpy(m["mean"] * m["ivar"]).to(dev)[gi].double()
        xi = torch.cat([torch.ones((N, 1), device=dev, dtype=torch.float64), xd.double()], dim=1)

        def torch_stats():
            Gs = torch.einsum("sti,stj,stk->sijk", iv.view(S, T, D), xi.view(S, T, D + 1), xi.view(S, T, D + 1))
            Zs = torch.einsum("sti,stn->sin", mi.view(S, T, D), xi.view(S, T, D + 1))
            return Gs, Zs
        Gs, Zs = torch_stats(); torch.cuda.synchronize(); t1 = []
        for _ in range(max(2, a.steps // 2)):
            t0 = time.perf_counter(); Gs, Zs = torch_stats(); torch.cuda.synchronize(); t1.append((time.perf_counter() - t0) * 1e3)
        acc0 = h.get_accu(0); Gt = np.tril(Gs[0].cpu().numpy())
        n = D + 1; flop = 2.0 * D * (n * (n + 1) / 2 + n) * N
        lines.append(dict(tool="bench_fsa", S=S, T=T, dimN=D, iterN=a.iterN, ms_accumulate=round(med(wall), 3), ms_nearest=round(med(near), 4),
                          ms_stats=round(med(st), 3), ms_eig=round(med(eig), 3), ms_rows=round(med(rows), 3), ms_apply=round(med(app), 4),
                          tflops_stats=round(flop / (med(st) * 1e-3) / 1e12, 3), estimates_per_s=round(S / ((med(eig) + med(rows)) * 1e-3), 1),
                          apply_gbps=round(N * D * 8 / (med(app) * 1e-3) / 1e9, 2), ms_torch_stats=round(med(t1), 3),
                          max_rel_G_diff_vs_torch=float(np.abs(acc0["G"] - Gt).max() / np.abs(Gt).max()),
                          status=[h.transform_status(s) for s in range(S)].count(0), out_checksum=round(float(out.double().sum().item()), 3)))
        del h, g, xd, Gs, Zs, out
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
