#!/usr/bin/env python
"""Time the training accumulation on the GPU: tools/bench_train.py [--steps 5] [--warmup 2] [--frames 1000000] [--out profiles/train.jsonl]

One JSON line per shape -- the benchmark's model (1024 codebooks, dimN 39) with 4 and with 16 Gaussians per codebook, one item per frame:
  ms_call        the whole dsr_train_accumulate (host sort of the items, uploads, three kernels, scores back), median of --steps calls
  ms_posterior   k_train_post alone (events inside the library); ms_contract: k_train_acc + k_train_reduce
  items_per_s    items / ms_call;  bytes_min: the traffic no schedule can avoid (x read by both kernels, gamma written and read once, the
                 chunk partials written and read, scores), GBps_kernels = bytes_min over the two kernel times
  gflops_useful  2 M refN (2 dimN + 2) fp64 flop of the contraction over ms_contract; gflops_issued counts the 16 x 16 tiles the MFMAs run
  ms_torch       the same sums by torch in fp64 (index_add_ of gamma[:, r] * [x | x^2 | 1+ | 1-] per r) from a gamma tensor that already
                 exists -- a yardstick for ms_contract, not a reference result"""
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dsr.load(); dev = torch.device("cuda:0")
    K, D, M = 1024, 39, a.frames
    rng = np.random.default_rng(3)
    x = torch.randn((M, D), device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(1))
    frame = np.arange(M, dtype=np.int32); dist = rng.integers(0, K, M).astype(np.int32)
    factor = np.where(rng.random(M) < 0.25, -0.5, 1.0).astype(np.float32)
    lines = []
    for R in (4, 16):
        g = dsr.Gmm(**synth.gmm_model(K, R, D, seed=12)); t = dsr.Trainer(g); t.set_timing(True)
        wall, post, con = [], [], []
        for i in range(a.warmup + a.steps):
            t.zero(); torch.cuda.synchronize()
            t0 = time.perf_counter(); t.accumulate(x, frame, dist, factor); dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                wall.append(dt); p, c = t.kernel_ms(); post.append(p); con.append(c)
        med = lambda v: sorted(v)[len(v) // 2]                                        # noqa: E731
        ms, msp, msc = med(wall), med(post), med(con)
        NC = 2 * D + 2; chunks = int(np.ceil(np.bincount(dist, minlength=K) / 256.0).sum())
        bytes_min = 2 * M * D * 4 + 2 * M * R * 4 + 2 * chunks * R * NC * 8 + M * 4 + M * 12
        # torch yardstick for the contraction
        gam = torch.rand((M, R), device=dev, dtype=torch.float64); fd = torch.from_numpy(factor).to(dev); dd = torch.from_numpy(dist.astype(np.int64)).to(dev)

        def torch_sums():
            xa = torch.cat([x.double(), x.double() ** 2, (fd > 0).double()[:, None], (fd <= 0).double()[:, None]], dim=1)
            acc = torch.zeros((K * R, NC), device=dev, dtype=torch.float64)
            for r in range(R):
                acc.index_add_(0, dd * R + r, gam[:, r, None] * xa)
            return acc
        torch_sums(); torch.cuda.synchronize()
        tt = []
        for _ in range(max(2, a.steps // 2)):
            t0 = time.perf_counter(); torch_sums(); torch.cuda.synchronize(); tt.append((time.perf_counter() - t0) * 1e3)
        d = t.get()
        lines.append(dict(tool="bench_train", K=K, refN=R, dimN=D, items=M, ms_call=round(ms, 3), ms_posterior=round(msp, 3), ms_contract=round(msc, 3),
                          items_per_s=round(M / (ms * 1e-3)), bytes_min=bytes_min, GBps_kernels=round(bytes_min / ((msp + msc) * 1e-3) / 1e9, 1),
                          gflops_useful=round(2.0 * M * R * NC / (msc * 1e-3) / 1e9, 1),
                          gflops_issued=round(2.0 * M * 16 * ((R + 15) // 16) * 16 * ((NC + 15) // 16) / (msc * 1e-3) / 1e9, 1),
                          ms_torch=round(med(tt), 3), count_total=round(float(d["count"].sum() + d["den"].sum()), 3)))
        del gam, t, g
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
