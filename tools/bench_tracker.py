#!/usr/bin/env python
"""Time the spherical-array tracker kernel (dsr_trk_run) on the GPU.

    python tools/bench_tracker.py [--shape U,T,M,orderN,useSubbandsN,modal|spatial,maxLocalN] [--iters N]

The input is a random source spectrum through the plane-wave simulator (a slowly drifting direction, noise at -30 dB).  Prints one JSON line:
ms per call, frames/s per utterance (the filter is sequential in time: T / call time) and per batch (U T / call time)."""
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64,100,512,3,16,modal,2")
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    U, T, M, orderN, use, kind, maxLocalN = a.shape.split(",")
    U, T, M, orderN, use, maxLocalN = int(U), int(T), int(M), int(orderN), int(use), int(maxLocalN)
    import numpy as np
    import torch
    import dsr._capi as K
    K.load()
    dev = torch.device("cuda:0")
    F = M // 2 + 1
    rng = np.random.default_rng(3)
    sim = K.SphTracker("modal", max(orderN, 3), M, useSubbandsN=1)       # the simulator needs the tables only
    X = torch.zeros((U, 32, T, F), dtype=torch.complex64, device=dev)
    seg = 10                                                     # the direction moves every `seg` frames
    for t0 in range(0, T, seg):
        src = (rng.standard_normal((U, min(seg, T - t0), F)) + 1j * rng.standard_normal((U, min(seg, T - t0), F))).astype(np.complex64)
        pw = K.PlaneWaveSim(sim, 0.6 + 0.002 * t0, 0.2 + 0.003 * t0)
        X[:, :, t0:t0 + seg, :] = pw.apply(torch.from_numpy(src).to(dev))
    X += 0.03 * X.abs().mean() * torch.randn(X.shape, dtype=torch.complex64, device=dev)
    trk = K.SphTracker(kind, orderN, M, useSubbandsN=use, sigma2_u=0.01, sigma2_v=0.1, sigma2_init=1.0, maxLocalN=maxLocalN)
    ms = []
    for _ in range(a.iters + 1):
        state = trk.newState(U, dev)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pos, pos64, info = trk.run(X, state=state)
        torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[1:])
    med = ms[len(ms) // 2]
    inf = info.cpu().numpy()
    print(json.dumps(dict(shape=a.shape, rows_2N=2 * trk.useSubbandsN * trk.L, ms_per_call=round(med, 3), ms_min=round(ms[0], 3), ms_max=round(ms[-1], 3),
                          frames_per_s_per_utterance=round(T / med * 1e3, 1), frames_per_s_per_batch=round(U * T / med * 1e3, 1),
                          mean_local_iterations=round(float((inf & 0xff).mean()), 2), error_frames=int(((inf >> 9) & 1).sum()))))


if __name__ == "__main__":
    main()
