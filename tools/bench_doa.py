"""Steered-response-power DOA (dsr_doa_srp) timed per kernel: ms per call, the device times of the SRP GEMM (k_doa_srp), the per-frame N-best
(k_doa_frame) and the accumulation (k_doa_acc) from the profiler, the SRP kernel's algorithmic fp64 rate counting 8 C nTheta nbins per frame
(against the ~75 TFLOP/s tools/probes/probe_f64_mfma.hip measured) and its snapshot read rate (against 8 TB/s).  One JSON line per shape.

  python tools/bench_doa.py                              # 1024 utt x 1257 frames x 8 ch x 31 theta, M 256; 32 x 1250 x 64 ch x 181 theta
  python tools/bench_doa.py --shape 64,1257,8,31,256 [--no-stages]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STAGES = [("k_doa_srp", "srp"), ("k_doa_frame", "frame_nbest"), ("k_doa_acc", "acc")]
PEAK_TFLOPS, PEAK_TBS = 75.0, 8.0


def run(U, T, Cn, nT, M, reps, stages=True):
    import torch
    import dsr._capi as dsr
    from torch.profiler import profile, ProfilerActivity
    dsr.load()
    dev = torch.device("cuda:0")
    F = M // 2 + 1
    d = dsr.DoaSRP(5, 16000, M, Cn)
    d.setArrayGeometry(np.arange(Cn) / 16000.0)
    d.setSearchParam(0.0, np.pi, np.pi / nT)                                  # nT directions
    assert d.thetaN() == nT, d.thetaN()
    g = torch.Generator(device=dev); g.manual_seed(1)
    X = torch.randn((U, Cn, T, F, 2), device=dev, generator=g, dtype=torch.float32)
    nf = torch.full((U,), T, dtype=torch.int32, device=dev)
    energy = torch.empty((U, T), dtype=torch.float32, device=dev)
    nbr = torch.empty((U, T, 5), dtype=torch.float64, device=dev)
    nbi = torch.empty((U, T, 5), dtype=torch.int32, device=dev)
    acc = torch.zeros((U, nT), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call():
        dsr.check(dsr._lib.dsr_doa_srp(d.h, p(X), p(nf), U, T, p(energy), None, p(nbr), p(nbi), p(acc), None, None, dsr.cur_stream()))
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    ms = {}
    if not stages:                                                            # under an outside profiler (tools/pmc.sh): no torch profiler
        print(json.dumps({"U": U, "frames": T, "C": Cn, "nTheta": nT, "M": M, "ms_per_call": round(wall, 3)}), flush=True)
        return
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        for key, name in STAGES:
            if key in ev.key:
                ms[name] = ms.get(name, 0.0) + t / 1e3
                break
    nbins = M // 2                                                            # the default range [1, M/2]
    flop = 8.0 * Cn * nT * nbins * U * T
    xbytes = X.numel() * 4.0
    res = {"U": U, "frames": T, "C": Cn, "nTheta": nT, "M": M, "ms_per_call": round(wall, 3), "ms_per_stage": {k: round(v, 3) for k, v in ms.items()},
           "gflop": round(flop / 1e9, 1), "finite": bool(torch.isfinite(acc).all().item())}
    if ms.get("srp", 0) > 0:
        tf = flop / (ms["srp"] * 1e-3) / 1e12
        gbs = xbytes / (ms["srp"] * 1e-3) / 1e9
        res.update(srp_tflops=round(tf, 2), srp_frac_of_f64_peak=round(tf / PEAK_TFLOPS, 3), snapshot_gbs=round(gbs, 1),
                   snapshot_frac_of_hbm=round(gbs / (PEAK_TBS * 1e3), 3))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="U,T,C,nTheta,M")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-stages", action="store_true", help="skip the per-kernel split (torch profiler), e.g. under rocprofv3")
    a = ap.parse_args()
    todo = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else [(1024, 1257, 8, 31, 256), (32, 1250, 64, 181, 256)]
    for U, T, Cn, nT, M in todo:
        run(U, T, Cn, nT, M, a.reps, not a.no_stages)


if __name__ == "__main__":
    main()
