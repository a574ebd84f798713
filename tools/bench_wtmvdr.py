#!/usr/bin/env python
"""Time dsr_wtmvdr_run on the GPU: tools/bench_wtmvdr.py [--shape dim,order]... [--frames 65536] [--steps 5] [--out profiles/wtmvdr.jsonl]

One JSON line per shape: ms per call (all kernels of dsr_wtmvdr_run) and frames per second, ms of each kernel (events around each launch,
dsr_wtmvdr_set_timing, in a pass of its own so that the whole-call time is taken without them), and beside them the ms per call of the existing
WarpMVDR envelope (LpcEnvelope, method 0, kind 0) on the same frames as a yardstick."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def median_ms(call, steps, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        e0.record(); call(); e1.record(); torch.cuda.synchronize(); times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    import torch
    import dsr._capi as dsr
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--warp", type=float, default=0.4595)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dsr.load(); dev = torch.device("cuda:0"); T = a.frames
    for sh in a.shape or ["320,60", "512,40"]:
        dim, order = (int(v) for v in sh.split(","))
        gen = torch.Generator(device=dev); gen.manual_seed(1)
        n = torch.arange(dim, dtype=torch.float32, device=dev)
        win = 0.54 - 0.46 * torch.cos(2.0 * torch.pi * n / (dim - 1))
        fr = (torch.randn((T, dim), dtype=torch.float32, device=dev, generator=gen).cumsum(1) * 300.0 * win).contiguous()      # coloured frames under a Hamming window
        wt = dsr.WtMvdrEnvelope(dim, order, 0, a.warp, False, 0.1)
        out = torch.zeros((T, dim // 2 + 1), dtype=torch.float64, device=dev)

        def call():
            dsr.check(dsr._lib.dsr_wtmvdr_run(wt.h, dsr._dev(fr), None, T, dsr._dev(out), None, None, dsr.cur_stream()))
        ms, ms_min = median_ms(call, a.steps, a.warmup)
        dsr.check(dsr._lib.dsr_wtmvdr_set_timing(wt.h, 1)); kms = []
        for _ in range(a.steps):
            call(); four = (C.c_double * 4)(); dsr.check(dsr._lib.dsr_wtmvdr_kernel_ms(wt.h, four)); kms.append(tuple(four))
        dsr.check(dsr._lib.dsr_wtmvdr_set_timing(wt.h, 0))
        med = [sorted(k[i] for k in kms)[len(kms) // 2] for i in range(4)]
        lpc = dsr.LpcEnvelope(dim, order, a.warp, 0, 0)
        out2 = torch.zeros_like(out)

        def call2():
            dsr.check(dsr._lib.dsr_lpc_run(lpc.h, dsr._dev(fr), T, dsr._dev(out2), dsr.cur_stream()))
        ms2, ms2_min = median_ms(call2, a.steps, a.warmup)
        line = dict(tool="bench_wtmvdr", dim=dim, order=order, T=T, warp=a.warp, ms=round(ms, 3), ms_min=round(ms_min, 3), frames_per_s=round(T / (ms * 1e-3)),
                    ms_k_lpc_transpose=round(med[0], 3), ms_k_wt_lp=round(med[1], 3), ms_k_wt_chain=round(med[2], 3), ms_k_wt_envelope=round(med[3], 3),
                    yardstick="LpcEnvelope(method 0, kind 0)", yardstick_ms=round(ms2, 3), yardstick_ms_min=round(ms2_min, 3),
                    yardstick_frames_per_s=round(T / (ms2 * 1e-3)), finite=bool(torch.isfinite(out).all().item()), steps=a.steps)
        s = json.dumps(line); print(s)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
