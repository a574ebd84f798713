#!/usr/bin/env python
"""Time dsr_mcc_run on the GPU: tools/bench_mcc.py [--shape U,C,N,L,linear|circular]... [--maxSource 1] [--steps 7] [--out profiles/mcc.jsonl]

One JSON line per shape: ms per call (median, minimum and maximum over the steps, device events around the call, after warm-up calls),
ms of k_mcc_cost, k_mcc_nbest and k_mcc_eig (events around each launch, dsr_mcc_set_timing, in a pass of its own), fp64 TFLOP/s on the Gram
matrices over k_mcc_cost's time counted as 2 C^2 (L-D) G B U (`gram_tflops_full`: the count of the full product; the kernel forms the lower
16x16 tiles only, `gram_tflops_issued` counts what its MFMAs execute, padded tiles included), GB/s on the samples (each block read once
per call by definition: the kernel re-stages a tile for every four candidates from cache), and blocks per second.  Linear arrays have
40 mm spacing, circular ones a radius of 100 mm; fs = 16000."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import dsr._capi as dsr
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None)
    ap.add_argument("--maxSource", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dsr.load(); dev = torch.device("cuda:0")
    for sh in a.shape or ["8,64,16384,4096,circular", "32,64,16384,4096,circular", "32,8,16384,1024,linear"]:
        f = sh.split(","); U, Cn, N, L = (int(v) for v in f[:4]); kind = f[4] if len(f) > 4 else "circular"
        sg = dsr.SearchGrid(kind, Cn, True, 16000)
        if kind == "circular":
            sg.setRadius(100.0)
        else:
            sg.setDistanceBtwMicrophones(40.0)
        m = dsr.MccLocalizer(sg, a.maxSource); G, D, B = m.G, m.D, N // L
        gen = torch.Generator(device=dev); gen.manual_seed(1)
        x = torch.randn((U, Cn, N), dtype=torch.float32, device=dev, generator=gen)

        S = a.maxSource; z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)     # outputs allocated once, outside the timed calls
        o = [z((U, B), torch.int32), z((U, B, S), torch.int32), z((U, B, S)), z((U, B, S, Cn), torch.int32), z((U, B, S, 3)), z((U, B, S, Cn))]

        def call():
            dsr.check(dsr._lib.dsr_mcc_run(m.h, dsr._dev(x), None, U, N, L, *[dsr._dev(t) for t in o], None, None, dsr.cur_stream()))
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(a.steps):
            e0.record(); call(); e1.record(); torch.cuda.synchronize(); times.append(e0.elapsed_time(e1))
        times.sort(); ms = times[len(times) // 2]
        m.setTiming(True); kms = []
        for _ in range(a.steps):
            call(); kms.append(m.kernelMs())
        m.setTiming(False)
        k3 = [sorted(float(k[j]) for k in kms)[len(kms) // 2] for j in range(3)]
        CT = (Cn + 15) // 16
        full = 2.0 * Cn * Cn * (L - D) * G * B * U; issued = 2.0 * 256 * (CT * (CT + 1) // 2) * (L - D) * G * B * U
        line = dict(tool="bench_mcc", kind=kind, U=U, C=Cn, N=N, L=L, B=B, G=G, D=D, maxSource=a.maxSource, ms=round(ms, 3), ms_min=round(times[0], 3),
                    ms_max=round(times[-1], 3), ms_k_mcc_cost=round(k3[0], 3), ms_k_mcc_nbest=round(k3[1], 3), ms_k_mcc_eig=round(k3[2], 3),
                    gram_tflops_full=round(full / (k3[0] * 1e-3) / 1e12, 2), gram_tflops_issued=round(issued / (k3[0] * 1e-3) / 1e12, 2),
                    samples_GBps=round(U * Cn * B * L * 4 / (ms * 1e-3) / 1e9, 2), blocks_per_s=round(U * B / (ms * 1e-3)), steps=a.steps)
        s = json.dumps(line); print(s)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
