#!/usr/bin/env python
"""Time dsr_gcc_run on the GPU: tools/bench_gcc.py [--shape U,T,C,fftLen[,star|all]]... [--kind phat] [--steps 5] [--out profiles/gcc.jsonl]

One JSON line per shape: ms per call (all kernels of dsr_gcc_run), ms of k_gcc_spectrum and of k_gcc_corr (events around each launch,
dsr_gcc_set_timing, in a pass of its own so that the whole-call time is taken without them), correlations per second, and the effective GB/s
on X (read once by k_gcc_spectrum per pair side) and on the cross-spectrum intermediate (written by k_gcc_spectrum, read by k_gcc_corr),
each over the time of the kernels that move it."""
import argparse
import ctypes
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
    ap.add_argument("--kind", default="phat")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dsr.load(); dev = torch.device("cuda:0")
    for sh in a.shape or ["32,1250,8,256,all", "32,1250,64,256,star"]:
        f = sh.split(","); U, T, C, N = (int(v) for v in f[:4]); mode = f[4] if len(f) > 4 else "star"
        pairs = [(0, c) for c in range(1, C)] if mode == "star" else [(i, j) for i in range(C) for j in range(i + 1, C)]
        P, F = len(pairs), N // 2 + 1
        g = dsr.Gcc(a.kind, pairs, sampleRate=16000.0, fftLen=N, nChan=C)
        gen = torch.Generator(device=dev); gen.manual_seed(1)
        X = torch.view_as_complex(torch.randn((U, C, T, F, 2), dtype=torch.float32, device=dev, generator=gen))
        sad = torch.ones((U, T), dtype=torch.int32, device=dev); sad[:, :10] = 0; sad[:, T // 2:T // 2 + 10] = 0
        ts = (torch.arange(1, T + 1, dtype=torch.float64, device=dev) * 0.008)[None].repeat(U, 1).contiguous()
        state = g.newState(U, dev)
        xs = torch.zeros((U, T, P, F), dtype=torch.complex128, device=dev)
        res = torch.zeros((U, T, P, 3), dtype=torch.float64, device=dev); valid = torch.zeros((U, T, P), dtype=torch.int32, device=dev)
        Xr = torch.view_as_real(X)

        def call():
            dsr.check(dsr._lib.dsr_gcc_run(g.h, dsr._dev(Xr), 0, None, dsr._dev(sad), dsr._dev(ts), 1, -g.HUGE, g.HUGE, U, T, dsr._dev(state), dsr._dev(res),
                                           dsr._dev(valid), None, dsr._dev(torch.view_as_real(xs)), dsr.cur_stream()))
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(a.steps):
            e0.record(); call(); e1.record(); torch.cuda.synchronize(); times.append(e0.elapsed_time(e1))
        times.sort(); ms = times[len(times) // 2]
        dsr.check(dsr._lib.dsr_gcc_set_timing(g.h, 1)); kms = []
        for _ in range(a.steps):
            call(); two = (ctypes.c_double * 2)(); dsr.check(dsr._lib.dsr_gcc_kernel_ms(g.h, two)); kms.append((two[0], two[1]))
        dsr.check(dsr._lib.dsr_gcc_set_timing(g.h, 0))
        ms_spec = sorted(k[0] for k in kms)[len(kms) // 2]; ms_corr = sorted(k[1] for k in kms)[len(kms) // 2]
        nSpeech = int(sad.sum().item()) * P
        line = dict(tool="bench_gcc", kind=a.kind, U=U, T=T, C=C, fftLen=N, pairs=P, pair_list=mode, ms=round(ms, 3), ms_min=round(times[0], 3),
                    ms_k_gcc_spectrum=round(ms_spec, 3), ms_k_gcc_corr=round(ms_corr, 3), corr_per_s=round(nSpeech / (ms * 1e-3)),
                    x_GBps=round(2 * U * P * T * F * 8 / (ms_spec * 1e-3) / 1e9, 1),
                    xspec_GBps=round(2 * nSpeech * F * 16 / ((ms_spec + ms_corr) * 1e-3) / 1e9, 1), steps=a.steps)
        s = json.dumps(line); print(s)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
