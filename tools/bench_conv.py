#!/usr/bin/env python
"""Time dsr_conv_apply on the GPU: tools/bench_conv.py [--shape U,C,L,P,T]... [--kind add] [--steps 5] [--out profiles/conv.jsonl]

One JSON line per shape: ms per call (events around the call, median after a warm-up) and input samples per second, ms of the transform
kernel and of the fold (dsr_conv_set_timing, in a pass of its own so that the whole-call time is taken without its events), the bytes the two
kernels move through global memory, and beside them the ms per call of the same convolution written with torch.fft.rfft / irfft in fp64 on the
same device (sections only, without the fp32 fold) as an outside yardstick."""
import argparse
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
    import numpy as np
    import torch
    import dsr._capi as dsr
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="U,C,L,P,T")
    ap.add_argument("--kind", default="add", choices=["add", "save"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dsr.load(); dev = torch.device("cuda:0")
    for sh in a.shape or ["64,8,1024,4000,160", "256,8,256,700,600"]:
        U, Cn, L, P, T = (int(v) for v in sh.split(","))
        h = np.random.default_rng(1).standard_normal((Cn, P)) * np.exp(-6.0 * np.arange(P) / P)
        cv = dsr.BlockConvolver(a.kind, L, h)
        N, size = cv.fftLen, cv.size
        gen = torch.Generator(device=dev); gen.manual_seed(1)
        x = (3000.0 * torch.randn((U, T, L), dtype=torch.float32, device=dev, generator=gen)).contiguous()
        st = cv.state(U, dev)
        y = torch.zeros((U, Cn, T, size), dtype=torch.float32, device=dev)

        def call():
            dsr.check(dsr._lib.dsr_conv_apply(cv.h, dsr._dev(x), None, U, T, dsr._dev(st), dsr._dev(y), dsr.cur_stream()))
        ms, ms_min = median_ms(call, a.steps, a.warmup)
        cv.set_timing(True); kms = []
        for _ in range(a.steps):
            call(); kms.append(cv.kernel_ms())
        cv.set_timing(False)
        med = [sorted(k[i] for k in kms)[len(kms) // 2] for i in range(2)]
        S = L + P - 1
        depth = -(-S // L)                                               # the sections a sample's chain reads
        b_fft = U * T * L * 4 + U * T * Cn * (N // 2 + 1) * 16 + (U * T * Cn * S * 8 if a.kind == "add" else U * T * Cn * size * 4)
        b_fold = (U * Cn * T * L * depth * 8 + U * Cn * T * L * 4) if a.kind == "add" else 0
        Hd = torch.fft.rfft(torch.from_numpy(h).to(dev), n=N, dim=1)

        def yard():
            X = torch.fft.rfft(x.to(torch.float64), n=N, dim=2)
            return torch.fft.irfft(X[:, None] * Hd[None, :, None], n=N, dim=3)[..., :S]
        try:
            ms2, ms2_min = median_ms(yard, a.steps, a.warmup)
        except RuntimeError as e:                                        # the yardstick holds every spectrum at once
            ms2 = ms2_min = None; print("yardstick failed: %s" % str(e).splitlines()[0], file=sys.stderr)
        line = dict(tool="bench_conv", kind=a.kind, U=U, C=Cn, L=L, P=P, T=T, N=N, ms=round(ms, 3), ms_min=round(ms_min, 3),
                    in_samples_per_s=round(U * T * L / (ms * 1e-3)), out_samples_per_s=round(U * Cn * T * L / (ms * 1e-3)),
                    ms_k_conv_fft=round(med[0], 3), ms_k_conv_fold=round(med[1], 3), fold_share=round(med[1] / (med[0] + med[1]), 3),
                    bytes_fft=b_fft, bytes_fold=b_fold, gbytes_per_s=round((b_fft + b_fold) / (ms * 1e-3) / 1e9, 1),
                    yardstick="torch.fft.rfft/irfft fp64, sections only", yardstick_ms=None if ms2 is None else round(ms2, 3),
                    yardstick_ms_min=None if ms2 is None else round(ms2_min, 3), finite=bool(torch.isfinite(y).all().item()), steps=a.steps)
        s = json.dumps(line); print(s)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")
        del x, y, st, cv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
