#!/usr/bin/env python3
"""Sample-rate converter micro benchmark (dsr_src_apply, one-shot): one JSON line per shape with ms per call (events around repeated calls, after
warm-up, output allocated once), the kernel's own ms (the handle's events), GB/s on samples read plus samples written, GFMA/s (outputs x 2K taps),
the cell taken, and two yardsticks measured in the same run: torch copy_ of a buffer that moves the same bytes, and the polyphase formulation with
torch.nn.functional.conv1d -- one output channel per phase, each phase's 2K taps placed at its base offset in a kernel of 2K + floor((L-1) M / L)
samples, stride M, the [rows][L][k] result transposed into [rows][k L].  conv1d is timed on at most --yard-rows rows and scaled to the batch.

  tools/bench_src.py --shape 1000,8,441000 --rates 44100,16000 --method best
  tools/bench_src.py --shape 1000,8,441000 --rates 48000,16000 --method fastest
  tools/bench_src.py --shape 32,64,480000 --rates 22050,16000 --method medium"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "distantspeechrecognition-mirror_amd"))
import torch
from dsr import _src

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="64,8,160000", help="U,C,N")
ap.add_argument("--rates", default="44100,16000", help="src,dst")
ap.add_argument("--method", default="best")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--yard-rows", type=int, default=256)
ap.add_argument("--no-conv1d", action="store_true")
a = ap.parse_args()
U, Cn, N = [int(v) for v in a.shape.split(",")]; src, dst = [int(v) for v in a.rates.split(",")]
_src.load(); dev = torch.device("cuda:0")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


c = _src.SampleRateConverter(src, dst, a.method)
nOut = c.out_samples(N); rows = U * Cn
x = torch.empty((U, Cn, N), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0)
y = torch.empty((U, Cn, nOut), dtype=torch.float32, device=dev)
c.set_timing(True)
ms = timed(lambda: c.apply(x, y=y), a.reps, a.warmup)
ms_kernel = c.kernel_ms()
moved = 4.0 * rows * (N + nOut); fma = float(rows) * nOut * 2 * c.K
p = c.path()
rec = dict(U=U, C=Cn, N=N, srcRate=src, dstRate=dst, method=a.method, L=c.L, M=c.M, K=c.K, outputs=nOut, table=_src.SRC_TABLE_NAMES[p[0]],
           input=("lds", "direct")[p[1]], tile=p[2], lds_bytes=p[3], ms_call=round(ms, 3), ms_kernel=round(ms_kernel, 3),
           GBps=round(moved / ms / 1e6, 1), GFMAps=round(fma / ms / 1e6, 1), GB_read=round(4e-9 * rows * N, 2), GB_written=round(4e-9 * rows * nOut, 2))

half = rows * (N + nOut) // 2                                                  # copy_ of half the samples reads and writes as many bytes as the call moves
b0 = torch.empty(half, dtype=torch.float32, device=dev).uniform_(-1.0, 1.0); b1 = torch.empty_like(b0)
ms_copy = timed(lambda: b1.copy_(b0), a.reps, a.warmup)
rec.update(copy_ms=round(ms_copy, 3), copy_GBps=round(8.0 * half / ms_copy / 1e6, 1), of_copy=round(ms_copy / ms, 3))
del b0, b1

if not a.no_conv1d and c.K > 0 and c.L * (2 * c.K + c.M) <= (1 << 24):
    try:
        t = c.table().astype(np.float32); L, M, K = c.L, c.M, c.K
        base = [(q * M) // L for q in range(L)]; W = 2 * K + base[-1]
        w = np.zeros((L, 1, W), np.float32)
        for q in range(L):
            w[q, 0, base[q]:base[q] + 2 * K] = t[(q * M) % L]
        w = torch.from_numpy(w).to(dev)
        r = min(rows, a.yard_rows); k = -(-nOut // L)
        xr = x.reshape(rows, 1, N)[:r]
        need = (k - 1) * M + W                                                 # samples the last output group reads, K - 1 of them before sample 0
        xp = torch.nn.functional.pad(xr, (K - 1, max(need - (K - 1) - N, 0)))
        yr = torch.empty((r, k * L), dtype=torch.float32, device=dev)

        def conv():
            o = torch.nn.functional.conv1d(xp, w, stride=M)[:, :, :k]
            yr.view(r, k, L).copy_(o.transpose(1, 2))
        ms_conv = timed(conv, max(a.reps // 2, 1), 1) * rows / r
        err = float((yr[:, :nOut] - y.reshape(rows, nOut)[:r]).abs().max())
        rec.update(conv1d_ms=round(ms_conv, 3), conv1d_rows_timed=r, conv1d_max_diff=err, speedup_over_conv1d=round(ms_conv / ms, 2))
    except Exception as e:                                                     # the yardstick is an extra: the call's time stands without it
        rec.update(conv1d_error=str(e)[:120])
print(json.dumps(rec), flush=True)
