"""Multi-channel WPE (dsr_wpe_multi) timed per stage: ms per call and per kernel (residual / theta, Gram, r vector, Cholesky + solves, output on
the tiled path; the one-workgroup kernel and its output kernel on the LDS path) from the profiler's device times, and the Gram's rate in
TFLOP/s counted as the issue's arithmetic does (lower-triangle entries x frames x channels x subbands x 8 per iteration).  One JSON line per shape.

  python tools/bench_wpe_multi.py                       # 64x8, 32x8, 64x16 at 1250 frames x 129 subbands; 8x10x1257 on both paths
  python tools/bench_wpe_multi.py --shape 64,8,1250,129 --path tiled
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STAGES = [("k_wt_resid<false>", "residual"), ("k_wt_gram", "gram"), ("k_wt_rvec", "rvec"), ("k_wt_chol", "chol_solve"), ("k_wt_resid<true>", "output"),
          ("k_wpe_series", "transpose"), ("k_wpe_multi_out", "lds_output"), ("k_wpe_multi<", "lds_estimate")]


def run(C, P, N, F, path, iters, reps):
    import torch
    import dsr._capi as dsr
    from torch.profiler import profile, ProfilerActivity
    dsr.load()
    dev = torch.device("cuda:0")
    M, lowerN = 2 * (F - 1), 2
    upperN = lowerN + P - 1
    g = torch.Generator(device=dev); g.manual_seed(1)
    Y = torch.complex(torch.randn((1, C, N, F), device=dev, generator=g), torch.randn((1, C, N, F), device=dev, generator=g)).to(torch.complex64)
    if path == "tiled":
        os.environ["DSR_WPE_MULTI_TILED"] = "1"
    else:
        os.environ.pop("DSR_WPE_MULTI_TILED", None)

    def call():
        return dsr.wpe_multi(Y, M, lowerN, upperN, iters, -20.0, 0.0, 16000.0)
    out, gn = call()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(gn).all().item())
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    ms = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        for key, name in STAGES:
            if key in ev.key:
                ms[name] = ms.get(name, 0.0) + t / 1e3
                break
    PT = C * P
    gram_flop = PT * (PT + 1) / 2 * N * C * F * 8.0 * iters
    res = {"C": C, "P": P, "N": N, "F": F, "path": path, "iterations": iters, "ms_per_call": round(wall, 3),
           "ms_per_stage": {k: round(v, 3) for k, v in ms.items()}, "finite": finite}
    if "gram" in ms and ms["gram"] > 0:
        res["gram_tflops"] = round(gram_flop / (ms["gram"] * 1e-3) / 1e12, 2)
    print(json.dumps(res), flush=True)
    del out, gn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="C,P,N,F")
    ap.add_argument("--path", default=None, choices=["tiled", "lds", "auto"])
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    if a.shape:
        todo = [(tuple(int(v) for v in s.split(",")), a.path or "auto") for s in a.shape]
    else:
        todo = [((64, 8, 1250, 129), "auto"), ((32, 8, 1250, 129), "auto"), ((64, 16, 1250, 129), "auto"),
                ((8, 10, 1257, 129), "lds"), ((8, 10, 1257, 129), "tiled")]
    for (C, P, N, F), path in todo:
        run(C, P, N, F, path, a.iterations, a.reps)


if __name__ == "__main__":
    main()
