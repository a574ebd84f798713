"""Subband echo cancellation (dsr_aec_apply) timed with device events: warm-up, several repeats, min and median ms per call, ns per dependent
step (ms / frames: every (utterance, bin) chain walks the frames in order, all chains in parallel), GB/s on the 24 algorithmic bytes per
(frame, bin) (played and recorded read, the residual written, complex64 each), and in the same run a copy_ of the same bytes for scale.
One JSON line per shape, appended to profiles/aec.jsonl.

  python tools/bench_aec.py                                    # the three one-tap kinds at 256,1257,256; the block filter and the two information
                                                               # filters at L 4, 16, 32 for U 32 and 256
  python tools/bench_aec.py --shape 256,1257,256,16 --kind block [--kind dtd] [--kind info] [--kind sqrtinfo] [--no-append]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), statistics.median(ms)


def run(kind, U, T, M, L, warm, reps):
    import torch
    import dsr._capi as dsr
    dsr.load()
    dev = torch.device("cuda:0"); F = M // 2 + 1
    g = torch.Generator(device=dev); g.manual_seed(1)
    V = torch.view_as_complex(30.0 * torch.randn((U, T, F, 2), device=dev, generator=g, dtype=torch.float32))
    A = 0.3 * V + torch.view_as_complex(torch.randn((U, T, F, 2), device=dev, generator=g, dtype=torch.float32))
    a = dsr.Aec(kind, M, L); st = a.newState(U, dev)
    out = [None]

    def call():
        out[0] = a.apply(V, A, None, st)
    lo, med = timed(call, warm, reps)
    nbytes = 24.0 * U * T * F
    src = torch.empty(int(nbytes) // 2 // 4, dtype=torch.float32, device=dev); dst = torch.empty_like(src)      # copy_: nbytes / 2 read + nbytes / 2 written
    clo, cmed = timed(lambda: dst.copy_(src), warm, reps)
    res = {"kind": kind, "U": U, "frames": T, "M": M, "L": a.L, "ms_min": round(lo, 3), "ms_median": round(med, 3), "ns_per_step": round(lo * 1e6 / T, 1),
           "gbs_24B": round(nbytes / (lo * 1e-3) / 1e9, 1), "copy_same_bytes_ms_min": round(clo, 3), "copy_same_bytes_ms_median": round(cmed, 3),
           "copy_gbs": round(nbytes / (clo * 1e-3) / 1e9, 1), "state_mib": round(a.stateBytes(U) / 2 ** 20, 1),
           "finite": bool(torch.isfinite(torch.view_as_real(out[0])).all().item())}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="U,T,M,L")
    ap.add_argument("--kind", action="append", help="nlms | kalman | block | dtd | info | sqrtinfo (default block)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-append", action="store_true", help="do not append to profiles/aec.jsonl (e.g. under a profiler)")
    a = ap.parse_args()
    if a.shape:
        todo = [(k,) + tuple(int(v) for v in s.split(",")) for s in a.shape for k in (a.kind or ["block"])]
    else:
        todo = [(k, 256, 1257, 256, 1) for k in ("nlms", "kalman", "block")] + [(k, U, 1257, 256, L) for k in ("block", "info", "sqrtinfo") for U in (32, 256) for L in (4, 16, 32)]
    for kind, U, T, M, L in todo:
        res = run(kind, U, T, M, L, a.warmup, a.reps)
        if not a.no_append:
            os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
            with open(os.path.join(ROOT, "profiles", "aec.jsonl"), "a") as f:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
