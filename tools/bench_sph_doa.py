"""Spherical-array 2-D SRP DOA (dsr_sph_srp) timed per kernel on both paths: ms per call, the device times of the SRP stage (k_sph_srp fused, or
k_doa_srp over the folded table), the per-frame N-best (k_sph_frame) and the accumulation (k_doa_acc) from the profiler, the SRP stage's
algorithmic fp64 rate counting 8 (dim C + dim units) nbins per frame fused and 8 C units nbins folded (against the ~75 TFLOP/s
tools/probes/probe_f64_mfma.hip measured), and the beamformer (dsr_sph_apply) with its snapshot read rate.  One JSON line per shape and path.

  python tools/bench_sph_doa.py                          # 32 utt x 1250 frames x EigenMike 32 ch, M 256, 31 x 63 units, maxOrder 4 and 8
  python tools/bench_sph_doa.py --shape 32,1250,32,4,31,63,256 [--path fused|folded] [--no-stages]
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

STAGES = [("k_sph_srp", "srp"), ("k_doa_srp", "srp"), ("k_sph_frame", "frame_nbest"), ("k_doa_acc", "acc"), ("k_sph_apply", "apply")]
PEAK_TFLOPS, PEAK_TBS = 75.0, 8.0


def _stage_ms(fn):
    import torch
    from torch.profiler import profile, ProfilerActivity
    ms = {}
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        for key, name in STAGES:
            if key in ev.key:
                ms[name] = ms.get(name, 0.0) + t / 1e3
                break
    return ms


def run(U, T, Cn, mo, nT, nP, M, path, reps, stages=True):
    import torch
    import dsr._capi as dsr
    dsr.load()
    dev = torch.device("cuda:0")
    F = M // 2 + 1
    if path:
        os.environ["DSR_SPH_SRP_PATH"] = path
    else:
        os.environ.pop("DSR_SPH_SRP_PATH", None)
    s = dsr.SphDoaSRP("EB", 5, 16000, M, Cn, mo)
    if Cn == 32:
        s.setEigenMikeGeometry()
    else:
        rng = np.random.default_rng(1)
        s.setArrayGeometry(42.0, np.arccos(rng.uniform(-1, 1, Cn)), rng.uniform(0, 2 * np.pi, Cn))
    s.setSearchParam(0.0, np.pi, -np.pi, np.pi, np.pi / nT, 2 * np.pi / nP)
    assert s.gridN() == (nT, nP), s.gridN()
    nU = nT * nP; dim = mo * mo
    t0 = time.perf_counter(); taken = s.path(); table_s = time.perf_counter() - t0
    g = torch.Generator(device=dev); g.manual_seed(1)
    X = torch.randn((U, Cn, T, F, 2), device=dev, generator=g, dtype=torch.float32)
    nf = torch.full((U,), T, dtype=torch.int32, device=dev)
    energy = torch.empty((U, T), dtype=torch.float32, device=dev)
    nbr = torch.empty((U, T, 5), dtype=torch.float64, device=dev)
    nbi = torch.empty((U, T, 5), dtype=torch.int32, device=dev)
    acc = torch.zeros((U, nU), dtype=torch.float64, device=dev)
    y = torch.empty((U, T, F, 2), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call():
        dsr.check(dsr._lib.dsr_sph_srp(s.h, p(X), p(nf), U, T, p(energy), None, p(nbr), p(nbi), p(acc), None, None, dsr.cur_stream()))

    def apply():
        dsr.check(dsr._lib.dsr_sph_apply(s.h, p(X), p(nf), U, T, p(y), None, dsr.cur_stream()))
    t0 = time.perf_counter(); call(); apply(); torch.cuda.synchronize(); first_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    res = {"U": U, "frames": T, "C": Cn, "maxOrder": mo, "dim": dim, "nTheta": nT, "nPhi": nP, "units": nU, "M": M, "path": taken,
           "ms_per_call": round(wall, 3), "host_table_s": round(table_s, 2), "first_call_s": round(first_s, 2)}
    if stages:
        ms = _stage_ms(call)
        ms.update({k: v for k, v in _stage_ms(apply).items() if k == "apply"})
        nbins = M // 2                                                        # the default range [1, M/2]
        per = (dim * Cn + dim * nU) if taken == "fused" else Cn * nU
        flop = 8.0 * per * nbins * U * T
        res.update(ms_per_stage={k: round(v, 3) for k, v in ms.items()}, gflop=round(flop / 1e9, 1))
        if ms.get("srp", 0) > 0:
            tf = flop / (ms["srp"] * 1e-3) / 1e12
            res.update(srp_tflops=round(tf, 2), srp_frac_of_f64_peak=round(tf / PEAK_TFLOPS, 3))
        if ms.get("apply", 0) > 0:
            gbs = (X.numel() * 4.0 + y.numel() * 4.0) / (ms["apply"] * 1e-3) / 1e9
            res.update(apply_gbs=round(gbs, 1), apply_frac_of_hbm=round(gbs / (PEAK_TBS * 1e3), 3))
    res["finite"] = bool(torch.isfinite(acc).all().item() and torch.isfinite(y).all().item())
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="U,T,C,maxOrder,nTheta,nPhi,M")
    ap.add_argument("--path", choices=["fused", "folded"], help="force one path (default: both)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-stages", action="store_true", help="skip the per-kernel split (torch profiler), e.g. under rocprofv3")
    a = ap.parse_args()
    todo = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else [(32, 1250, 32, 4, 31, 63, 256), (32, 1250, 32, 8, 31, 63, 256)]
    for shape in todo:
        for path in ([a.path] if a.path else ["fused", "folded"]):
            run(*shape, path, a.reps, not a.no_stages)


if __name__ == "__main__":
    main()
