#!/usr/bin/env python3
"""Multi-stream combine micro benchmark (csrc/ms_kernels.hip): [--shape N,KA,KV] ..., one JSON line per shape with
  ms per combine, in place and out of place (median of --rounds windows of --reps calls each, with the windows' min and max),
  the achieved GB/s on the 4 N (2 KA + KV) bytes the combination has to move, and the path the dispatch took,
and two yardsticks timed in the same run on the same tensors:
  copy      torch copy_ of the audio matrix, 8 N KA bytes moved (the yardstick DESIGN.md section 7 uses), and the combine's rate as a share of it;
  torch     the plain formulation (wA * sA.double() + wV * sV.double()[:, map]).float().
Default shapes: identity-sized, many-to-one, the scalar path, the global gather.  A last line gives what a two-model decode adds to a one-model
decode at the benchmark's shape: the two GMM stages and the combine, by device events."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "distantspeechrecognition-mirror_amd"))
import torch
import dsr._capi as dsr
import dsr._ms as M
from tests import synth
ap = argparse.ArgumentParser()
ap.add_argument("--shape", action="append", default=None, help="N,KA,KV (repeatable)")
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-decode-cost", action="store_true")
a = ap.parse_args()
shapes = a.shape or ["998000,1024,1024", "998000,1024,64", "998000,1023,64", "250000,1024,%d" % (M.LDS_BUDGET // 4 + 256)]
dsr.load(); dev = torch.device("cuda:0")
NAMES = {M.VECTOR_LDS: "vector+lds", M.SCALAR_LDS: "scalar+lds", M.GATHER: "gather"}
WA, WV = 0.95, 0.05


def timed(fn, reps=None, rounds=None):
    """-> (median, min, max) ms per call over `rounds` windows of `reps` calls, after a warm-up window"""
    reps = reps or a.reps; rounds = rounds or a.rounds
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def model(K, D=2):
    return dsr.Gmm(refN=np.ones(K, np.int32), mean=np.zeros((K, D), np.float32), ivar=np.ones((K, D), np.float32), det=np.zeros(K, np.float32),
                   val=np.zeros(K, np.float32))


for sh in shapes:
    N, KA, KV = [int(v) for v in sh.split(",")]
    table = np.arange(KA, dtype=np.int32) % KV
    ms = M.MultiStream(model(KA), model(KV), M.DistribMap({"ds%d" % k: "ds%d" % t for k, t in enumerate(table)}), WA, WV)
    sA = torch.randn((N, KA), device=dev); sV = torch.randn((N, KV), device=dev); out = torch.empty_like(sA)
    path, rows, lds = ms.path(True)
    nbytes = 4 * N * (2 * KA + KV)
    t_out = timed(lambda: ms.combine(sA, sV, out=out))
    t_in = timed(lambda: ms.combine(sA, sV, out=sA))                 # the values drift with every call; the traffic does not
    sA.normal_()
    t_copy = timed(lambda: out.copy_(sA))
    tmap = torch.from_numpy(table.astype(np.int64)).to(dev)
    t_torch = timed(lambda: (WA * sA.double() + WV * sV.double()[:, tmap]).float(), reps=2, rounds=3)
    copy_GBps = 8 * N * KA / (t_copy[0] * 1e-3) / 1e9
    rec = dict(shape=[N, KA, KV], path=NAMES[path], rowsPerTile=rows, ldsBytes=lds, bytes=nbytes,
               ms_out_of_place=t_out[0], ms_out_of_place_min_max=t_out[1:], ms_in_place=t_in[0], ms_in_place_min_max=t_in[1:],
               GBps_out_of_place=nbytes / (t_out[0] * 1e-3) / 1e9, GBps_in_place=nbytes / (t_in[0] * 1e-3) / 1e9,
               copy_ms=t_copy[0], copy_ms_min_max=t_copy[1:], copy_GBps=copy_GBps,
               share_of_copy_rate_out_of_place=nbytes / (t_out[0] * 1e-3) / 1e9 / copy_GBps, share_of_copy_rate_in_place=nbytes / (t_in[0] * 1e-3) / 1e9 / copy_GBps,
               torch_ms=t_torch[0], torch_ms_min_max=t_torch[1:], torch_over_combine=t_torch[0] / t_in[0])
    print(json.dumps(rec), flush=True)
    del sA, sV, out, ms; torch.cuda.empty_cache()

if not a.no_decode_cost:
    # the benchmark's shape (bench.py: 1000 utterances of 10 s, 1024 states of 4 Gaussians over 39 dimensions, scoring mode 2) with a second model of
    # 64 states of 4 Gaussians over 13 dimensions
    N, KA, KV = 998000, 1024, 64
    gA, gV = dsr.Gmm(**synth.gmm_model(KA, 4, 39, seed=12)), dsr.Gmm(**synth.gmm_model(KV, 4, 13, seed=13))
    table = np.arange(KA, dtype=np.int32) % KV
    ms = M.MultiStream(gA, gV, M.DistribMap({"ds%d" % k: "ds%d" % t for k, t in enumerate(table)}), WA, WV)
    xA, xV = torch.randn((N, 39), device=dev), torch.randn((N, 13), device=dev)
    sA = torch.empty((N, KA), device=dev); sV = torch.empty((N, KV), device=dev)
    L = dsr.load(); p = lambda t: dsr._dev(t); st = lambda: dsr.cur_stream()
    t_a = timed(lambda: dsr.check(L.dsr_gmm_score(gA.h, p(xA), N, 2, p(sA), None, st())))
    t_v = timed(lambda: dsr.check(L.dsr_gmm_score(gV.h, p(xV), N, 2, p(sV), None, st())))
    t_c = timed(lambda: ms.combine(sA, sV, out=sA))
    print(json.dumps(dict(two_model_decode_cost=dict(shape=[N, KA, KV], gmm_audio_ms=t_a[0], gmm_video_ms=t_v[0], combine_in_place_ms=t_c[0],
                                                      added_ms=t_v[0] + t_c[0], added_over_gmm_audio=(t_v[0] + t_c[0]) / t_a[0]))), flush=True)
