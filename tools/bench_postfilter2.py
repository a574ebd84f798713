#!/usr/bin/env python
"""Time the noise suppressors, the binaural masks and the threshold estimators on the GPU:
tools/bench_postfilter2.py [--shape U,T,fftLen[,C]]... [--steps 5] [--out FILE, default profiles/postfilter2.jsonl; the lines are appended]

One JSON line per operator and shape: ms per call (median, events around the call), GB/s on the snapshots the call reads, and for the estimators
frame x candidates per second.  No brute-force (candidate x bin) kernel is kept in the tree, so no ratio against one is printed."""
import argparse
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postfilter2.jsonl"))
    a = ap.parse_args()
    dsr.load(); dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True); times = []
        for _ in range(a.steps):
            e0.record(); fn(); e1.record(); torch.cuda.synchronize(); times.append(e0.elapsed_time(e1))
        times.sort(); return times[len(times) // 2], times[0]

    def emit(**kw):
        s = json.dumps(dict(tool="bench_postfilter2", steps=a.steps, **kw)); print(s)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")

    for sh in a.shape or ["32,1250,256,8", "32,1250,512,2"]:
        f = [int(v) for v in sh.split(",")]; U, T, M = f[:3]; Cn = f[3] if len(f) > 3 else 2; F = M // 2 + 1
        gen = torch.Generator(device=dev); gen.manual_seed(1)
        X = torch.view_as_complex(torch.randn((U, Cn, T, F, 2), dtype=torch.float32, device=dev, generator=gen))
        L, R = X[:, 0].contiguous(), X[:, 1 % Cn].contiguous()
        base = dict(U=U, T=T, fftLen=M)
        inB = U * Cn * T * F * 8; outB = U * T * F * 8

        ss = dsr.SpectralSubtractor(M)
        for c in range(Cn):
            ss.setChannel(0.9)
        st = ss.newState(U, dev)
        ms, mn = timed(lambda: ss.apply(X, st, train_only=True))
        emit(op="specsub_train", C=Cn, ms=round(ms, 3), ms_min=round(mn, 3), x_GBps=round(inB / (ms * 1e-3) / 1e9, 1), **base)
        ss.stopTraining(st); ss.startNoiseSubtraction()
        out = torch.zeros((U, T, F), dtype=torch.complex64, device=dev)
        call = lambda: dsr.check(dsr._lib.dsr_specsub_apply(ss.h, dsr._dev(X), None, U, T, dsr._dev(out), F, 0, dsr._dev(st), dsr.cur_stream()))
        ms, mn = timed(call)
        emit(op="specsub_subtract", C=Cn, ms=round(ms, 3), ms_min=round(mn, 3), x_GBps=round((inB + outB) / (ms * 1e-3) / 1e9, 1), **base)

        w = dsr.WienerFilter(M, False, 0.6); ws = w.newState(U, dev)
        call = lambda: dsr.check(dsr._lib.dsr_wiener_apply(w.h, dsr._dev(L), dsr._dev(R), None, U, T, dsr._dev(out), F, 0, dsr._dev(ws), dsr.cur_stream()))
        ms, mn = timed(call)
        emit(op="wiener", ms=round(ms, 3), ms_min=round(mn, 3), x_GBps=round(3 * outB / (ms * 1e-3) / 1e9, 1), **base)

        for kind in ("kim", "iid"):
            m = dsr.BinaryMask(kind, 0, M, 1.0, 0.5); mst = m.newState(U, dev)
            call = lambda: dsr.check(dsr._lib.dsr_binmask_apply(m.h, dsr._dev(L), dsr._dev(R), None, U, T, dsr._dev(out), F, 0, None, None, dsr._dev(mst), dsr.cur_stream()))
            ms, mn = timed(call)
            emit(op="mask_" + kind, ms=round(ms, 3), ms_min=round(mn, 3), x_GBps=round(3 * outB / (ms * 1e-3) / 1e9, 1), **base)

        for kind, width in (("kim", 0.02), ("iid", 0.02), ("fdiid", 1000.0)):
            e = dsr.ThresholdEstimator(kind, M, 0.0, 0.0, width, dPowerCoeff=1.0 / 15); est = e.newState(U, dev)
            call = lambda: dsr.check(dsr._lib.dsr_thest_run(e.h, dsr._dev(L), dsr._dev(R), None, U, T, dsr._dev(est), dsr.cur_stream()))
            ms, mn = timed(call)
            emit(op="estimator_" + kind, nCand=e.nLoop, ms=round(ms, 3), ms_min=round(mn, 3), x_GBps=round(2 * outB / (ms * 1e-3) / 1e9, 1),
                 frame_cand_per_s=round(U * T * e.nLoop / (ms * 1e-3)), bin_cand_decisions_per_s=round(U * T * e.nLoop * (F - 1) / (ms * 1e-3)), **base)


if __name__ == "__main__":
    main()
