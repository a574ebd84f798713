"""The multi-beam spherical-array apply (dsr_sph_beams) against the single-beam eigenbeam apply (dsr_sph_apply, the DS kind): device-event time
per call for NB = 1, 4, 8, 16 on the VALU and the fp64-MFMA kernel (DSR_SPH_BEAMS_PATH), the bytes the call must move (X once, Y once) with
TB/s and the fraction of 8 TB/s, and for the MFMA kernel the executed fp64 rate (16 padded rows: 8 C 16 flop per frame and bin).  The calls
are timed interleaved, round by round, after a warm-up of every shape; median, minimum and maximum over the rounds are reported.  One JSON
line per (maxOrder, call), appended to profiles/sph_beams.jsonl.

  python tools/bench_sph_beams.py                     # 32 utt x 1250 frames x EigenMike 32 ch, M 256, maxOrder 4 and 8
  python tools/bench_sph_beams.py --shape 32,1250,32,4,256 --rounds 20
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_TBS = 8.0


def run(U, T, Cn, mo, M, rounds, inner, out):
    import torch
    import dsr._capi as dsr
    dsr.load()
    dev = torch.device("cuda:0")
    F = M // 2 + 1

    def handle(kind):
        s = dsr.SphBeamformer(kind, 16000, M, Cn, mo, ratio=1.0 if kind == "HWNC" else None)
        if Cn == 32:
            s.setEigenMikeGeometry()
        else:
            rng = np.random.default_rng(1)
            s.setArrayGeometry(42.0, np.arccos(rng.uniform(-1, 1, Cn)), rng.uniform(0, 2 * np.pi, Cn))
        s.setLookDirection(1.0, 0.3)
        return s
    ds = handle("DS")
    rng = np.random.default_rng(2)
    g = torch.Generator(device=dev); g.manual_seed(1)
    X = torch.randn((U, Cn, T, F, 2), device=dev, generator=g, dtype=torch.float32)
    nf = torch.full((U,), T, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    calls = {}
    y1 = torch.empty((U, T, F, 2), dtype=torch.float32, device=dev)
    calls["apply_ds"] = (lambda: dsr.check(dsr._lib.dsr_sph_apply(ds.h, p(X), p(nf), U, T, p(y1), None, dsr.cur_stream())), 1, None)
    for NB in (1, 4, 5, 8, 16):
        for path in ("valu", "mfma"):
            s = handle("DS")                                                  # a handle per call: its device table stays as uploaded
            for b in range(1, NB):
                s.setBeam(b, float(rng.uniform(0.2, 2.9)), float(rng.uniform(-3, 3)))
            y = torch.empty((U, NB, T, F, 2), dtype=torch.float32, device=dev)

            def call(s=s, y=y, NB=NB, path=path):
                os.environ["DSR_SPH_BEAMS_PATH"] = path
                dsr.check(dsr._lib.dsr_sph_beams(s.h, p(X), p(nf), U, T, NB, p(y), dsr.cur_stream()))
            calls["beams_nb%d_%s" % (NB, path)] = (call, NB, path)
    for fn, _, _ in calls.values():                                          # warm-up: code objects, table uploads
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):                                                  # interleaved: every call once per round
        for k, (fn, _, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record(); e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    os.environ.pop("DSR_SPH_BEAMS_PATH", None)
    for k, (fn, NB, path) in calls.items():
        v = np.array(ms[k]); med = float(np.median(v))
        nbytes = 8.0 * U * T * F * (Cn + NB)
        res = {"U": U, "frames": T, "C": Cn, "maxOrder": mo, "M": M, "call": k, "NB": NB, "kernel": path or "k_sph_apply",
               "ms_median": round(med, 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4), "rounds": rounds, "inner": inner,
               "bytes_moved": nbytes, "tbs": round(nbytes / (med * 1e-3) / 1e12, 3), "frac_of_hbm": round(nbytes / (med * 1e-3) / 1e12 / PEAK_TBS, 3)}
        if path == "mfma":
            res["executed_f64_tflops"] = round(8.0 * Cn * 16 * U * T * F / (med * 1e-3) / 1e12, 2)
        line = json.dumps(res)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="U,T,C,maxOrder,M")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sph_beams.jsonl"))
    a = ap.parse_args()
    todo = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else [(32, 1250, 32, 4, 256), (32, 1250, 32, 8, 256)]
    for shape in todo:
        run(*shape, a.rounds, a.inner, a.out)


if __name__ == "__main__":
    main()
