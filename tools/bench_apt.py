#!/usr/bin/env python
"""Time all-pass transform estimation and the mean transforms on the GPU: tools/bench_apt.py [--shape S,G,L,nSub,leaves]... [--steps 5]
[--warmup 2] [--out FILE]

Two JSON lines per shape, one for the bilinear transform and one for SLAPT (S speakers, G Gaussians of nSub sub-features of L spread evenly
over `leaves` regression classes, a power of two: the nodes leaves .. 2 leaves - 1 of a complete tree; every leaf has enough frames, so every
(speaker, leaf) is searched at itself; CepstraOnly bias; statistics of means warped with alpha = 0.1):
  ms_estimate    the whole dsr_apt_estimate (host tree, uploads, the rounds of kernels with their copies back, the searches), median of --steps
  rounds         launches of each kernel in one estimate (the longest search);  evals  trial points of all searches together
  ms_matrix      k_apt_matrix summed over the rounds (events inside the library);  ms_lhood  k_apt_lhood likewise;  ms_apply  k_apt_apply of
                 adapt_all (its k_apt_matrix launch is not in it)
  gflops_matrix  2 x 299 x 299 x 3/4 fp64 flop a Cauchy product (the mean range of j), L - 2 of them a trial point and 48 more for SLAPT
  gflops_lhood   2 L (D + bias size) flop a Gaussian and trial point for the two transform passes
  ms_mllr_estimate   dsr_mllr_estimate for the same model and statistics: the yardstick, a closed-form solve instead of a search"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import torch
    import dsr._capi as dsr
    from tests import apt_np as P
    from tests import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="S,G,subFeatLen,nSubFeat,leaves")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in (a.shape or ["1,4096,13,3,1", "32,4096,13,3,4", "128,4096,13,3,8"])]
    dsr.load()
    med = lambda v: sorted(v)[len(v) // 2]                                            # noqa: E731
    lines = []
    for S, G, L, nSub, NL in shapes:
        assert NL >= 1 and NL & (NL - 1) == 0 and G % 16 == 0
        D = L * nSub
        gm = synth.gmm_model(G // 16, 16, D, seed=12)
        rng = np.random.default_rng(3)
        gm["mean"] = (rng.standard_normal((G, nSub, L)) / (1.0 + np.arange(L))[None, None, :] ** 2).reshape(G, D).astype(np.float32)
        g = dsr.Gmm(**gm)
        classes = (NL + np.arange(G) % NL).astype(np.uint16); g.set_reg_classes(classes)
        c = rng.uniform(1.0, 30.0, (S, G))
        warped = P.transform(P.matrix(P.RAPT, [0.1], L), gm["mean"], nSub).astype(np.float64)
        sumO = c[:, :, None] * (warped[None] + 0.05 * rng.standard_normal((S, G, D)))
        hm = dsr.Mllr(g, S)
        for s in range(S):
            hm.set_stats(s, c=c[s], sumO=sumO[s])
        wm = []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); hm.estimate(0.0); dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                wm.append(dt)
        del hm
        for kind, name in ((dsr.APT_RAPT, "BLT"), (dsr.APT_SLAPT, "SLAPT")):
            h = dsr.Apt(g, S, kind, L, nSub, 1); h.set_timing(True)
            for s in range(S):
                h.set_stats(s, c=c[s], sumO=sumO[s])
            wall, mt, lh, ap_ = [], [], [], []
            for i in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); h.estimate(0.0); dt = (time.perf_counter() - t0) * 1e3
                out = h.adapt_all(); torch.cuda.synchronize()
                if i >= a.warmup:
                    ms = h.kernel_ms(); wall.append(dt); mt.append(ms[0]); lh.append(ms[1]); ap_.append(ms[2])
            evals = sum(len(h.trace(int(s), int(node))[0]) for s, node, _ in h.plan())
            products = (L - 2) + (48 if kind == dsr.APT_SLAPT else 0)
            f_matrix = 2.0 * 299 * 299 * 0.75 * products * evals
            f_lhood = 2.0 * L * (D + L) * (G / NL) * evals
            conf = [float(h.get_params(s, NL)[0][0]) for s in range(min(S, 3))]
            lines.append(dict(tool="bench_apt", kind=name, S=S, G=G, subFeatLen=L, nSubFeat=nSub, leaves=NL, ms_estimate=round(med(wall), 3), rounds=h.rounds(),
                              evals=evals, ms_matrix=round(med(mt), 3), ms_lhood=round(med(lh), 3), ms_apply=round(med(ap_), 4),
                              gflops_matrix=round(f_matrix / (med(mt) * 1e-3) / 1e9, 1), gflops_lhood=round(f_lhood / (med(lh) * 1e-3) / 1e9, 1),
                              ms_mllr_estimate=round(med(wm), 3), conf=conf, out_checksum=round(float(out.double().sum().item()), 3)))
            del h, out
        del g
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
