#!/usr/bin/env python
"""Time MLLR estimation and the mean transforms on the GPU: tools/bench_mllr.py [--shape S,G,D,leaves]... [--steps 5] [--warmup 2] [--out FILE]

One JSON line per shape (S speakers, G Gaussians of dimension D spread evenly over `leaves` regression classes, a power of two: the classes are
the nodes leaves .. 2 leaves - 1 of a complete tree; every leaf has enough frames, so every (speaker, leaf) is solved at itself):
  ms_estimate    the whole dsr_mllr_estimate (host tree and sort, uploads, kernels, back-off, trees filled), median of --steps calls
  ms_stats       k_mllr_stats + k_mllr_reduce (events inside the library);  ms_solve: k_mllr_solve;  ms_apply: k_mllr_apply of adapt_all
  tflops_stats   2 D ((D + 1)(D + 2) / 2 + D + 1) G S fp64 flop over ms_stats (the useful flop of the contraction; the reduction over the tree's
                 nodes is in the time, not in the count)
  solves_per_s   S leaves D symmetric eigen-solves of order D + 1 over ms_solve
  ms_torch_stats / ms_torch_solve   the same leaf statistics by torch.einsum in fp64 and the solves by torch.linalg.pinv(rcond = 1e-7) @ z --
                 yardsticks, not reference results (the internal nodes are left out of the torch side)"""
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
    from tests import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="S,G,D,leaves")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in (a.shape or ["1,4096,39,1", "32,4096,39,4", "128,4096,39,8"])]
    dsr.load(); dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]                                            # noqa: E731
    lines = []
    for S, G, D, L in shapes:
        assert L >= 1 and L & (L - 1) == 0 and G % 16 == 0
        gm = synth.gmm_model(G // 16, 16, D, seed=12); g = dsr.Gmm(**gm)
        classes = (L + np.arange(G) % L).astype(np.uint16); g.set_reg_classes(classes)
        rng = np.random.default_rng(3)
        c = rng.uniform(1.0, 30.0, (S, G)); sumO = c[:, :, None] * (gm["mean"][None].astype(np.float64) + 0.5 * rng.standard_normal((S, G, D)))
        h = dsr.Mllr(g, S); h.set_timing(True)
        for s in range(S):
            h.set_stats(s, c=c[s], sumO=sumO[s])
        wall, st, so, ap_ = [], [], [], []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); h.estimate(0.0); dt = (time.perf_counter() - t0) * 1e3
            out = h.adapt_all(); torch.cuda.synchronize()
            if i >= a.warmup:
                ms = h.kernel_ms(); wall.append(dt); st.append(ms[0]); so.append(ms[1]); ap_.append(ms[2])
        n = D + 1
        # torch yardsticks: the leaf statistics and the solves
        cd = torch.from_numpy(c).to(dev); sd = torch.from_numpy(sumO).to(dev); iv = torch.from_numpy(gm["ivar"]).to(dev).double()
        xi = torch.cat([torch.from_numpy(gm["mean"]).to(dev).double(), torch.ones((G, 1), device=dev, dtype=torch.float64)], dim=1)
        sel = [torch.from_numpy(np.nonzero(classes == L + l)[0]).to(dev) for l in range(L)]

        def torch_stats():
            Gs, Zs = [], []
            for ix in sel:
                w = cd[:, ix, None] * iv[None, ix]                                     # [S][g][D]
                Gs.append(torch.einsum("sgi,gp,gq->sipq", w, xi[ix], xi[ix])); Zs.append(torch.einsum("sgi,gp->sip", sd[:, ix] * iv[None, ix], xi[ix]))
            return Gs, Zs

        def torch_solve(Gs, Zs):
            return [(torch.linalg.pinv(Gm, rcond=1e-7, hermitian=True) @ Zm[..., None])[..., 0] for Gm, Zm in zip(Gs, Zs)]
        Gs, Zs = torch_stats(); torch_solve(Gs, Zs); torch.cuda.synchronize()
        t1, t2 = [], []
        for _ in range(max(2, a.steps // 2)):
            t0 = time.perf_counter(); Gs, Zs = torch_stats(); torch.cuda.synchronize(); t1.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); Wt = torch_solve(Gs, Zs); torch.cuda.synchronize(); t2.append((time.perf_counter() - t0) * 1e3)
        Wd = h.transform(0, L); dev_vs_torch = float(np.abs(Wd - Wt[0][0].cpu().numpy()).max())
        flop = 2.0 * D * (n * (n + 1) / 2 + n) * G * S
        lines.append(dict(tool="bench_mllr", S=S, G=G, dimN=D, leaves=L, ms_estimate=round(med(wall), 3), ms_stats=round(med(st), 3), ms_solve=round(med(so), 3),
                          ms_apply=round(med(ap_), 4), tflops_stats=round(flop / (med(st) * 1e-3) / 1e12, 3), solves_per_s=round(S * L * D / (med(so) * 1e-3)),
                          ms_torch_stats=round(med(t1), 3), ms_torch_solve=round(med(t2), 3), max_abs_W_diff_vs_torch=dev_vs_torch,
                          out_checksum=round(float(out.double().sum().item()), 3)))
        del h, g, cd, sd, Gs, Zs, Wt, out
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
