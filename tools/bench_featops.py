#!/usr/bin/env python
"""Time the scalar feature operators on the GPU: tools/bench_featops.py [--U 256] [--T 1000] [--steps 10] [--out profiles/featops.jsonl]

One JSON line per operator: ms per call (events around the call, median after a warm-up).
  yin      U x T frames of N = 512 samples (the Headset1 frames at shift 160, tiled), threshold 0.5.  Beside the time: the share of frames that
           leave after each chunk of 64 lags; the issue-rate bound -- three fp32 vector instructions per (lag, j) pair of the chunks that were
           evaluated (the chunks the early exit skipped are not counted), at 256 CUs x 4 SIMDs x one wave-instruction per 2 cycles x 2.4 GHz --
           and the fraction of it reached; and the ms of the same difference function d(tau) written with torch on the same device (unfold,
           subtract, square, sum over j, in slices of frames that fit in memory), without the running sum and the search.
  spike    SpikeFilter (tapN 5) and SpikeFilter2 on U utterances of T blocks of 320 samples: ms per call, samples per second, GB/s."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distantspeechrecognition-mirror_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WAVE_INSTR_PER_S = 256 * 4 * 0.5 * 2.4e9          # fp32 vector wave-instructions per second of the whole part


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
    ap.add_argument("--U", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dsr.load(); dev = torch.device("cuda:0")
    U, T = a.U, a.T
    s = np.load(os.path.join(ROOT, "tests", "golden", "Headset1_16k_s16.npy")).astype(np.float32)
    lines = []

    # ---- YIN
    N, shift, W = 512, 160, 256
    nfr = (len(s) - N + shift - 1) // shift
    fr = s[np.arange(N)[None, :] + shift * np.arange(nfr)[:, None]]
    idx = (np.arange(U)[:, None] * 37 + np.arange(T)[None, :]) % nfr                 # every utterance starts elsewhere in the recording
    x = torch.from_numpy(fr).to(dev)[torch.from_numpy(idx).to(dev)].contiguous()     # [U][T][N]
    p, v, c = dsr.yin_pitch(x, 16000, 0.5, return_value=True, return_chunks=True)
    chunks = c.cpu().numpy().reshape(-1)
    voiced = float((p.reshape(-1) > 0).float().mean().item())
    exit_share = [round(float((chunks == k).mean()), 4) for k in range(1, (W - 1) // 64 + 2)]
    pitch = torch.zeros((U, T, 1), dtype=torch.float32, device=dev)

    def call():
        dsr.check(dsr._lib.dsr_yin_pitch_run(dsr._dev(x), None, U, T, N, 16000, 0.5, dsr._dev(pitch), None, None, dsr.cur_stream()))
    ms, ms_min = median_ms(call, a.steps, a.warmup)
    pairs = int(chunks.astype(np.int64).sum()) * 64 * W
    pairs_all = U * T * (W - 1) * W
    bound_ms = 3.0 * (pairs / 64) / WAVE_INSTR_PER_S * 1e3
    xf = x.reshape(U * T, N)
    slice_frames = 2048

    def yard():
        for f0 in range(0, U * T, slice_frames):
            xs = xf[f0:f0 + slice_frames]
            win = xs.unfold(1, W, 1)[:, 1:W]                                          # [F][tau][j] = x[j + tau]
            d = ((xs[:, None, :W] - win) ** 2).sum(-1)
        return d
    try:
        ms2, ms2_min = median_ms(yard, max(2, a.steps // 3), 1)
    except RuntimeError as e:
        ms2 = ms2_min = None; print("yardstick failed: %s" % str(e).splitlines()[0], file=sys.stderr)
    lines.append(dict(tool="bench_featops", op="yin", U=U, T=T, N=N, threshold=0.5, kernel_frames_per_workgroup=dsr.yin_kernel(N), ms=round(ms, 3),
                      ms_min=round(ms_min, 3), frames_per_s=round(U * T / (ms * 1e-3)), voiced_share=round(voiced, 4), exit_share_by_chunk=exit_share,
                      pairs_evaluated=pairs, pairs_without_early_exit=pairs_all, issue_bound_ms=round(bound_ms, 3),
                      issue_bound="3 fp32 vector instructions a pair, 1.2288e12 wave-instructions/s", fraction_of_issue_bound=round(bound_ms / ms, 3),
                      yardstick="torch: unfold, subtract, square, sum over j (d(tau) only), %d frames a slice" % slice_frames,
                      yardstick_ms=None if ms2 is None else round(ms2, 3), yardstick_ms_min=None if ms2 is None else round(ms2_min, 3), steps=a.steps))
    del x, xf, pitch, p, v, c
    torch.cuda.empty_cache()

    # ---- SpikeFilter, SpikeFilter2: U utterances of T blocks of 320 samples, a spike every 50th block
    n = 320
    nb = len(s) // n
    blocks = s[:nb * n].reshape(nb, n).copy()
    blocks[::50, 150] += 20000.0
    idx = (np.arange(U)[:, None] * 11 + np.arange(T)[None, :]) % nb
    xb = torch.from_numpy(blocks).to(dev)[torch.from_numpy(idx).to(dev)].contiguous()
    y = torch.zeros_like(xb)

    def spike():
        dsr.check(dsr._lib.dsr_spike_filter_run(dsr._dev(xb), None, U, T, n, 5, dsr._dev(y), dsr.cur_stream()))
    ms, ms_min = median_ms(spike, a.steps, a.warmup)
    lines.append(dict(tool="bench_featops", op="spike_filter", U=U, T=T, n=n, tapN=5, ms=round(ms, 3), ms_min=round(ms_min, 3),
                      samples_per_s=round(U * T * n / (ms * 1e-3)), gbytes_per_s=round(2 * U * T * n * 4 / (ms * 1e-3) / 1e9, 1), steps=a.steps))
    mslope, cnt = dsr.spike_filter2_state(U, 100.0, dev)

    def spike2():
        mslope.fill_(100.0); cnt.zero_()
        dsr.check(dsr._lib.dsr_spike_filter2_run(dsr._dev(xb), None, U, T, n, 3, 7000.0, 15.0, 0.2, dsr._dev(mslope), dsr._dev(cnt), dsr._dev(y), dsr.cur_stream()))
    ms, ms_min = median_ms(spike2, a.steps, a.warmup)
    lines.append(dict(tool="bench_featops", op="spike_filter2", U=U, T=T, n=n, ms=round(ms, 3), ms_min=round(ms_min, 3),
                      samples_per_s=round(U * T * n / (ms * 1e-3)), ns_per_sample_of_an_utterance=round(ms * 1e6 / (T * n), 2),
                      spikes_per_utterance=round(float(cnt.float().mean().item()), 1), gbytes_per_s=round(2 * U * T * n * 4 / (ms * 1e-3) / 1e9, 1),
                      steps=a.steps))
    for line in lines:
        sj = json.dumps(line); print(sj)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(sj + "\n")


if __name__ == "__main__":
    main()
