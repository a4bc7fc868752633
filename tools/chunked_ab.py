#!/usr/bin/env python3
"""Timing of the chunked sampler (flowmse_amd.chunked.enhance_long) on the GPU box: frames/s at batch 8 for recordings of
8 s, 30 s and 60 s, and -- for the 8 s one only (T = 1024, the longest length held to the oracle) -- the existing
single-call path (evaluate.enhance_waveform) on the same box in the same process, arms alternating, median of the
repetitions (as tools/ab.py alternates builds).

    python tools/chunked_ab.py [--reps 7] [--warmup 2] [--N 5] [--batch 8] [--out profiles/chunked_ab.md]

fp32, Euler, synthetic weights and signals, keyed noise.  A repetition is one whole call, samples on the device in, numpy
waveform out (it ends in a device-to-host copy, so the host clock sees finished work).  frames/s counts the recording's
REAL frames (L // 128 + 1), not the Tg = (K - 1) hop + Tc frames the chunks hold: the overlap and the tail padding are
the mode's overhead and show in the rate.  ``--out`` writes the table only; the text around it is written by hand.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--chunk_frames", type=int, default=256)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from flowmse_amd.chunked import enhance_long, plan_chunks
    from flowmse_amd.evaluate import enhance_waveform
    from flowmse_amd.model import VFModel
    from flowmse_amd.util import synth
    assert torch.cuda.is_available(), "chunked_ab.py measures on the GPU; there is no CPU timing"
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape)))
                               for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()
    key, seed = 0x912975D344AF26C6, 7

    def chunked(y):
        return enhance_long(model, y, chunk_frames=a.chunk_frames, overlap_frames=a.overlap_frames, batch=a.batch, N=a.N,
                            noise_key=key, noise_seed=seed)

    def single(y):
        return enhance_waveform(model, y, N=a.N, noise_keys=[key], noise_seed=seed)

    def timed(fn, y):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(y)
        return time.perf_counter() - t0, out

    rows = []
    for seconds in (8, 30, 60):
        n = 1023 * 128 if seconds == 8 else seconds * 16000       # "8 s": 130944 samples = exactly 1024 frames
        y = torch.from_numpy(synth.normal(seconds, 9, (1, n), 0.1)).cuda()
        T = n // 128 + 1
        K, hop, Tg = plan_chunks(T, a.chunk_frames, a.overlap_frames)
        arms = [("chunked", chunked)] + ([("single call", single)] if seconds == 8 else [])
        times = {name: [] for name, _ in arms}
        for r in range(a.warmup + a.reps):                         # arms alternate inside every repetition
            for name, fn in arms:
                dt, out = timed(fn, y)
                assert out.shape == (n,)
                if r >= a.warmup:
                    times[name].append(dt)
        for name, _ in arms:
            med = statistics.median(times[name])
            rows.append((f"{seconds} s", T, name, K if name == "chunked" else 1,
                         K * a.chunk_frames if name == "chunked" else ((T + 63) // 64) * 64,
                         1e3 * med, T / med, 1e3 * min(times[name]), 1e3 * max(times[name])))
            print(f"{seconds:3d} s  T {T:5d}  {name:12s} K {rows[-1][3]:3d}  frames sampled {rows[-1][4]:5d}  median {1e3 * med:8.2f} ms  "
                  f"{T / med:9.1f} frames/s  (min {rows[-1][7]:.2f} max {rows[-1][8]:.2f} ms over {a.reps})", flush=True)
    hop = a.chunk_frames - a.overlap_frames
    print(f"overlap overhead Tc / hop = {a.chunk_frames} / {hop} = {a.chunk_frames / hop:.4f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("| recording | real frames T | arm | sampler rows K | frames sampled | median ms | frames/s | min ms | max ms |\n")
            f.write("|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]} | {r[5]:.2f} | {r[6]:.0f} | {r[7]:.2f} | {r[8]:.2f} |\n")
            f.write(f"\nTc / hop = {a.chunk_frames} / {hop} = {a.chunk_frames / hop:.4f}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
