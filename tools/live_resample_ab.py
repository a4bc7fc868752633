#!/usr/bin/env python3
"""Timing of live enhancement at 48 kHz (``LiveEnhancer(input_rate=48000, output_rate="input")``) on the GPU box against
the 16 kHz live push it is built around.

    python tools/live_resample_ab.py [--parent DIR] [--runs 3] [--reps 3] [--N 5] [--out profiles/live_resample_ab_table.md]

The protocol of tools/live_ab.py: recordings of 10 s and 60 s at chunk_frames 64 and 256 (overlaps 16 and 32), fp32, Euler,
synthetic weights and signals, keyed noise.  The recording is synthetic at 48 kHz; the 16 kHz arm gets what
``resample(y, 48000, 16000)`` makes of it.

* arm ``live16``: the 16 kHz recording as numpy blocks of 2048 pushed to one ``LiveEnhancer`` with no rate arguments.  With
  ``--parent DIR`` it runs in a checkout of the parent commit (its own library, built there); without, in this tree.
* arm ``live48``: the 48 kHz recording as numpy blocks of 6144 (2048 at 16 kHz scaled to the rate) pushed to one
  ``LiveEnhancer(input_rate=48000, output_rate="input")`` in this tree.

Every push is timed from the call to the end of a device synchronisation after it, in both arms, and counted as a chunk
push if it sampled a chunk (``live_plan`` on the 16 kHz count) and as an idle push otherwise: an idle push at 16 kHz is the
block's copy to the device; at 48 kHz it is that copy, the input resampler's launch and its buffer moves.  One child
process per arm and run (model construction and two warm-up passes per configuration untimed), alternating
live16-live48-..., ``--runs`` of each, ``--reps`` timed passes per configuration inside each.  ``--out`` writes the table."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = [(10, 64, 16), (10, 256, 32), (60, 64, 16), (60, 256, 32)]
BLOCK, RATE = 2048, 48000


def arm(name, root, reps, N):
    sys.path.insert(0, root)
    import torch
    from flowmse_amd.live import LiveEnhancer, live_plan
    from flowmse_amd.model import VFModel
    from flowmse_amd.resample import resample
    from flowmse_amd.util import synth
    assert torch.cuda.is_available(), "live_resample_ab.py measures on the GPU; there is no CPU timing"
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()
    key, seed = 0x912975D344AF26C6, 7
    for seconds, Tc, To in CONFIGS:
        n = seconds * RATE
        y = torch.from_numpy(synth.normal(seconds, 9, (1, n), 0.1))
        y16 = resample(y.cuda(), RATE, 16000).cpu()
        peak = y16.abs().max().item()
        kw = dict(chunk_frames=Tc, overlap_frames=To, N=N)
        if name == "live48":
            live = LiveEnhancer(model, norm=peak, key=key, seed=seed, input_rate=RATE, output_rate="input", **kw)
            blocks = [y[0, i:i + BLOCK * 3].numpy() for i in range(0, n, BLOCK * 3)]
            count16 = lambda: live._rs_in.samples_out                          # noqa: E731  the 16 kHz samples final so far
        else:
            live = LiveEnhancer(model, norm=peak, key=key, seed=seed, **kw)
            blocks = [y16[0, i:i + BLOCK].numpy() for i in range(0, y16.size(1), BLOCK)]
            count16 = lambda: live.samples_in                                   # noqa: E731
        for r in range(2 + reps):                                   # two warm-up passes
            live.reset()
            torch.cuda.synchronize()
            chunk, idle, total = [], [], 0
            for b in blocks:
                before = live_plan(count16(), Tc, To)[0]
                t1 = time.perf_counter()
                total += live.push(b).shape[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t1
                (chunk if live_plan(count16(), Tc, To)[0] > before else idle).append(dt)
            total += live.finish().shape[0]
            assert total == (n if name == "live48" else y16.size(1))
            if r >= 2:
                print(json.dumps(dict(arm=name, seconds=seconds, Tc=Tc, chunk=chunk, idle=idle)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("live16", "live48"), default=None, help="internal: run one arm in this process")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="internal: the tree the arm imports")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (arm live16)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child process in seconds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        arm(a.arm, os.path.abspath(a.root), a.reps, a.N)
        return 0
    rows = []
    for run in range(a.runs):
        for name in ("live16", "live48"):
            root = os.path.abspath(a.parent) if (name == "live16" and a.parent) else os.path.dirname(HERE)
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--arm", name,
                                "--root", root, "--reps", str(a.reps), "--N", str(a.N)], cwd=root, capture_output=True,
                               text=True)
            if r.returncode != 0:                                   # a failed child ends the tool: nothing more is started
                print(r.stdout[-2000:], r.stderr[-3000:], file=sys.stderr)
                return r.returncode
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            print(f"run {run} arm {name}: done", flush=True)
    lines = ["| recording | Tc | arm | chunk pushes | chunk push ms: median | min | max | idle pushes | idle push ms: median | "
             "min | max |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for seconds, Tc, _ in CONFIGS:
        for name in ("live16", "live48"):
            sel = [r for r in rows if (r["arm"], r["seconds"], r["Tc"]) == (name, seconds, Tc)]
            c = [1e3 * d for r in sel for d in r["chunk"]]
            i = [1e3 * d for r in sel for d in r["idle"]]
            lines.append(f"| {seconds} s | {Tc} | {name} | {len(c)} | {statistics.median(c):.3f} | {min(c):.3f} | {max(c):.3f} | "
                         f"{len(i)} | {statistics.median(i):.3f} | {min(i):.3f} | {max(i):.3f} |")
        # the spread between passes: the median chunk push of every timed pass
        for name in ("live16", "live48"):
            per = [1e3 * statistics.median(r["chunk"]) for r in rows if (r["arm"], r["seconds"], r["Tc"]) == (name, seconds, Tc)]
            lines.append(f"| {seconds} s | {Tc} | {name}: per-pass medians | {len(per)} | {statistics.median(per):.3f} | "
                         f"{min(per):.3f} | {max(per):.3f} | | | | |")
    text = "\n".join(lines) + f"\n\n{a.runs} alternating runs x {a.reps} repetitions per arm, N = {a.N}, blocks of {BLOCK} at " \
        f"16 kHz and {3 * BLOCK} at 48 kHz" + (f"; arm live16 in {a.parent}\n" if a.parent else "; both arms in this tree\n")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
