#!/usr/bin/env python3
"""Timing of the trailing-chunk live mode (flowmse_amd.live.LiveEnhancer(hop_frames=...)) against the default schedule.

    python tools/live_trailing_ab.py --parent DIR [--runs 3] [--N 5] [--seconds 30] [--out table.md] [--raw runs.jsonl]

One 30 s synthetic stream in numpy blocks of 512 samples, pushed to one ``LiveEnhancer`` as fast as the calls return (not paced
at 16 kHz), every push's output copied to the host, then ``finish()``; full network, synthetic weights, Euler, keyed noise,
fp32 and bf16.  Arms, all at ``chunk_frames = 64``:

* ``parent``: ``LiveEnhancer(chunk_frames=64, overlap_frames=16)`` in a checkout of the parent commit (``--parent DIR``, its own
  library built there).
* ``default``: the same object in this tree -- ``live.py`` changed, so the default path is held against the parent's spread.
* ``H32``, ``H16``, ``H8``: ``hop_frames`` 32, 16, 8 with ``fade_frames = H / 4`` in this tree.

Every arm is a child process of its own (model construction and one warm-up pass over the first 5 s per precision are not
timed); the processes alternate parent-default-H32-H16-H8, ``--runs`` times.  Per arm and precision the table has the
algorithmic latency, the duration of the pushes that completed a chunk (median and worst over all runs), the wall time per chunk
(median over the runs, and their range), the real-time factor of every run, and latency + worst push: what a user hears.
``--raw`` keeps every run's figures as JSON lines.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK, TC, TO = 512, 64, 16
ARMS = ["parent", "default", "H32", "H16", "H8"]
PRECISIONS = ["fp32", "bf16"]


def arm(name, root, N, seconds):
    sys.path.insert(0, root)
    import torch
    from flowmse_amd.live import LiveEnhancer, latency_samples, live_plan
    from flowmse_amd.model import VFModel
    from flowmse_amd.util import synth
    assert torch.cuda.is_available(), "live_trailing_ab.py measures on the GPU; there is no CPU timing"
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()
    n = seconds * 16000
    y = synth.normal(seconds, 9, (n,), 0.1)
    blocks = [y[i:i + BLOCK] for i in range(0, n, BLOCK)]
    if name in ("parent", "default"):
        geo, plan = dict(overlap_frames=TO), dict(To=TO)
        latency = latency_samples(TC)
    else:
        H = int(name[1:])
        geo = plan = dict(hop_frames=H, fade_frames=H // 4)
        latency = latency_samples(TC, **plan)
    for precision in PRECISIONS:
        model.dnn.set_precision(precision)
        live = LiveEnhancer(model, norm=float(abs(y).max()), key=0x912975D344AF26C6, seed=7, chunk_frames=TC, N=N, **geo)
        for timed in (False, True):
            live.reset()
            use = blocks if timed else blocks[:5 * 16000 // BLOCK]
            torch.cuda.synchronize()
            pushes, total = [], 0
            t0 = time.perf_counter()
            for b in use:
                before = live_plan(live.samples_in, TC, **plan)[0]
                t1 = time.perf_counter()
                total += live.push(b).shape[0]
                dt = time.perf_counter() - t1
                if live_plan(live.samples_in, TC, **plan)[0] > before:
                    pushes.append(dt)
            total += live.finish().shape[0]
            wall = time.perf_counter() - t0
            assert total == sum(len(b) for b in use)
            if timed:
                K = live_plan(n, TC, finished=True, **plan)[0]
                print(json.dumps(dict(arm=name, precision=precision, latency=latency, K=K, wall=wall, seconds=seconds,
                                      push_median=statistics.median(pushes), push_max=max(pushes), pushes=len(pushes))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS, default=None, help="internal: run one arm in this process")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="internal: the tree the arm imports")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (arm parent)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--seconds", type=int, default=30)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child process in seconds")
    ap.add_argument("--out", default=None)
    ap.add_argument("--raw", default=None)
    a = ap.parse_args()
    if a.arm:
        arm(a.arm, os.path.abspath(a.root), a.N, a.seconds)
        return 0
    arms = [x for x in ARMS if x != "parent" or a.parent]
    rows = []
    for run in range(a.runs):
        for name in arms:
            root = os.path.abspath(a.parent) if name == "parent" else os.path.dirname(HERE)
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--arm", name,
                                "--root", root, "--N", str(a.N), "--seconds", str(a.seconds)], cwd=root, capture_output=True,
                               text=True)
            if r.returncode != 0:                                   # a failed child ends the tool: nothing more is started
                print(r.stdout[-2000:], r.stderr[-3000:], file=sys.stderr)
                return r.returncode
            rows += [dict(json.loads(line), run=run) for line in r.stdout.splitlines() if line.startswith("{")]
            print(f"run {run} arm {name}: done", flush=True)
    if a.raw:
        with open(a.raw, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    lines = ["| precision | arm | K | latency: samples | s | chunk push ms: median | worst | ms per chunk: median (min .. max of runs) | "
             "real-time factor per run | latency + worst push, s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for precision in PRECISIONS:
        for name in arms:
            sel = [r for r in rows if (r["arm"], r["precision"]) == (name, precision)]
            per = [1e3 * r["wall"] / r["K"] for r in sel]
            worst = max(r["push_max"] for r in sel)
            lat = sel[0]["latency"]
            lines.append(f"| {precision} | {name} | {sel[0]['K']} | {lat} | {lat / 16000:.3f} | "
                         f"{1e3 * statistics.median(r['push_median'] for r in sel):.2f} | {1e3 * worst:.2f} | "
                         f"{statistics.median(per):.2f} ({min(per):.2f} .. {max(per):.2f}) | "
                         + " ".join(f"{r['seconds'] / r['wall']:.1f}" for r in sel) + f" | {lat / 16000 + worst:.3f} |")
    text = "\n".join(lines) + f"\n\n{a.runs} alternating runs per arm, N = {a.N}, {a.seconds} s in blocks of {BLOCK}" + \
        (f"; arm parent in {os.path.basename(os.path.abspath(a.parent))}\n" if a.parent else "; no parent arm\n")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
