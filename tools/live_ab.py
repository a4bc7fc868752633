#!/usr/bin/env python3
"""Timing of live enhancement (flowmse_amd.live.LiveEnhancer) on the GPU box against the chunked file mode it is pinned to.

    python tools/live_ab.py [--parent DIR] [--runs 3] [--reps 3] [--N 5] [--out profiles/live_ab_table.md]

For recordings of 10 s and 60 s at chunk_frames 64 and 256 (overlaps 16 and 32), fp32, Euler, synthetic weights and signals,
keyed noise:

* arm ``long``: ``enhance_long(batch=1)`` on the whole recording, samples on the device in, numpy waveform out.  With
  ``--parent DIR`` it runs in a checkout of the parent commit (its own library, built there); without, in this tree.
* arm ``live``: the same recording fed to one ``LiveEnhancer`` as numpy blocks of 2048 as fast as the calls return, every
  push's output copied to the host, then ``finish()``.

Every arm is a child process of its own (model construction and two warm-up passes are not timed); the processes alternate
long-live-long-live-..., ``--runs`` of each, and inside a process every configuration is timed ``--reps`` times.  Reported
per configuration, over all runs x reps: the median wall time per chunk (whole call / K), the real-time factor (seconds of
audio per second of wall time), and for the live arm the duration of the pushes that sampled a chunk -- the delay from the
arrival of a chunk's last sample to its output, which comes on top of the algorithmic latency of 128 Tc + 382 samples.
The outputs of the two arms are compared bit for bit when both run in this tree.  ``--out`` writes the table only.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = [(10, 64, 16), (10, 256, 32), (60, 64, 16), (60, 256, 32)]
BLOCK = 2048


def arm(name, root, reps, N):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from flowmse_amd.chunked import enhance_long, plan_chunks
    from flowmse_amd.model import VFModel
    from flowmse_amd.util import synth
    assert torch.cuda.is_available(), "live_ab.py measures on the GPU; there is no CPU timing"
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()
    key, seed = 0x912975D344AF26C6, 7
    for seconds, Tc, To in CONFIGS:
        n = seconds * 16000
        y = torch.from_numpy(synth.normal(seconds, 9, (1, n), 0.1))
        peak = y.abs().max().item()
        K = plan_chunks(n // 128 + 1, Tc, To)[0]
        kw = dict(chunk_frames=Tc, overlap_frames=To, N=N)
        if name == "live":
            from flowmse_amd.live import LiveEnhancer, live_plan
            live = LiveEnhancer(model, norm=peak, key=key, seed=seed, **kw)
            blocks = [y[0, i:i + BLOCK].numpy() for i in range(0, n, BLOCK)]
        else:
            yd = y.cuda()
        for r in range(2 + reps):                                   # two warm-up passes
            torch.cuda.synchronize()
            chunk_pushes = []
            t0 = time.perf_counter()
            if name == "live":
                live.reset()
                parts = []
                for b in blocks:
                    before = live_plan(live.samples_in, Tc, To)[0]
                    t1 = time.perf_counter()
                    parts.append(live.push(b))
                    dt = time.perf_counter() - t1
                    if live_plan(live.samples_in, Tc, To)[0] > before:
                        chunk_pushes.append(dt)
                parts.append(live.finish())
                out = np.concatenate(parts)
            else:
                out = enhance_long(model, yd, batch=1, noise_key=key, noise_seed=seed, **kw)
            wall = time.perf_counter() - t0
            assert out.shape == (n,)
            if r >= 2:
                print(json.dumps(dict(arm=name, seconds=seconds, Tc=Tc, To=To, K=K, wall=wall, chunk_pushes=chunk_pushes,
                                      digest=hashlib.sha256(out.tobytes()).hexdigest() if r == 2 else None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("long", "live"), default=None, help="internal: run one arm in this process")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="internal: the tree the arm imports")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (arm long)")
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
        for name in ("long", "live"):
            root = os.path.abspath(a.parent) if (name == "long" and a.parent) else os.path.dirname(HERE)
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--arm", name,
                                "--root", root, "--reps", str(a.reps), "--N", str(a.N)], cwd=root, capture_output=True,
                               text=True)
            if r.returncode != 0:                                   # a failed child ends the tool: nothing more is started
                print(r.stdout[-2000:], r.stderr[-3000:], file=sys.stderr)
                return r.returncode
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            print(f"run {run} arm {name}: done", flush=True)
    lines = ["| recording | Tc / To | K | arm | ms per chunk (median) | min | max | real-time factor | chunk push ms: median | max |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for seconds, Tc, To in CONFIGS:
        digests = {}
        for name in ("long", "live"):
            sel = [r for r in rows if (r["arm"], r["seconds"], r["Tc"]) == (name, seconds, Tc)]
            K = sel[0]["K"]
            per = [1e3 * r["wall"] / K for r in sel]
            pushes = [1e3 * d for r in sel for d in r["chunk_pushes"]]
            digests[name] = {r["digest"] for r in sel if r["digest"] is not None}
            lines.append(f"| {seconds} s | {Tc} / {To} | {K} | {name} | {statistics.median(per):.2f} | {min(per):.2f} | "
                         f"{max(per):.2f} | {seconds / statistics.median(r['wall'] for r in sel):.1f} | "
                         + (f"{statistics.median(pushes):.2f} | {max(pushes):.2f} |" if pushes else "- | - |"))
        if not a.parent:
            assert digests["long"] == digests["live"] and len(digests["live"]) == 1, (seconds, Tc, "the arms' bytes differ")
    text = "\n".join(lines) + f"\n\n{a.runs} alternating runs x {a.reps} repetitions per arm, N = {a.N}, blocks of {BLOCK}" + \
        ("; outputs of the two arms equal bit for bit\n" if not a.parent else f"; arm long in {a.parent}\n")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
