#!/usr/bin/env python3
"""Timing of the live pool (flowmse_amd.livepool.LivePool) on the GPU box against one LiveEnhancer per stream.

    python tools/livepool_ab.py [--parent DIR] [--runs 3] [--reps 1] [--N 5] [--out profiles/livepool_ab_table.md]

Eight mono sessions of 30 s each, pushed round-robin in blocks of 2048 as fast as the calls return, at chunk_frames 256 and
64 (overlaps 32 and 16), fp32, Euler, synthetic weights and signals, keyed noise:

* arm ``each``: eight ``LiveEnhancer`` s, one per session; a round pushes one block to each and copies what it returns to
  the host.  With ``--parent DIR`` it runs in a checkout of the parent commit (its own library, built there); without, in
  this tree.
* arm ``pool``: one ``LivePool(width=8)`` with the eight sessions; a round pushes one block to each and calls ``step()``
  once, the outputs copied to the host.

Every arm is a child process of its own (model construction and one warm-up pass are not timed); the processes alternate
each-pool-each-pool-..., ``--runs`` of each.  Reported per geometry, over all runs x reps: the aggregate real-time factor
(seconds of audio of all sessions per second of wall time), the median and the worst wall time of the rounds that sampled
a chunk (what a caller waits for its samples beyond the algorithmic latency), for the pool the share of filler rows, and
whether every pool run beat every run of the other arm.  The outputs are hashed and the digests compared within an arm (the
runs of one arm must give the same bytes); across the arms they differ by design, width 1 against width 8.  ``--out`` writes
the table only.
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
CONFIGS = [(256, 32), (64, 16)]
SESSIONS, SECONDS, BLOCK = 8, 30, 2048


def arm(name, root, reps, N):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from flowmse_amd.model import VFModel
    from flowmse_amd.util import synth
    assert torch.cuda.is_available(), "livepool_ab.py measures on the GPU; there is no CPU timing"
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()
    seed, n = 7, SECONDS * 16000
    ys = [synth.normal(40 + i, 9, (n,), 0.1) for i in range(SESSIONS)]
    peaks = [float(np.abs(y).max()) for y in ys]
    keys = [0x912975D344AF26C6 + i for i in range(SESSIONS)]
    for Tc, To in CONFIGS:
        kw = dict(chunk_frames=Tc, overlap_frames=To, N=N)
        for r in range(1 + reps):                                   # one warm-up pass
            if name == "each":
                from flowmse_amd.live import LiveEnhancer
                lives = [LiveEnhancer(model, norm=peaks[i], key=keys[i], seed=seed, **kw) for i in range(SESSIONS)]
            else:
                from flowmse_amd.livepool import LivePool
                pool = LivePool(model, width=SESSIONS, seed=seed, **kw)
                sess = [pool.open(keys[i], peaks[i]) for i in range(SESSIONS)]
                index = {s: i for i, s in enumerate(sess)}
            parts = [[] for _ in range(SESSIONS)]
            sampled, fillers, rows = [], 0, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for at in list(range(0, n, BLOCK)) + [None]:           # None: the round that finishes the sessions
                t1 = time.perf_counter()
                if name == "each":
                    got = 0
                    for i, live in enumerate(lives):
                        out = live.push(ys[i][at:at + BLOCK]) if at is not None else live.finish()
                        got += out.shape[0]
                        parts[i].append(out)
                else:
                    for i, s in enumerate(sess):
                        s.push(ys[i][at:at + BLOCK]) if at is not None else s.finish()
                    got = 0
                    for s, out in pool.step():
                        got += out.shape[1]
                        parts[index[s]].append(out[0])
                    fillers += sum(pool.last_step["fillers"].values())
                    rows += pool.last_step["rows"]
                if got:
                    sampled.append(time.perf_counter() - t1)
            wall = time.perf_counter() - t0
            outs = [np.concatenate(p) for p in parts]
            assert all(o.shape == (n,) for o in outs)
            if r >= 1:
                digest = hashlib.sha256(b"".join(o.tobytes() for o in outs)).hexdigest() if r == 1 else None
                print(json.dumps(dict(arm=name, Tc=Tc, To=To, wall=wall, sampled=sampled, fillers=fillers, rows=rows,
                                      digest=digest)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("each", "pool"), default=None, help="internal: run one arm in this process")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="internal: the tree the arm imports")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (arm each)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280, help="time limit of one child process in seconds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        arm(a.arm, os.path.abspath(a.root), a.reps, a.N)
        return 0
    rows = []
    for run in range(a.runs):
        for name in ("each", "pool"):
            root = os.path.abspath(a.parent) if (name == "each" and a.parent) else os.path.dirname(HERE)
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--arm", name,
                                "--root", root, "--reps", str(a.reps), "--N", str(a.N)], cwd=root, capture_output=True,
                               text=True)
            if r.returncode != 0:                                   # a failed child ends the tool: nothing more is started
                print(r.stdout[-2000:], r.stderr[-3000:], file=sys.stderr)
                return r.returncode
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            print(f"run {run} arm {name}: done", flush=True)
    audio = SESSIONS * SECONDS
    lines = ["| Tc / To | arm | real-time factor (median) | min | max | sampling round ms: median | worst | filler share |",
             "|---|---|---|---|---|---|---|---|"]
    notes = []
    for Tc, To in CONFIGS:
        walls = {}
        for name in ("each", "pool"):
            sel = [r for r in rows if (r["arm"], r["Tc"]) == (name, Tc)]
            walls[name] = [r["wall"] for r in sel]
            rounds = [1e3 * d for r in sel for d in r["sampled"]]
            digests = {r["digest"] for r in sel if r["digest"] is not None}
            assert len(digests) == 1, (name, Tc, "the runs of one arm gave different bytes")
            share = sum(r["fillers"] for r in sel) / max(sum(r["fillers"] + r["rows"] for r in sel), 1)
            lines.append(f"| {Tc} / {To} | {name} | {audio / statistics.median(walls[name]):.1f} | {audio / max(walls[name]):.1f} | "
                         f"{audio / min(walls[name]):.1f} | {statistics.median(rounds):.2f} | {max(rounds):.2f} | "
                         + (f"{share:.3f} |" if name == "pool" else "- |"))
        ratio = statistics.median(walls["each"]) / statistics.median(walls["pool"])
        every = max(walls["pool"]) < min(walls["each"])
        notes.append(f"{Tc} / {To}: pool against each {ratio:.2f}x in aggregate rate; every pool run "
                     f"{'beat' if every else 'did NOT beat'} every run of the other arm")
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + \
        f"\n\n{SESSIONS} mono sessions of {SECONDS} s, blocks of {BLOCK}, {a.runs} alternating runs x {a.reps} repetitions per arm, " \
        f"N = {a.N}" + (f"; arm each in {a.parent}\n" if a.parent else "; both arms in this tree\n")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
