#!/usr/bin/env python3
"""Timing of the live pool at 48 kHz in and out (sessions opened with ``input_rate=48000, output_rate="input"``) on the GPU box
against the arrangement it replaces: a 16 kHz ``LivePool`` with a ``StreamResampler`` per channel before and behind it.

    python tools/livepool_resample_ab.py [--parent DIR] [--runs 3] [--reps 1] [--N 5] [--out profiles/livepool_resample_ab_table.md]

Eight mono sessions of 30 s each at 48 kHz, pushed round-robin in numpy blocks of 6144 as fast as the calls return, one
``step()`` per round, at chunk_frames 256 and 64 (overlaps 32 and 16), fp32, Euler, synthetic weights and signals, keyed noise,
``LivePool(width=8)`` in both arms:

* arm ``parent``: sixteen ``StreamResampler`` s around eight 16 kHz sessions.  A round pushes one block through each session's
  in-resampler (one ``flowse_resample_poly_window`` launch each) into the session, calls ``step()`` once and pushes what each
  session returns through its out-resampler; the outputs are copied to the host.  With ``--parent DIR`` it runs in a checkout of
  the parent commit (its own library, built there); without, in this tree, whose 16 kHz sessions and ``StreamResampler`` make
  the calls they made before.
* arm ``pool``: the eight sessions opened at 48 kHz in and out; a round pushes one block to each and calls ``step()`` once (one
  ``flowse_resample_poly_window_rows`` launch in, one out), the outputs copied to the host.

Every arm is a child process of its own (model construction and one warm-up pass are not timed); the processes alternate
parent-pool-parent-pool-..., ``--runs`` of each.  Reported per geometry, over all runs x reps: the aggregate real-time factor
(seconds of audio of all sessions per second of wall time), the median and the worst wall time of a round, of the rounds that
sampled a chunk and of those that did not, the spread of both arms, and whether every pool run beat every parent run.  The
outputs are hashed: all runs of BOTH arms must give the same bytes (the pool's contract).  ``--out`` writes the table only.
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
SESSIONS, SECONDS, RATE, BLOCK = 8, 30, 48000, 6144


def arm(name, root, reps, N):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from flowmse_amd.livepool import LivePool
    from flowmse_amd.model import VFModel
    from flowmse_amd.resample import StreamResampler, resample
    from flowmse_amd.util import synth
    assert torch.cuda.is_available(), "livepool_resample_ab.py measures on the GPU; there is no CPU timing"
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()
    seed, n = 7, SECONDS * RATE
    ys = [synth.normal(40 + i, 9, (n,), 0.1) for i in range(SESSIONS)]
    peaks = [resample(torch.from_numpy(y)[None].cuda(), RATE, 16000).abs().max().item() for y in ys]   # of the 16 kHz signals
    keys = [0x912975D344AF26C6 + i for i in range(SESSIONS)]
    for Tc, To in CONFIGS:
        for r in range(1 + reps):                                   # one warm-up pass
            pool = LivePool(model, width=SESSIONS, seed=seed, chunk_frames=Tc, overlap_frames=To, N=N)
            if name == "parent":
                sess = [pool.open(keys[i], peaks[i]) for i in range(SESSIONS)]
                front = [StreamResampler(RATE, 16000, "cuda") for _ in range(SESSIONS)]
                behind = [StreamResampler(16000, RATE, "cuda") for _ in range(SESSIONS)]
            else:
                sess = [pool.open(keys[i], peaks[i], input_rate=RATE, output_rate="input") for i in range(SESSIONS)]
            index = {s: i for i, s in enumerate(sess)}
            parts = [[] for _ in range(SESSIONS)]
            sampled, idle = [], []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for at in list(range(0, n, BLOCK)) + [None]:           # None: the round that finishes the sessions
                t1 = time.perf_counter()
                got = 0
                if name == "parent":
                    for i, s in enumerate(sess):
                        if at is not None:
                            s.push(front[i].push(ys[i][at:at + BLOCK], as_tensor=True))
                        else:
                            s.push(front[i].finish(as_tensor=True))
                            s.finish()
                    for s, out in pool.step(as_tensor=True):
                        i = index[s]
                        back = [behind[i].push(out[0], as_tensor=True)] + ([behind[i].finish(as_tensor=True)] if s.closed else [])
                        out = torch.cat(back).cpu().numpy()
                        got += out.shape[0]
                        parts[i].append(out)
                else:
                    for i, s in enumerate(sess):
                        s.push(ys[i][at:at + BLOCK]) if at is not None else s.finish()
                    for s, out in pool.step():
                        got += out.shape[1]
                        parts[index[s]].append(out[0])
                (sampled if got else idle).append(time.perf_counter() - t1)
            wall = time.perf_counter() - t0
            outs = [np.concatenate(p)[:n] for p in parts]           # arm parent: the trim its caller does by hand
            assert all(o.shape == (n,) for o in outs)
            if r >= 1:
                digest = hashlib.sha256(b"".join(o.tobytes() for o in outs)).hexdigest() if r == 1 else None
                print(json.dumps(dict(arm=name, Tc=Tc, To=To, wall=wall, sampled=sampled, idle=idle, digest=digest,
                                      launches=pool.stats.get("resample_launches"))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("parent", "pool"), default=None, help="internal: run one arm in this process")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="internal: the tree the arm imports")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (arm parent)")
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
        for name in ("parent", "pool"):
            root = os.path.abspath(a.parent) if (name == "parent" and a.parent) else os.path.dirname(HERE)
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--arm", name,
                                "--root", root, "--reps", str(a.reps), "--N", str(a.N)], cwd=root, capture_output=True,
                               text=True)
            if r.returncode != 0:                                   # a failed child ends the tool: nothing more is started
                print(r.stdout[-2000:], r.stderr[-3000:], file=sys.stderr)
                return r.returncode
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            print(f"run {run} arm {name}: done", flush=True)
    audio = SESSIONS * SECONDS
    ms = lambda v: f"{1e3 * statistics.median(v):.2f} | {1e3 * max(v):.2f}"
    lines = ["| Tc / To | arm | real-time factor (median) | min | max | round ms: median | worst | sampling round ms: median | worst "
             "| other round ms: median | worst | resampler launches |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for Tc, To in CONFIGS:
        walls = {}
        digests = {r["digest"] for r in rows if r["Tc"] == Tc and r["digest"] is not None}
        assert len(digests) == 1, (Tc, "the runs of the two arms gave different bytes")
        for name in ("parent", "pool"):
            sel = [r for r in rows if (r["arm"], r["Tc"]) == (name, Tc)]
            walls[name] = [r["wall"] for r in sel]
            sampled, idle = [d for r in sel for d in r["sampled"]], [d for r in sel for d in r["idle"]]
            launches = sel[0]["launches"] if name == "pool" else 2 * SESSIONS * (len(sampled) + len(idle)) // len(sel)
            lines.append(f"| {Tc} / {To} | {name} | {audio / statistics.median(walls[name]):.1f} | {audio / max(walls[name]):.1f} | "
                         f"{audio / min(walls[name]):.1f} | {ms(sampled + idle)} | {ms(sampled)} | {ms(idle)} | "
                         f"{launches}{' (at most)' if name == 'parent' else ''} |")
        ratio = statistics.median(walls["parent"]) / statistics.median(walls["pool"])
        if max(walls["pool"]) < min(walls["parent"]):
            verdict = "every pool run beat every parent run"
        elif min(walls["pool"]) > max(walls["parent"]):
            verdict = "every pool run was SLOWER than every parent run"
        else:
            verdict = "the arms overlap: within spread"
        notes.append(f"{Tc} / {To}: pool against parent {ratio:.3f}x in aggregate rate; walls parent "
                     f"{min(walls['parent']):.3f} .. {max(walls['parent']):.3f} s, pool {min(walls['pool']):.3f} .. "
                     f"{max(walls['pool']):.3f} s; {verdict}")
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + \
        f"\n\n{SESSIONS} mono sessions of {SECONDS} s at {RATE} Hz in and out, blocks of {BLOCK}, {a.runs} alternating runs x {a.reps} " \
        f"repetitions per arm, N = {a.N}; the same bytes in every run of both arms" + \
        (f"; arm parent in {a.parent}\n" if a.parent else "; both arms in this tree\n")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
