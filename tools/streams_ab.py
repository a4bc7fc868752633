#!/usr/bin/env python3
"""A-B of the multi-lane sampler against one sampler call at a time (and against another build of the project).

    python tools/streams_ab.py --parent-tree DIR [--out profiles/streams_ab.md] [--reps 20] [--warmup 5]

Arms, one process each, in the order P S1 S2 S3 S4 P S1 S2 S3 S4:
  P   the tree under --parent-tree (a built checkout of the parent commit, e.g. a ``git worktree``), items one after the
      other through ``NCSNpp.rk_sample``; the arm uses nothing newer, so this same file drives both trees
  S1  this tree, the same sequential loop
  S2..S4  this tree, one ``NCSNpp.rk_sample_multi`` call per repetition on 2..4 lanes
Workload A: four utterances [1,1,256,256]; workload B: T = 128, 192, 256, 320 (lengths that cannot share a batch).  Euler
N = 5, fp32, synthetic weights and inputs.  Each arm reports aggregate frames/s over the timed repetitions (one
synchronise before and after all of them) for both workloads.

Every arm runs under its own ``timeout -k 10``; after an arm that fails nothing else is started.  Without
--parent-tree the P arms are left out.  ``--arm NAME`` runs one arm in this process and prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
WORKLOADS = {"A": [256, 256, 256, 256], "B": [128, 192, 256, 320]}


def run_arm(arm, tree, reps, warmup):
    sys.path.insert(0, tree)
    import torch
    from flowmse_amd.model import VFModel
    from flowmse_amd.sampling import time_grid
    from flowmse_amd.util import synth
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape)))
                               for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()
    ts, dts = (v.tolist() for v in time_grid(1.0, 0.03, 5))
    lanes = 1 if arm in ("P", "S1") else int(arm[1:])
    res = {"arm": arm, "tree": tree, "lanes": lanes}
    for name, lens in WORKLOADS.items():
        ys = [torch.from_numpy(synth.synth_spectrogram(20 + i, 1, 256, T)).cuda() for i, T in enumerate(lens)]
        zs = [torch.from_numpy(synth.synth_noise(20 + i, 1, 256, T)).cuda() for i, T in enumerate(lens)]
        x0 = [model.ode.prior_sampling(y.shape, y, z)[0].contiguous() for y, z in zip(ys, zs)]
        xs = [x.clone() for x in x0]

        def once():
            for x, s in zip(xs, x0):
                x.copy_(s)
            if lanes == 1:
                for x, y in zip(xs, ys):
                    model.dnn.rk_sample(x, y, ts, dts, "euler")
            else:
                model.dnn.rk_sample_multi(xs, ys, ts, dts, "euler", lanes=lanes)

        for _ in range(warmup):
            once()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            once()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = {"frames_per_s": reps * sum(lens) / dt, "ms_per_rep": 1e3 * dt / reps,
                     "checksum": float(sum(x.abs().sum().item() for x in xs))}
    print("STREAMS_AB " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, help="run this single arm (P, S1..S4) in this process")
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="--arm: the project tree to import")
    ap.add_argument("--parent-tree", default=None, help="built checkout of the commit to compare against")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arm-timeout", type=int, default=240, help="seconds per arm")
    ap.add_argument("--out", default=None, help="write the table here (markdown)")
    args = ap.parse_args()
    if args.arm:
        return run_arm(args.arm, os.path.abspath(args.tree), args.reps, args.warmup)
    arms = (["P"] if args.parent_tree else []) + ["S1", "S2", "S3", "S4"]
    rows = []
    for arm in arms + arms:
        tree = os.path.abspath(args.parent_tree) if arm == "P" else os.path.dirname(HERE)
        cmd = ["timeout", "-k", "10", str(args.arm_timeout), sys.executable, os.path.abspath(__file__), "--arm", arm,
               "--tree", tree, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STREAMS_AB ")]
        if r.returncode != 0 or not line:
            print(f"arm {arm} failed with exit status {r.returncode}; stopping here\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}",
                  flush=True)
            return 1
        rows.append(json.loads(line[-1][len("STREAMS_AB "):]))
        print(line[-1], flush=True)
    text = ["| run | arm | lanes | A: frames/s | A: ms / 4 utterances | B: frames/s | B: ms / 4 utterances |",
            "|---|---|---|---|---|---|---|"]
    for i, r in enumerate(rows):
        text.append(f"| {i // len(arms) + 1} | {r['arm']} | {r['lanes']} | {r['A']['frames_per_s']:.0f} | "
                    f"{r['A']['ms_per_rep']:.2f} | {r['B']['frames_per_s']:.0f} | {r['B']['ms_per_rep']:.2f} |")
    same = all(len({r[w]["checksum"] for r in rows}) == 1 for w in WORKLOADS)      # one value per workload over all arms
    text.append("")
    text.append(f"Output checksums equal across all arms and both runs: {'yes' if same else 'NO'}")
    print("\n".join(text), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
