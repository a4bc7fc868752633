#!/usr/bin/env python3
"""A-B timing of ``enhance --pool`` against the PARENT commit's ``enhance`` on a folder of short recordings, on the GPU box.

    python tools/pooled_ab.py --parent DIR [--runs 3] [--files 48] [--N 5] [--batch 8] [--work out/pooled_ab]
                              [--out TABLE.md]

``--parent`` is a checkout of the parent commit with its library built (``git worktree add DIR HEAD~1`` and
``python -m flowmse_amd.build`` in it).  The folder: ``--files`` synthetic 16 kHz mono recordings (the noisy signals of
``evaluate._synthetic_pairs``, 16-bit wav) with durations cycled over 1, 2, 3, 4, 6 and 10 s, and a checkpoint of the full
network with the synthetic weights, both written under ``--work`` once.

    A   python -m flowmse_amd.enhance --input FOLDER --ckpt CKPT --output ...          in the parent checkout
    B   the same command with --pool                                                   in this checkout

fp32, Euler, keyed noise (seed 3), one child process per run, arms alternating A-B-A-B.  The time is the one the command
prints itself -- from the first file's load to the last file's write, model construction excluded -- and the rate is the
folder's REAL frames (sum of L // 128 + 1) over it.  Gate: B's median rate is not below A's median by more than A's own
run-to-run spread (max - min of A's runs); the tool exits with status 1 if it is.  ``--out`` writes the table.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SECONDS = (1, 2, 3, 4, 6, 10)


def prepare(work, files):
    """The folder and the checkpoint (written once); returns (folder, ckpt, real frames of the folder)."""
    import numpy as np
    import torch
    from scipy.io import wavfile
    from flowmse_amd.evaluate import _synthetic_pairs
    from flowmse_amd.model import VFModel
    from flowmse_amd.util import synth
    folder, ckpt = os.path.join(work, "in"), os.path.join(work, "synthetic_full.ckpt")
    os.makedirs(folder, exist_ok=True)
    frames = 0
    for name, _, noisy in _synthetic_pairs(files, seconds=list(SECONDS), sr=16000):
        frames += noisy.shape[0] // 128 + 1
        path = os.path.join(folder, name)
        if not os.path.exists(path):
            wavfile.write(path, 16000, np.rint(noisy * 32767.0).astype(np.int16))
    if not os.path.exists(ckpt):
        model = VFModel(backbone="ncsnpp", ode="flowmatching")
        sd = {"dnn." + n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in model.dnn.named_parameters()}
        torch.save({"hyper_parameters": {"backbone": "ncsnpp", "ode": "flowmatching"}, "state_dict": sd}, ckpt)
    return folder, ckpt, frames


def run(cwd, folder, ckpt, out, a, extra):
    cmd = [sys.executable, "-W", "ignore", "-m", "flowmse_amd.enhance", "--input", folder, "--ckpt", ckpt, "--output", out,
           "--N", str(a.N), "--batch", str(a.batch), "--seed", "3"] + extra
    r = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} (in {cwd}) exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    m = re.search(r"enhanced (\d+) recordings \((\d+) frames\) in ([0-9.]+) s", r.stdout)
    if not m:
        raise SystemExit(f"no timing line in the output of {' '.join(cmd)}:\n{r.stdout[-2000:]}")
    return int(m.group(1)), int(m.group(2)), float(m.group(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checkout of the parent commit, library built")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", type=int, default=48)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--work", default=os.path.join(ROOT, "out", "pooled_ab"))
    ap.add_argument("--limit", type=int, default=400, help="time limit of one child process in seconds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    if not os.path.exists(os.path.join(parent, "flowmse_amd", "libflowse_hip.so")):
        raise SystemExit(f"--parent {parent}: no built library (python -m flowmse_amd.build in it first)")
    work = os.path.abspath(a.work)
    folder, ckpt, frames = prepare(work, a.files)
    arms = {"A": (parent, []), "B": (ROOT, ["--pool"])}
    rates = {k: [] for k in arms}
    for r in range(a.runs):
        for k, (cwd, extra) in arms.items():                        # A-B-A-B
            n, counted, secs = run(cwd, folder, ckpt, os.path.join(work, f"out_{k}"), a, extra)
            assert n == a.files and counted == frames, (k, n, counted, frames)
            rates[k].append(frames / secs)
            print(f"run {r + 1} {k}: {secs:7.2f} s  {rates[k][-1]:9.1f} real frames/s", flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = max(rates["A"]) - min(rates["A"])
    ratio = med["B"] / med["A"]
    ok = med["B"] >= med["A"] - spread
    lines = [f"| arm | command | runs (real frames/s) | median | min | max |", "|---|---|---|---|---|---|"]
    for k, what in (("A", "parent commit, `enhance`"), ("B", "this commit, `enhance --pool`")):
        v = rates[k]
        lines.append(f"| {k} | {what} | {', '.join(f'{x:.0f}' for x in v)} | {med[k]:.0f} | {min(v):.0f} | {max(v):.0f} |")
    lines.append("")
    lines.append(f"{a.files} files, {frames} real frames, N = {a.N}, batch {a.batch}, fp32. B / A = {ratio:.3f}; A's run-to-run "
                 f"spread (max - min) = {spread:.0f} frames/s; gate (B median >= A median - spread): "
                 f"{'met' if ok else 'MISSED'}.")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
