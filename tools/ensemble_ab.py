#!/usr/bin/env python3
"""A-B timing of ``evaluate --samples 4`` against what a user does without it: four runs of the PARENT commit's
``evaluate`` with four seeds and a host average of the 16-bit wavs.  On the GPU box.

    python tools/ensemble_ab.py --parent DIR [--runs 3] [--samples 4] [--files 16] [--N 5] [--work out/ensemble_ab]
                                [--out TABLE.md]

``--parent`` is a checkout of the parent commit with its library built (``git worktree add DIR HEAD~1`` and
``python -m flowmse_amd.build`` in it).

    A   for s in 1..D:  python -m flowmse_amd.evaluate --synthetic 16 --synthetic_seconds 2,3,4 --noise keyed --N 5 --seed s
        in the parent checkout, one process after the other, then the mean of the D wavs of every file on the host
        (read as int16, averaged in float64, written as 16-bit wav)
    B   python -m flowmse_amd.evaluate --synthetic 16 --synthetic_seconds 2,3,4 --noise keyed --N 5 --seed 1 --samples D
        in this checkout

fp32, Euler, ``--batch 1``: A's sampler calls are one row wide, B's are D rows wide.  The time is the wall time of the WHOLE
arm -- process start, synthetic weights, model construction, every file, the metrics, the reports, and in A the averaging --
since that is what the user waits for; the time each command prints for its file loop alone is listed beside it.  Arms
alternate A-B-A-B.  Gate: B's median time is not above A's median by more than A's own run-to-run spread (max - min of A's
runs); the tool exits with status 1 if it is.  ``--out`` writes the table.
The two arms do not write the same samples (A averages quantised wavs of seeds 1..D, B the linear spectra of draws 0..D-1
of seed 1); the tool times them and checks only that both wrote every file.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDS = "2,3,4"


def evaluate(cwd, out, a, extra):
    cmd = [sys.executable, "-W", "ignore", "-m", "flowmse_amd.evaluate", "--folder_destination", out, "--synthetic",
           str(a.files), "--synthetic_seconds", SECONDS, "--noise", "keyed", "--N", str(a.N)] + extra
    r = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} (in {cwd}) exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    m = re.search(r"enhanced (\d+) utterances \((\d+) frames\) in ([0-9.]+) s", r.stdout)
    if not m or int(m.group(1)) != a.files:
        raise SystemExit(f"no timing line for {a.files} utterances in the output of {' '.join(cmd)}:\n{r.stdout[-2000:]}")
    return float(m.group(3))                                       # the command's own figure: its file loop, no start-up


def host_average(dirs, out):
    """The mean of the wavs of ``dirs`` per file name, as a user without --samples forms it."""
    import numpy as np
    from scipy.io import wavfile
    os.makedirs(out, exist_ok=True)
    names = sorted(os.listdir(os.path.join(dirs[0], "files")))
    for n in names:
        waves = [wavfile.read(os.path.join(d, "files", n))[1].astype(np.float64) for d in dirs]
        wavfile.write(os.path.join(out, n), 16000, np.rint(np.mean(waves, axis=0)).astype(np.int16))
    return len(names)


def arm_a(parent, work, a):
    t0 = time.perf_counter()
    dirs = [os.path.join(work, f"A_seed{s}") for s in range(1, a.samples + 1)]
    loops = sum(evaluate(parent, d, a, ["--seed", str(s)]) for s, d in enumerate(dirs, 1))
    n = host_average(dirs, os.path.join(work, "A_mean"))
    return time.perf_counter() - t0, loops, n


def arm_b(work, a):
    t0 = time.perf_counter()
    out = os.path.join(work, "B")
    loop = evaluate(ROOT, out, a, ["--seed", "1", "--samples", str(a.samples)])
    return time.perf_counter() - t0, loop, len(os.listdir(os.path.join(out, "files")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checkout of the parent commit, library built")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--work", default=os.path.join(ROOT, "out", "ensemble_ab"))
    ap.add_argument("--limit", type=int, default=300, help="time limit of one child process in seconds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    if not os.path.exists(os.path.join(parent, "flowmse_amd", "libflowse_hip.so")):
        raise SystemExit(f"--parent {parent}: no built library (python -m flowmse_amd.build in it first)")
    work = os.path.abspath(a.work)
    os.makedirs(work, exist_ok=True)
    secs, loops = {"A": [], "B": []}, {"A": [], "B": []}
    for r in range(a.runs):
        for k in ("A", "B"):                                        # A-B-A-B
            t, loop, n = arm_a(parent, work, a) if k == "A" else arm_b(work, a)
            assert n == a.files, (k, n)
            secs[k].append(t)
            loops[k].append(loop)
            print(f"run {r + 1} {k}: {t:7.2f} s, of which the file loops {loop:6.2f} s", flush=True)
    med = {k: statistics.median(v) for k, v in secs.items()}
    spread = max(secs["A"]) - min(secs["A"])
    ok = med["B"] <= med["A"] + spread
    lines = ["| arm | what | runs (s) | median | min | max | file loops alone (s) |", "|---|---|---|---|---|---|---|"]
    for k, what in (("A", f"parent commit, {a.samples} x `evaluate --seed s` + host mean of the wavs"),
                    ("B", f"this commit, `evaluate --samples {a.samples}`")):
        v = secs[k]
        lines.append(f"| {k} | {what} | {', '.join(f'{x:.2f}' for x in v)} | {med[k]:.2f} | {min(v):.2f} | {max(v):.2f} | "
                     f"{', '.join(f'{x:.2f}' for x in loops[k])} |")
    lines.append("")
    lines.append(f"{a.files} files of {SECONDS} s, N = {a.N}, batch 1, fp32, D = {a.samples}. A / B = {med['A'] / med['B']:.3f} "
                 f"(medians); A's run-to-run spread (max - min) = {spread:.2f} s, B's = {max(secs['B']) - min(secs['B']):.2f} s; "
                 f"gate (B median <= A median + A's spread): {'met' if ok else 'MISSED'}. File loops alone (the time each "
                 f"command prints, summed over A's {a.samples} processes): A / B = "
                 f"{statistics.median(loops['A']) / statistics.median(loops['B']):.3f}.")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
