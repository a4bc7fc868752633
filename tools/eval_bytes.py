#!/usr/bin/env python3
"""Output bytes of the command-line front ends, for comparing two commits of the Python front end byte for byte.

    python tools/eval_bytes.py a.json            # in a checkout of commit A (library built)
    python tools/eval_bytes.py b.json            # in a checkout of commit B
    cmp a.json b.json

Runs a fixed list of ``flowmse_amd.evaluate`` and ``flowmse_amd.enhance`` commands on synthetic weights and signals, one after
another, each a fresh child process under its own ``timeout -k 10``, and stops at the first non-zero exit status.  Prints
(and, with a path, writes) one JSON object: run name -> {file path below the run's folder: SHA-256 of the file}.

  evaluate  --synthetic 5 --synthetic_seconds 1.0,2.0,3.0 --N 2 --seed 7 (padded lengths 128, 256, 384, 128, 256):
            --noise torch and keyed, each at (--batch, --streams) = (1,1) (2,1) (1,2) (2,2); keyed and torch (2,1) with
            --metrics device; keyed (2,1) with --valid_loss 2.  Every file: files/*.wav, _results.csv, _avg_results.txt,
            _settings.txt
  enhance   --synthetic 3 --synthetic_seconds 1.0,5.0 --N 2 --seed 7, plain and --pool --batch 2 (the chunked and the pooled
            callers of the fused spectrogram kernels)

``--gpus 2`` is not here: tests/test_gpu_keyed_noise.py covers it.  A tool, not a test: it pins nothing.  About a minute on
one GPU, most of it the thirteen model loads.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300                      # seconds per child process

EVALUATE = ["-m", "flowmse_amd.evaluate", "--synthetic", "5", "--synthetic_seconds", "1.0,2.0,3.0", "--N", "2", "--seed", "7"]
ENHANCE = ["-m", "flowmse_amd.enhance", "--synthetic", "3", "--synthetic_seconds", "1.0,5.0", "--N", "2", "--seed", "7"]


def runs():
    """[(name, argv without the output folder, the option that names the folder)]"""
    out = []
    for noise in ("torch", "keyed"):
        for b, s in ((1, 1), (2, 1), (1, 2), (2, 2)):
            out.append((f"evaluate/{noise}/batch{b}_streams{s}",
                        EVALUATE + ["--noise", noise, "--batch", str(b), "--streams", str(s)], "--folder_destination"))
    for noise in ("keyed", "torch"):
        out.append((f"evaluate/{noise}/batch2_streams1_metrics_device",
                    EVALUATE + ["--noise", noise, "--batch", "2", "--metrics", "device"], "--folder_destination"))
    out.append(("evaluate/keyed/batch2_streams1_valid_loss2",
                EVALUATE + ["--noise", "keyed", "--batch", "2", "--valid_loss", "2"], "--folder_destination"))
    out.append(("enhance/plain", ENHANCE, "--output"))
    out.append(("enhance/pool_batch2", ENHANCE + ["--pool", "--batch", "2"], "--output"))
    return out


def sha_tree(folder):
    out = {}
    for d, _, files in os.walk(folder):
        for n in files:
            p = os.path.join(d, n)
            with open(p, "rb") as f:
                out[os.path.relpath(p, folder)] = hashlib.sha256(f.read()).hexdigest()
    return dict(sorted(out.items()))


def main(path=None):
    result = {}
    with tempfile.TemporaryDirectory() as work:
        for name, argv, dest in runs():
            folder = os.path.join(work, name.replace("/", "_"))
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, "-W", "ignore"] + argv + [dest, folder]
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"{name}: {' '.join(cmd)} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
            print(f"{name}: {r.stdout.strip().splitlines()[-1]}", file=sys.stderr, flush=True)
            result[name] = sha_tree(folder)
    text = json.dumps(result, indent=1, sort_keys=True) + "\n"
    if path:
        with open(path, "w") as f:
            f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else None))
