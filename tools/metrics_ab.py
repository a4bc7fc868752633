#!/usr/bin/env python3
"""Timing of the device metrics (flowmse_amd.metrics) on the GPU box, for signals of 1 s, 4 s and 10 s: per file,

    host      the float64 numpy / scipy restatement ``estoi_reference`` plus the host ``energy_ratios`` (fp32 ``np.dot``, as
              ``evaluate --metrics host`` computes them), after the device-to-host copy of the enhanced waveform.  This is the
              RESTATEMENT, not pystoi: the package is not available here, and what it costs has not been measured
    device    ``metrics_device`` as queued work: 32 files queued one after the other, ONE read-back of the [32, 4] table
              (as ``evaluate --metrics device`` does per sampler call), divided by 32
    sampler   ``evaluate.enhance_waveform`` (Euler N = 5, fp32, full network, synthetic weights) for the same file

    python tools/metrics_ab.py [--reps 7] [--warmup 2] [--files 32] [--out profiles/metrics_ab.md]

The arms alternate inside every repetition; the table gives the median, timed with the host clock between device
synchronisations (every arm ends with its result on the host).  ``--out`` writes the table only; the text around it is
written by hand.
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
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from flowmse_amd import metrics as M
    from flowmse_amd.evaluate import _synthetic_pairs, energy_ratios, enhance_waveform
    from flowmse_amd.model import VFModel
    from flowmse_amd.util import synth
    assert torch.cuda.is_available(), "metrics_ab.py measures on the GPU; there is no CPU timing"
    model = VFModel(backbone="ncsnpp", ode="flowmatching")
    model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape)))
                               for n, p in model.dnn.named_parameters()})
    model = model.cuda().eval()

    rows = []
    for seconds in (1, 4, 10):
        _, clean, noisy = _synthetic_pairs(1, seconds=float(seconds))[0]
        yd = torch.from_numpy(noisy)[None].cuda()
        xd = torch.from_numpy(clean).cuda()
        torch.manual_seed(0)
        x_hat = enhance_waveform(model, yd, N=a.N, as_tensor=True)
        table = torch.empty(a.files, 4, dtype=torch.float64, device="cuda")

        def host():
            w = x_hat.cpu().numpy()
            return (M.estoi_reference(clean, w),) + tuple(energy_ratios(w, clean, noisy - clean))

        def device():
            for row in table:
                M.metrics_device(xd, yd[0], x_hat, out=row)
            return table.cpu().numpy()

        def sampler():
            return enhance_waveform(model, yd, N=a.N)

        arms = [("host", host, 1), ("device", device, a.files), ("sampler", sampler, 1)]
        times = {name: [] for name, _, _ in arms}
        last = {}
        for r in range(a.warmup + a.reps):
            for name, fn, per in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = fn()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[name].append((time.perf_counter() - t0) / per)
        diff = abs(float(last["device"][0][0]) - last["host"][0])
        assert diff <= 1e-7 and np.array_equal(last["device"][0], last["device"][-1]), (diff, last["device"][0], last["host"])
        for name, _, _ in arms:
            t = times[name]
            rows.append((f"{seconds} s", noisy.shape[0], name, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)))
            print(f"{seconds:3d} s  {name:8s} median {rows[-1][3]:9.3f} ms per file  (min {rows[-1][4]:.3f} max {rows[-1][5]:.3f} over "
                  f"{a.reps})", flush=True)
        print(f"{seconds:3d} s  estoi host {last['host'][0]:.12f} device {float(last['device'][0][0]):.12f}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("| signal | samples | arm | median ms per file | min ms | max ms |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.3f} | {r[4]:.3f} | {r[5]:.3f} |\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
