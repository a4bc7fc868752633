#!/usr/bin/env python3
"""Black-box RK45 sampler: scipy on the host (the reference's path) against the fused device solve (flowse_rk45_sample).

    python tools/blackbox_ab.py [--shapes 1,256,256 8,256,256] [--runs 3] [--tol 1e-5] [--precision fp32]

Full-size network with synthetic weights, the sampler's defaults (T_rev 1, t_eps 0.03, rtol = atol = --tol).  For each
shape and path: nfev, accepted steps, wall time (median of --runs after one warm-up), frames/s (B * T frames per
solve), then the rel-L2 between the two end points.  The host path is the same HIP model behind a plain lambda, which
get_black_box_solver sends to scipy.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from flowmse_amd.model import VFModel  # noqa: E402
from flowmse_amd.sampling import get_black_box_solver  # noqa: E402
from flowmse_amd.util import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,256,256", "8,256,256"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--precision", default="fp32")
    a = ap.parse_args()
    m = VFModel(backbone="ncsnpp", ode="flowmatching")
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    m = m.cuda().eval()
    m.dnn.set_precision(a.precision)
    host_field = lambda x, t, y: m(x, t, y)   # noqa: E731  (no rk45_sample_: scipy path)
    print(f"black-box RK45, rtol = atol = {a.tol:g}, precision {a.precision}, {torch.cuda.get_device_name(0)}", flush=True)
    for spec in a.shapes:
        B, F, T = (int(v) for v in spec.split(","))
        y = torch.from_numpy(synth.synth_spectrogram(0, B, F, T)).cuda()
        z = torch.from_numpy(synth.synth_noise(0, B, F, T)).cuda()
        ends = {}
        for name, field in (("host", host_field), ("fused", m)):
            solver = get_black_box_solver(m.ode, field, y, rtol=a.tol, atol=a.tol, z=z)
            times = []
            for i in range(a.runs + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x, nfev = solver()
                torch.cuda.synchronize()
                if i:
                    times.append(time.perf_counter() - t0)
            with torch.no_grad():
                x0 = m.ode.prior_sampling(y.shape, y, z)[0].contiguous()
                _, _, _, acc = m.rk45_sample_(x0, y, 1.0, 0.03, a.tol, a.tol)
            wall = statistics.median(times)
            ends[name] = x.cpu()
            print(f"[{B},1,{F},{T}] {name:5s}: nfev {nfev}, accepted {len(acc)}, wall {wall * 1e3:.1f} ms "
                  f"(median of {a.runs}), {B * T / wall:.1f} frames/s, {wall / nfev * 1e3:.2f} ms/nfev", flush=True)
        d = (ends["fused"] - ends["host"]).abs().pow(2).sum().sqrt() / ends["host"].abs().pow(2).sum().sqrt()
        print(f"[{B},1,{F},{T}] endpoint rel-L2 fused vs host: {float(d):.3e}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
