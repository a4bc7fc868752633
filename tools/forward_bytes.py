#!/usr/bin/env python3
"""Output bytes of one network forward per pinned plan, for comparing two builds of the library bit for bit.

    FLOWSE_LIB_PATH=<build A>/libflowse_hip.so python tools/forward_bytes.py a.json
    FLOWSE_LIB_PATH=<build B>/libflowse_hip.so python tools/forward_bytes.py b.json      # fresh process each
    cmp a.json b.json

The cases, the model (released architecture, synthetic weights) and the inputs are those of tests/test_gpu_plan_pins.py:
per (precision mode, B, T) one forward at F = 256, recorded as the SHA-256 of the complex64 output.  Where the plan pins
say that two builds launch the same kernels, this says that they also compute the same bits.

A tool, not a test: it pins nothing.  About half a minute on one GPU.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch

import _cases as C
import test_gpu_plan_pins as P
from flowmse_amd.util import synth


def main(path):
    assert torch.cuda.is_available(), "needs a GPU"
    dnn = P._model().dnn
    out = {}
    for mode, cases in P.CASES.items():
        dnn.set_precision(mode)
        for B, T in cases:
            x = C.c64(synth.complex_normal(41, 1, (B, 1, P.F, T), 0.5))
            y = C.c64(synth.synth_spectrogram(41, B, P.F, T))
            t = torch.full((B,), 0.515, device="cuda")
            with torch.no_grad():
                v = dnn(torch.cat([x, y], 1).cuda(), t)
            torch.cuda.synchronize()
            v = v.cpu().contiguous()
            raw = (torch.view_as_real(v) if v.is_complex() else v).numpy().tobytes()
            out[P._key(mode, B, T)] = hashlib.sha256(raw).hexdigest()
    dnn.set_precision("fp32")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
