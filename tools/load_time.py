#!/usr/bin/env python3
"""Wall time of flowse_model_load_weights, for comparing two builds of the library.

    FLOWSE_LIB_PATH=<build A>/libflowse_hip.so python tools/load_time.py      # fresh process each
    FLOWSE_LIB_PATH=<build B>/libflowse_hip.so python tools/load_time.py

The released architecture with synthetic weights (tests/test_gpu_plan_pins.py's model), in the fp32 and the bf16 mode: a
host clock around the call, ending in a device synchronise; the first upload of a mode (it allocates) and the median of
five more.  Prints one JSON line.  A tool, not a test: it pins nothing.
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch

import test_gpu_plan_pins as P
from flowmse_amd import _lib


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    dnn = P._model().dnn
    blob = dnn.canonical_blob().contiguous()
    out = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT)}
    for mode in ("fp32", "bf16"):
        dnn.set_precision(mode)
        ms = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(_lib.lib.flowse_model_load_weights(dnn._handle, ctypes.c_void_p(blob.data_ptr()), blob.numel()))
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        out[mode] = {"first_ms": round(ms[0], 2), "median_ms": round(statistics.median(ms[1:]), 2),
                     "min_ms": round(min(ms[1:]), 2), "max_ms": round(max(ms[1:]), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
