#!/usr/bin/env python3
"""Output bytes of the kernels that split K inside the block, for comparing two builds of the library bit for bit.

    FLOWSE_LIB_PATH=<build A>/libflowse_hip.so python tools/smallm_bytes.py a.json
    FLOWSE_LIB_PATH=<build B>/libflowse_hip.so python tools/smallm_bytes.py b.json      # fresh process each
    cmp a.json b.json

Goes through tests/_gpu.py on the tests' own seeded inputs and records, per case, the SHA-256 of the fp32 NCHW output and the
route the library reports (flowse_op_last_conv_route; for a block: of its last convolution):

  op level     every case of tests/_smallm_ref.CASES (all eleven small-image instances, every ring edge, ragged tiles, 1x1 and
               1x2 images, fp32-out 16-bit instances) and STREAM_CASES of tests/test_gpu_ops.py (the streaming 1x1 kernel)
  block level  ResnetBlocks, whose bytes carry the fused GroupNorm statistics of the first conv (a wrong statistic changes
               the block's output): the shapes of test_resblock_split_k_shapes_vs_oracle in fp32, TINY16 (two calls on one
               handle) and the small_flat_splitk / tiny_4x4_concat / up rows of CASES16 in bf16 and fp16

A tool, not a test: it pins nothing, a numeric change to these kernels stays free to make.  Seconds on one GPU.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch

import _cases as C
import _gpu as G
import _smallm_ref as R
import test_gpu_blocks as TB
import test_gpu_ops as TO
from flowmse_amd.util import synth


def sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def op_cases(out):
    for c in R.CASES:
        x, w, bias, bias2, res = R.inputs(c)
        x1 = x[:, :c.C1].contiguous()
        x2 = x[:, c.C1:].contiguous() if c.C2 else None
        if c.dt is None:
            got = G.conv2d(x1, w, bias, x2, bias2, res, c.scale, splitk=True)
        else:
            got = G.conv2d_16(x1, w, R.DT_CODE[c.dt], bias, x2, bias2, res, c.scale, out_f32=c.out32)
        out[f"smallm/{c.name}"] = {"route": G.last_route(), "sha256": sha(got)}
    for case in TO.STREAM_CASES:
        B, H, W, C1, C2, Cout, has_b, has_b2, has_res, scale = case
        x1 = TO.rnd(1, (B, C1, H, W))
        x2 = TO.rnd(2, (B, C2, H, W)) if C2 else None
        w = TO.rnd(3, (Cout, C1 + C2, 1, 1), (1.0 / (C1 + C2)) ** 0.5)
        bias = TO.rnd(4, (Cout,), 0.1) if has_b else None
        bias2 = TO.rnd(5, (B, Cout + 8), 0.1) if has_b2 else None
        res = TO.rnd(6, (B, Cout, H, W)) if has_res else None
        got = G.conv2d(x1, w, bias, x2, bias2, res, scale, splitk=True)
        out["stream/" + "x".join(str(v) for v in case[:6])] = {"route": G.last_route(), "sha256": sha(got)}


def block_cases(out):
    shapes = TB.test_resblock_split_k_shapes_vs_oracle.pytestmark[0].args[1]
    wl = TB._weights(C.resblock_keys(256, 256, 512, None), "sk.")
    for tag, shp in shapes:
        blk = G.Block("resnet", 256, 256, temb_dim=512).load(wl)
        x = torch.from_numpy(synth.normal(9, 21, shp))
        temb = torch.from_numpy(synth.normal(9, 22, (shp[0], 512)))
        got = blk(x, temb=temb)
        out[f"resblock_fp32/{tag}"] = {"route": G.last_route(), "sha256": sha(got)}
    for mode, _ in TB.MODES16:
        for tag, shp in TB.TINY16:
            blk = G.Block("resnet", 256, 256, temb_dim=512).load(
                TB._weights(C.resblock_keys(256, 256, 512, None), f"b16.{tag}."), precision=mode)
            for call, seed in enumerate((11, 14)):
                x = torch.from_numpy(synth.normal(7, seed, shp))
                temb = torch.from_numpy(synth.normal(7, seed + 1, (shp[0], 512)))
                got = blk(x, temb=temb)
                out[f"tiny16_{mode}/{tag}/call{call}"] = {"route": G.last_route(), "sha256": sha(got)}
        for tag, cin, cout, shp, kw, split in TB.CASES16:
            if tag not in ("small_flat_splitk", "tiny_4x4_concat", "up"):
                continue
            wl16 = TB._weights(C.resblock_keys(cin, cout, 512, True if kw else None), f"b16.{tag}.")
            blk = G.Block("resnet", cin, cout, temb_dim=512, **kw).load(wl16, precision=mode)
            x = torch.from_numpy(synth.normal(7, 11, shp))
            temb = torch.from_numpy(synth.normal(7, 12, (shp[0], 512)))
            got = blk(x, temb=temb) if split is None else blk(x[:, :split].contiguous(), x[:, split:].contiguous(), temb=temb)
            out[f"resblock16_{mode}/{tag}"] = {"route": G.last_route(), "sha256": sha(got)}


def main(path):
    assert torch.cuda.is_available(), "needs a GPU"
    out = {}
    op_cases(out)
    block_cases(out)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
