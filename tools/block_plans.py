#!/usr/bin/env python3
"""Launch plan and output bytes of every ResnetBlock case of the block-level tests, for comparing two builds of the library.

    FLOWSE_LIB_PATH=<build A>/libflowse_hip.so python tools/block_plans.py a.json
    FLOWSE_LIB_PATH=<build B>/libflowse_hip.so python tools/block_plans.py b.json
    cmp a.json b.json

Goes through tests/_gpu.py on the tests' own seeded inputs and records, per case, the launch labels of the forward with
their launch counts (flowse_profile_begin / _end, in plan order) and the SHA-256 of the fp32 NCHW output:

  tests/test_gpu_blocks.py            RB (+ rb_gn12 from two tensors, rb_widen in bf16 mode), CASES16 and TINY16 in bf16 and fp16, the shapes of
                                      test_resblock_split_k_shapes_vs_oracle, SLICED
  tests/test_gpu_upblock_shortcut.py  UP, the shifted bias, the small up block

once as the library plans them and once each under FLOWSE_NO_SCFOLD=1 (no folded shortcut), FLOWSE_NO_SC_LOW=1 (no
low-resolution shortcut) and FLOWSE_NO_SMALLM=1 (no small-image kernels: the blocks of <= 2048 pixels go back to K slices,
so the merged reduction and the reduction that finishes GroupNorm_1 appear at the tiny shapes too).  Each of the four is a
child process under its own time limit; the first one that fails ends the run.

A tool, not a test: it pins nothing.  About a minute on one GPU.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ["", "FLOWSE_NO_SCFOLD", "FLOWSE_NO_SC_LOW", "FLOWSE_NO_SMALLM"]
CHILD_SECONDS = 300


def child(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch

    import _cases as C
    import _gpu as G
    import test_gpu_blocks as TB
    import test_gpu_upblock_shortcut as TU
    from flowmse_amd.util import synth

    assert torch.cuda.is_available(), "needs a GPU"
    out = {}

    def run(name, blk, x, split, temb):
        got, labels = TB.forward_with_labels(blk, x, split, temb)
        out[name] = {"launches": [[k, n] for k, n in labels.items()],
                     "sha256": hashlib.sha256(got.contiguous().numpy().tobytes()).hexdigest()}

    for tag, cin, cout, shp, kw, sc in TB.RB:
        for mode in ("fp32", "bf16") if tag == "rb_widen" else ("fp32",):     # (48 channels keep fp32 storage in bf16 mode)
            blk = G.Block("resnet", cin, cout, temb_dim=64, **kw).load(
                TB._weights(C.resblock_keys(cin, cout, 64, sc), tag + "."), precision=mode)
            x = torch.from_numpy(synth.normal(5, 5, shp))
            temb = torch.from_numpy(synth.normal(5, 4, (2, 64)))[:shp[0]]
            run(f"rb_{mode}/{tag}", blk, x, None, temb)
            if tag == "rb_gn12":
                run(f"rb_{mode}/{tag}_two_tensors", blk, x, 256, temb)
    for mode, _ in TB.MODES16:
        for tag, cin, cout, shp, kw, split in TB.CASES16:
            wl = TB._weights(C.resblock_keys(cin, cout, 512, True if kw else None), f"b16.{tag}.")
            blk = G.Block("resnet", cin, cout, temb_dim=512, **kw).load(wl, precision=mode)
            x = torch.from_numpy(synth.normal(7, 11, shp))
            temb = torch.from_numpy(synth.normal(7, 12, (shp[0], 512)))
            run(f"cases16_{mode}/{tag}", blk, x, split, temb)
        for tag, shp in TB.TINY16:
            blk = G.Block("resnet", 256, 256, temb_dim=512).load(
                TB._weights(C.resblock_keys(256, 256, 512, None), f"b16.{tag}."), precision=mode)
            for call, seed in enumerate((11, 14)):
                x = torch.from_numpy(synth.normal(7, seed, shp))
                temb = torch.from_numpy(synth.normal(7, seed + 1, (shp[0], 512)))
                run(f"tiny16_{mode}/{tag}/call{call}", blk, x, None, temb)
    wl = TB._weights(C.resblock_keys(256, 256, 512, None), "sk.")
    for tag, shp in TB.test_resblock_split_k_shapes_vs_oracle.pytestmark[0].args[1]:
        blk = G.Block("resnet", 256, 256, temb_dim=512).load(wl)
        x = torch.from_numpy(synth.normal(9, 21, shp))
        temb = torch.from_numpy(synth.normal(9, 22, (shp[0], 512)))
        run(f"split_k_fp32/{tag}", blk, x, None, temb)
    for tag, mode, cin, cout, shp, split, _ in TB.SLICED:
        wl, x, temb = TB.sliced_inputs(tag, cin, cout, shp)
        run(f"sliced_{mode}/{tag}", G.Block("resnet", cin, cout, temb_dim=512).load(wl, precision=mode), x, split, temb)
    ups = [(t, ci, co, shp, 0.0) for t, ci, co, shp in TU.UP]
    ups += [(TU.UP[1][0] + "_bias50",) + TU.UP[1][1:] + (50.0,), ("b2_256_16", 256, 256, (2, 256, 16, 16), 0.0)]
    for tag, cin, cout, shp, shift in ups:
        blk = G.Block("resnet", cin, cout, up=True, temb_dim=512).load(TU._weights(cin, cout, tag.replace("_bias50", ""), shift))
        x = torch.from_numpy(synth.normal(17, 31, shp))
        temb = torch.from_numpy(synth.normal(17, 32, (shp[0], 512)))
        run(f"up_fp32/{tag}", blk, x, None, temb)
    with open(path, "w") as f:
        json.dump(out, f)


def main(path):
    merged = {}
    for hook in HOOKS:
        env = dict(os.environ)
        for h in HOOKS[1:]:
            env.pop(h, None)
        if hook:
            env[hook] = "1"
        part = f"{path}.{hook or 'default'}.part"
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", part]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            sys.exit(f"{hook or 'no hook'}: exit status {rc}; stopping")
        with open(part) as f:
            merged[hook or "default"] = json.load(f)
        os.remove(part)
    with open(path, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in merged.values())} cases under {len(HOOKS)} settings -> {path}")


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main(sys.argv[1])
