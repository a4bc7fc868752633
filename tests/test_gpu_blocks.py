"""GPU: the network's composite modules, one at a time, against the REFERENCE's own module outputs
(tests/golden/op_rb_*, op_attn_*, op_combine, written by oracle/gen_golden.py from the unmodified
ResnetBlockBigGANpp / AttnBlockpp / Combine, layerspp.py:44-91,212-274).  The single-module C-ABI handles
(flowse_block_create / flowse_block_forward) run the same weight packer, launch planner and kernels as the full
model, so this pins GroupNorm -> conv -> temb bias -> GroupNorm -> conv -> shortcut -> skip per block rather than only
through whole-network forwards."""
import pytest
import torch

import _cases as C
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
TOL = 2e-5

RB = [("rb_plain", 32, 32, (2, 32, 16, 8), {}, None),
      ("rb_widen", 48, 32, (2, 48, 16, 8), {}, None),
      ("rb_down", 32, 32, (2, 32, 16, 8), dict(down=True), True),
      ("rb_up", 32, 32, (2, 32, 8, 8), dict(up=True), True),
      ("rb_gn12", 384, 128, (1, 384, 8, 8), {}, None)]


def _weights(keys, prefix):
    return {k: torch.from_numpy(synth.synth_param(prefix + k, s)) for k, s in keys}


@pytest.mark.parametrize("tag,cin,cout,shp,kw,sc", RB)
def test_resblock_vs_reference(tag, cin, cout, shp, kw, sc):
    import _gpu as G
    g = C.gold("op_" + tag)
    blk = G.Block("resnet", cin, cout, temb_dim=64, **kw).load(_weights(C.resblock_keys(cin, cout, 64, sc), tag + "."))
    x = torch.from_numpy(synth.normal(5, 5, shp))
    temb = torch.from_numpy(synth.normal(5, 4, (2, 64)))[:shp[0]]
    out = blk(x, temb=temb)
    err = C.rel_l2(out, g["out"])
    print(tag, "rel-L2 vs reference module", err)
    assert out.shape == g["out"].shape and err < TOL


def test_resblock_concat_input_straddling_group():
    """The up-path blocks read cat[h, skip] from two tensors (ncsnpp.py:337); 384 = 256 + 128 channels puts one
    GroupNorm group (12 channels) across the seam."""
    import _gpu as G
    g = C.gold("op_rb_gn12")
    blk = G.Block("resnet", 384, 128, temb_dim=64).load(_weights(C.resblock_keys(384, 128, 64, None), "rb_gn12."))
    x = torch.from_numpy(synth.normal(5, 5, (1, 384, 8, 8)))
    temb = torch.from_numpy(synth.normal(5, 4, (2, 64)))[:1]
    out = blk(x[:, :256].contiguous(), x[:, 256:].contiguous(), temb=temb)
    assert C.rel_l2(out, g["out"]) < TOL


@pytest.mark.parametrize("tag,shape", [("attn_L64", (32, 8, 8)), ("attn_L256", (64, 16, 16)), ("attn_L16", (256, 4, 4))])
def test_attnblock_vs_reference(tag, shape):
    import _gpu as G
    Cc, H, W = shape
    g = C.gold("op_" + tag)
    blk = G.Block("attn", Cc, Cc).load(_weights(C.attn_keys(Cc), tag + "."))
    x = torch.from_numpy(synth.normal(5, 3, (2, Cc, H, W)))
    out = blk(x)
    err = C.rel_l2(out, g["out"])
    print(tag, "rel-L2 vs reference module", err)
    assert err < TOL


def test_combine_vs_reference():
    import _gpu as G
    g = C.gold("op_combine")
    keys = [("Conv_0.weight", (32, 4, 1, 1)), ("Conv_0.bias", (32,))]
    blk = G.Block("combine", 4, 32).load(_weights(keys, "comb."))
    xp = torch.from_numpy(synth.normal(5, 6, (2, 4, 8, 8)))
    yh = torch.from_numpy(synth.normal(5, 7, (2, 32, 8, 8)))
    assert C.rel_l2(blk(xp, yh), g["out"]) < TOL
    # the launcher's record of the block's one conv is what the route names for it, statistics asked for: the kernel that
    # leaves the next GroupNorm's statistics
    import ctypes
    from flowmse_amd import _lib
    buf = ctypes.create_string_buffer(96)
    assert _lib.lib.flowse_op_conv_route(0, 0, 2, 8, 8, 4, 0, 32, 1, 1024, buf, 96) == 0        # 1024 = FLOWSE_OFFER_STATS
    assert G.last_route() == "cin4_stats" == buf.value.decode().split()[0], (G.last_route(), buf.value)


def test_block_handle_rejects_misuse():
    import ctypes as Ct
    import _gpu as G
    from flowmse_amd import _lib
    h = Ct.c_void_p()
    assert _lib.lib.flowse_block_create(0, 32, 32, 1, 1, 64, Ct.byref(h)) != 0          # up and down
    assert _lib.lib.flowse_block_create(1, 32, 48, 0, 0, 0, Ct.byref(h)) != 0           # attention changes width
    blk = G.Block("resnet", 32, 32, temb_dim=64)
    x = torch.zeros(1, 8, 8, 32, device="cuda")
    with pytest.raises(_lib.FlowseError):                                                 # weights not loaded
        _lib.check(_lib.lib.flowse_block_forward(blk.h, _lib.ptr(x), 32, None, _lib.ptr(x), _lib.ptr(x), 1, 8, 8, None))


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit STORAGE modes (BASELINE configs 3 / 5): activations between kernels are bf16 / half, products on the 16-bit
# matrix cores, accumulation and GroupNorm statistics in fp32.  Every module variant, at shapes that take each kernel
# family (LDS-halo 3x3 with fused GroupNorm, flat 1x1 / 3x3, split-K, FIR, 4-channel heads), against the fp32 CPU oracle.
# The reference has no 16-bit path; the bounds are what 8 (bf16) / 11 (half) mantissa bits give for one module and are
# asserted as measured ceilings, not as parity with the reference: <= 2x what the MI355X runs measure (per ResnetBlock
# 3.0-3.8e-3 bf16 / 3.7-4.8e-4 half over the shapes below, attention block 2.3e-3 / 2.9e-4), so that an accuracy regression of the 16-bit kernels fails.
MODES16 = [("bf16", 6e-3), ("fp16", 8e-4)]
CASES16 = [  # tag, cin, cout, (B, C, H, W), kwargs, two-source split
    ("plain_halo", 128, 128, (2, 128, 64, 128), {}, None),
    ("plain_halo_16x16_tile", 128, 128, (8, 128, 128, 128), {}, None),      # >= 512 blocks of 256 pixels: two sub-tiles per block
    ("concat_halo_16x16_tile", 256, 128, (8, 256, 128, 128), {}, 128),
    ("concat_halo_shortcut", 256, 128, (2, 256, 64, 128), {}, 128),
    ("concat384_straddle", 384, 128, (2, 384, 64, 128), {}, 256),
    ("small_flat_splitk", 256, 256, (2, 256, 8, 8), {}, None),
    ("tiny_4x4_concat", 512, 256, (2, 512, 4, 4), {}, 256),
    ("down", 128, 128, (2, 128, 64, 64), dict(down=True), None),
    ("up", 256, 256, (2, 256, 16, 16), dict(up=True), None),
]


@pytest.mark.parametrize("mode,bound", MODES16)
@pytest.mark.parametrize("tag,cin,cout,shp,kw,split", CASES16)
def test_resblock_16bit_storage_vs_oracle(tag, cin, cout, shp, kw, split, mode, bound):
    import _gpu as G
    from oracle import ncsnpp_oracle as O
    sc = True if kw else None
    keys = C.resblock_keys(cin, cout, 512, sc)
    wl = _weights(keys, f"b16.{tag}.")
    blk = G.Block("resnet", cin, cout, temb_dim=512, **kw).load(wl, precision=mode)
    x = torch.from_numpy(synth.normal(7, 11, shp))
    temb = torch.from_numpy(synth.normal(7, 12, (shp[0], 512)))
    ref = O.resblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x, temb, **kw)
    got = blk(x, temb=temb) if split is None else blk(x[:, :split].contiguous(), x[:, split:].contiguous(), temb=temb)
    err = C.rel_l2(got, ref)
    print(f"resblock {tag} {mode}: rel-L2 vs fp32 oracle {err:.3e}")
    assert got.shape == ref.shape and err < bound


def test_resblock_16bit_shortcut_folded_vs_own_launch():
    """The 1x1 shortcut of a large 16-bit block runs as extra K steps of Conv_1's launch; under FLOWSE_NO_SCFOLD=1 (read when
    the plan is built) it is a launch of its own whose output rides as Conv_1's residual: same result as the folded plan,
    within the mode's ceiling."""
    import os
    import _gpu as G
    from oracle import ncsnpp_oracle as O
    tag, cin, cout, shp, kw, split = [c for c in CASES16 if c[0] == "concat_halo_shortcut"][0]
    keys = C.resblock_keys(cin, cout, 512, None)
    wl = _weights(keys, f"b16.{tag}.")
    x = torch.from_numpy(synth.normal(7, 11, shp))
    temb = torch.from_numpy(synth.normal(7, 12, (shp[0], 512)))
    ref = O.resblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x, temb)
    outs = {}
    for own in (False, True):
        if own:
            os.environ["FLOWSE_NO_SCFOLD"] = "1"
        try:
            blk = G.Block("resnet", cin, cout, temb_dim=512).load(wl, precision="bf16")
            outs[own] = blk(x[:, :split].contiguous(), x[:, split:].contiguous(), temb=temb)
        finally:
            os.environ.pop("FLOWSE_NO_SCFOLD", None)
    e0, e1, d = C.rel_l2(outs[False], ref), C.rel_l2(outs[True], ref), C.rel_l2(outs[True], outs[False])
    print(f"folded {e0:.3e}  own launch {e1:.3e}  between them {d:.3e}")
    assert e0 < 6e-3 and e1 < 6e-3 and 0 < d < 6e-3               # (d > 0: the hook really gave another plan)


def _worst_sample(got, ref):
    return max(C.rel_l2(got[b], ref[b]) for b in range(ref.shape[0]))


# 256 -> 256 ResnetBlocks on 1 x 1 / 1 x 2 images (below the released network's smallest level, 2 x 2): the 16-bit in-block
# split-K kernel (conv_smallm16b_kernel) leaves GroupNorm_1's partial statistics for blocks of H W pixels, i.e. 32 (block,
# channel) pairs per pixel of its 32-pixel tile -- 1024 pairs for 512 threads at H W = 1.  Pixels 16..31 of a tile are
# samples 16..31 at B = 32 and samples 16..23 at B = 24 (a partial tile), so the worst SAMPLE is asserted, and every block
# runs twice on one handle with different inputs so that statistics left in the workspace by the first call cannot stand
# in for ones the second call failed to write.  MI355X: worst sample 2.8e-3 bf16 / 3.4e-4 half (with the statistics pass
# writing only the first 512 pairs: rel-L2 ~1e2 at B = 32 and B = 24).
TINY16 = [("b32_1x1", (32, 256, 1, 1)), ("b24_1x1", (24, 256, 1, 1)), ("b16_1x2", (16, 256, 1, 2))]


@pytest.mark.parametrize("mode,bound", MODES16)
@pytest.mark.parametrize("tag,shp", TINY16)
def test_resblock_16bit_tiny_images_vs_oracle(tag, shp, mode, bound):
    import _gpu as G
    from oracle import ncsnpp_oracle as O
    wl = _weights(C.resblock_keys(256, 256, 512, None), f"b16.{tag}.")
    W = O._W({f"all_modules.0.{k}": v for k, v in wl.items()})
    blk = G.Block("resnet", 256, 256, temb_dim=512).load(wl, precision=mode)
    for call, seed in enumerate((11, 14)):
        x = torch.from_numpy(synth.normal(7, seed, shp))
        temb = torch.from_numpy(synth.normal(7, seed + 1, (shp[0], 512)))
        ref = O.resblock(W, 0, x, temb)
        got = blk(x, temb=temb)
        err, worst = C.rel_l2(got, ref), _worst_sample(got, ref)
        print(f"resblock {tag} {mode} call {call}: rel-L2 vs fp32 oracle {err:.3e}, worst sample {worst:.3e}")
        assert got.shape == ref.shape and err < bound and worst < bound


# AttnBlocks at the network's attention level (H = 16) for T = 256 / 1024 / 640 frames: L = 256 / 1024 / 640 tokens (more
# than 256 keys: several key tiles per wave of the attention kernel); W = 40 is no multiple of 16 (the 16-bit 1x1 / GroupNorm
# kernels' narrow-image forms).
ATTN_LONG = [("L1024", (1, 256, 16, 64)), ("L640_w40", (2, 256, 16, 40))]


@pytest.mark.parametrize("mode,bound", MODES16)
@pytest.mark.parametrize("shp", [(2, 256, 16, 16)] + [s for _, s in ATTN_LONG], ids=["L256"] + [t for t, _ in ATTN_LONG])
def test_attnblock_16bit_storage_vs_oracle(shp, mode, bound):
    import _gpu as G
    from oracle import ncsnpp_oracle as O
    wl = _weights(C.attn_keys(256), "b16.attn.")
    blk = G.Block("attn", 256, 256).load(wl, precision=mode)
    x = torch.from_numpy(synth.normal(7, 13, shp))
    ref = O.attnblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x)
    err = C.rel_l2(blk(x), ref)
    print(f"attnblock {shp} {mode}: rel-L2 vs fp32 oracle {err:.3e}")
    assert err < bound


@pytest.mark.parametrize("tag,shp", ATTN_LONG)
def test_attnblock_long_vs_oracle(tag, shp):
    """fp32 AttnBlocks over 1024 / 640 tokens against the oracle module (no reference goldens exist at these lengths)."""
    import _gpu as G
    from oracle import ncsnpp_oracle as O
    wl = _weights(C.attn_keys(256), f"attn_{tag}.")
    blk = G.Block("attn", 256, 256).load(wl)
    x = torch.from_numpy(synth.normal(5, 3, shp))
    ref = O.attnblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x)
    err = C.rel_l2(blk(x), ref)
    print(f"attnblock {tag} fp32: rel-L2 vs oracle {err:.3e}")
    assert err < TOL


def test_16bit_storage_falls_back_when_channels_do_not_tile():
    """Channel counts that are not multiples of 32 keep fp32 storage (precision then only selects operand types where a
    16-bit kernel applies): results stay fp32-class."""
    import _gpu as G
    g = C.gold("op_rb_widen")
    blk = G.Block("resnet", 48, 32, temb_dim=64).load(_weights(C.resblock_keys(48, 32, 64, None), "rb_widen."),
                                                     precision="bf16")
    x = torch.from_numpy(synth.normal(5, 5, (2, 48, 16, 8)))
    temb = torch.from_numpy(synth.normal(5, 4, (2, 64)))
    assert C.rel_l2(blk(x, temb=temb), g["out"]) < TOL


@pytest.mark.parametrize("tag,shp", [("flat", (2, 256, 8, 8)), ("f43_slices", (2, 256, 16, 16)), ("b1", (1, 256, 4, 4)),
                                     ("b1_16", (1, 256, 16, 16)), ("b8_16", (8, 256, 16, 16)), ("b32_4", (32, 256, 4, 4)),
                                     ("b1_32", (1, 256, 32, 32)), ("b32_1x1", (32, 256, 1, 1)),
                                     ("b24_1x1", (24, 256, 1, 1)), ("b16_1x2", (16, 256, 1, 2))])
def test_resblock_split_k_shapes_vs_oracle(tag, shp):
    """ResnetBlocks on images so small that every conv runs split over K (flat slices at 8x8 / 4x4, F(4,3) slices at
    16x16; 32-row tiles for a single utterance) with the two-pass reduction -- incl. the shortcut-free merged forms and
    the reduction fused with GroupNorm_1 -- against the oracle.  Since round 5 these shapes run the in-block split-K kernels
    (conv_smallm.hip): b8_16 = 2048 pixels on 64-channel tiles, b32_4 = two samples per 32-pixel tile (512 pixels of 4 x 4
    images), b1_32 = one utterance at 32 x 32 (32 statistics blocks per sample); *_1x1 / b16_1x2: more (statistics block,
    channel) pairs per tile than threads (the statistics pass loops), b24_1x1 on a partial tile -- asserted per sample."""
    import _gpu as G
    from oracle import ncsnpp_oracle as O
    keys = C.resblock_keys(256, 256, 512, None)
    wl = _weights(keys, "sk.")
    blk = G.Block("resnet", 256, 256, temb_dim=512).load(wl)
    x = torch.from_numpy(synth.normal(9, 21, shp))
    temb = torch.from_numpy(synth.normal(9, 22, (shp[0], 512)))
    ref = O.resblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x, temb)
    got = blk(x, temb=temb)
    err, worst = C.rel_l2(got, ref), _worst_sample(got, ref)
    print(tag, "split-K resblock vs oracle", err, "worst sample", worst)
    assert err < TOL and worst < TOL


def forward_with_labels(blk, x, split, temb):
    """-> (block output, {launch label: launches} of that forward, in launch order)"""
    import ctypes as Ct
    import json
    from flowmse_amd import _lib
    _lib.check(_lib.lib.flowse_profile_begin(blk.h, 1))
    got = blk(x, temb=temb) if split is None else blk(x[:, :split].contiguous(), x[:, split:].contiguous(), temb=temb)
    buf = Ct.create_string_buffer(1 << 16)
    _lib.check(_lib.lib.flowse_profile_end(blk.h, buf, len(buf)))
    return got, {k: v["launches"] for k, v in json.loads(buf.value.decode()).items() if not k.startswith("_")}


# ResnetBlocks with 2049..8191 pixels over the batch: past the small-image kernels (<= 2048 pixels), short of one block per
# CU -- every 3x3 conv runs as K slices with a reduction launch, and the plan folds work into those reductions.  The last
# column: launches per label family (the label up to its "@") that show the case reached its plan; 0 = must not appear.
#   F(4,3) slices need H % 8 == 0 and W % 16 == 0 and normalise on load; other widths run flat slices on a materialised input
#   Conv_0's reduction takes GroupNorm_1 from 128 (group, sample) blocks on: B >= 4 at 32 groups
#   a concat input (256 + 256 -> 256) has the 1x1 shortcut Conv_2; its slices ride on Conv_1's reduction: ONE splitk_reduce
# Which block-level case covers which form of the plan (Builder::resblock's record):
#   shortcut     none: every 256 -> 256 row here | own launch: rb_widen, rb_gn12, CASES16 tiny_4x4_concat / up / down, the
#                small up block of test_gpu_upblock_shortcut.py | low resolution: UP of test_gpu_upblock_shortcut.py |
#                merged: the *_merged rows | folded: CASES16 concat_halo_shortcut, concat384_straddle, concat_halo_16x16_tile
#   GroupNorm_0  on load: the f43_* rows, CASES16 *_halo* | materialised: the flat_* rows, RB
#   GroupNorm_1  applied by Conv_0's reduction: flat_apply* | mean / scale from Conv_0's reduction: f43_stats* | gn() + on
#                load: f43_b1*, CASES16 *_halo* | materialised: flat_b3, RB, the small-image rows of the test above
SLICED = [  # tag, mode, cin, cout, (B, C, H, W), two-source split, label family -> launches
    ("f43_stats", "fp32", 256, 256, (4, 256, 16, 48), None,
     {"conv0_3x3_gn": 1, "splitk_reduce_gn": 1, "conv1_3x3_gn": 1, "splitk_reduce": 1, "gn_finalize": 1, "gn_norm": 0}),
    ("flat_apply", "fp32", 256, 256, (4, 256, 24, 24), None,
     {"conv0_3x3": 1, "splitk_reduce_gn": 1, "conv1_3x3": 1, "splitk_reduce": 1, "gn_norm": 1, "gn_finalize": 0}),
    ("f43_stats_merged", "fp32", 512, 256, (4, 512, 16, 48), 256,
     {"conv2_1x1": 1, "conv0_3x3_gn": 1, "splitk_reduce_gn": 1, "conv1_3x3_gn": 1, "splitk_reduce": 1}),
    ("flat_apply_merged", "fp32", 512, 256, (4, 512, 24, 24), 256,
     {"conv2_1x1": 1, "conv0_3x3": 1, "splitk_reduce_gn": 1, "conv1_3x3": 1, "splitk_reduce": 1}),
    ("f43_b1", "fp32", 256, 256, (1, 256, 48, 48), None,
     {"conv0_3x3_gn": 1, "splitk_reduce_gn": 0, "gn_finalize": 2, "conv1_3x3_gn": 1, "splitk_reduce": 2}),
    ("f43_b1_merged", "fp32", 512, 256, (1, 512, 48, 48), 256,
     {"conv2_1x1": 1, "conv0_3x3_gn": 1, "splitk_reduce_gn": 0, "gn_finalize": 2, "conv1_3x3_gn": 1, "splitk_reduce": 2}),
    ("flat_b3", "fp32", 256, 256, (3, 256, 32, 24), None,
     {"conv0_3x3": 1, "splitk_reduce_gn": 0, "gn_norm": 2, "conv1_3x3": 1, "splitk_reduce": 2}),
    ("flat16_merged", "bf16", 512, 256, (4, 512, 32, 32), 256,
     {"conv2_1x1": 1, "conv0_3x3": 1, "splitk_reduce_gn": 1, "conv1_3x3": 1, "splitk_reduce": 1}),
    ("flat16_merged", "fp16", 512, 256, (4, 512, 32, 32), 256,
     {"conv2_1x1": 1, "conv0_3x3": 1, "splitk_reduce_gn": 1, "conv1_3x3": 1, "splitk_reduce": 1}),
]


def sliced_inputs(tag, cin, cout, shp):
    """weights, input and raw time embedding of a SLICED row (tools/block_plans.py runs the same)"""
    wl = _weights(C.resblock_keys(cin, cout, 512, None), f"sl.{tag}.")
    return wl, torch.from_numpy(synth.normal(9, 23, shp)), torch.from_numpy(synth.normal(9, 24, (shp[0], 512)))


@pytest.mark.parametrize("tag,mode,cin,cout,shp,split,want", SLICED, ids=[f"{c[0]}-{c[1]}" for c in SLICED])
def test_resblock_sliced_range_vs_oracle(tag, mode, cin, cout, shp, split, want):
    import _gpu as G
    from oracle import ncsnpp_oracle as O
    assert 2048 < shp[0] * shp[2] * shp[3] < 8192
    bound = dict(MODES16).get(mode, TOL)
    wl, x, temb = sliced_inputs(tag, cin, cout, shp)
    blk = G.Block("resnet", cin, cout, temb_dim=512).load(wl, precision=mode)
    ref = O.resblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x, temb)
    got, labels = forward_with_labels(blk, x, split, temb)
    err, worst = C.rel_l2(got, ref), _worst_sample(got, ref)
    print(f"resblock {tag} {mode}: rel-L2 vs oracle {err:.3e}, worst sample {worst:.3e}; launches: {labels}")
    assert got.shape == ref.shape and err < bound and worst < bound
    families = {}
    for k, n in labels.items():
        families[k.split("@")[0]] = families.get(k.split("@")[0], 0) + n
    assert {f: families.get(f, 0) for f in want} == want, labels
