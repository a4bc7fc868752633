"""GPU: the output stage of conv3x3_w2d_kernel (transposed products, conv_w2d.hip w2d_out) -- store map and statistics.

A. Per element.  rel-L2 over a whole tensor does not say WHERE a store map is wrong; here every output element is held
   against the fp64 direct convolution, relative to its own scale S = (conv(|act|, |w|) + |bias| + |bias2| + |res|) *
   scale, and the worst element is named as (b, y mod 16, x mod 16, channel) = (sample, place in the tile, channel).  A
   swapped pixel pair or channel quad is O(1) in that quotient.
B. Statistics.  The (mean, M2) partials of the stage have no entry point of their own: a ResnetBlock whose two convs run
   on this kernel feeds Conv_0's partials to GroupNorm_1, against the oracle's module; with Conv_0.bias + 20 the mean of
   Conv_0's output is far above its spread and a wrong pivot, count or merge shows as an error far above the bound."""
import ctypes as Ct
import json

import pytest
import torch
import torch.nn.functional as F

import _cases as C
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
TOL = 2e-5                  # rel-L2: the bound of test_gpu_ops / test_gpu_blocks

# B, H, W, C1, C2, Cout, with GroupNorm + SiLU
CASES = [
    (1, 16, 16, 32, 0, 64, True),       # one tile touching all four borders, one chunk, 32-channel blocks
    (2, 32, 48, 32, 32, 64, True),      # concat, two chunks, W = 3 tiles (row-major walk), 32-channel blocks, two samples
    (2, 32, 48, 32, 32, 64, False),     # the same without normalisation (gamma = None)
    (4, 64, 64, 32, 0, 256, True),      # 256 blocks of 64 channels (NJ = 2), channel offsets up to 192, one tile per block
    (4, 128, 128, 64, 0, 128, True),    # NJ = 2, two tiles per block (stage between tiles, buffer-1 reuse), even chunk count
]
# max |got - ref| / S of the commit BEFORE the output stage was rewritten, whose conv tensor this one's equals bit for
# bit, in the order of CASES (figures: test_w2d_per_element); the bound is twice the largest.
Q_PARENT = [4.789e-07, 9.414e-07, 6.486e-07, 1.026e-06, 7.005e-07]
Q_BOUND = 2.0 * max(Q_PARENT)


def rnd(seed, shape, std=1.0):
    return torch.from_numpy(synth.normal(91, seed, shape, std))


def run_case(case):
    """-> dict(q = max |got - ref| / S, at = its place, rel = rel-L2, route, repeat = second call bit-identical)"""
    import _gpu as G
    B, H, W, C1, C2, Cout, gn = case
    Cc = C1 + C2
    scale = 0.70710678
    x1 = rnd(1, (B, C1, H, W)) * 1.5 + 0.3
    x2 = rnd(2, (B, C2, H, W)) * 0.7 - 0.2 if C2 else None
    g = 1.0 + rnd(3, (Cc,), 0.2) if gn else None
    be = rnd(4, (Cc,), 0.2) if gn else None
    w = rnd(5, (Cout, Cc, 3, 3), (1.0 / (Cc * 9)) ** 0.5)
    bias = rnd(6, (Cout,), 0.1)
    bias2 = rnd(7, (B, Cout + 4), 0.1)                   # per sample: the rows differ
    res = rnd(8, (B, Cout, H, W))
    act = (torch.cat([x1, x2], 1) if C2 else x1).double()
    if gn:
        act = F.silu(F.group_norm(act, min(Cc // 4, 32), g.double(), be.double(), eps=1e-6))
    b2 = bias2[:, :Cout, None, None].double()
    ref = (F.conv2d(act, w.double(), bias.double(), padding=1) + b2 + res.double()) * scale
    S = (F.conv2d(act.abs(), w.double().abs(), bias.double().abs(), padding=1) + b2.abs() + res.double().abs()) * scale
    got = G.conv3x3_f43(x1, w, g, be, bias, x2, bias2, res, scale, True, form="w2d")
    route = G.last_route()
    again = G.conv3x3_f43(x1, w, g, be, bias, x2, bias2, res, scale, True, form="w2d")
    quo = (got.double() - ref).abs() / S
    k = int(quo.argmax())
    b, c, y, x = (int(v) for v in torch.unravel_index(torch.tensor(k), quo.shape))
    return dict(q=float(quo.max()), at=(b, y % 16, x % 16, c), rel=C.rel_l2(got, ref.float()), route=route,
                repeat=torch.equal(got, again))


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_w2d_per_element(idx):
    """Every output element against the fp64 direct convolution, relative to its own scale S.

    max |got - ref| / S measured with the parent commit's kernel (the wave-private transposition), MI355X, worst element as
    (b, y % 16, x % 16, channel), in the order of CASES:
        (1,16,16,32,0,64)      4.789e-07 at (0, 15, 4, 19)        (2,32,48,32,32,64)     9.414e-07 at (1, 15, 0, 3)
        the same, gamma None   6.486e-07 at (1, 15, 5, 63)        (4,64,64,32,0,256)     1.026e-06 at (2, 15, 0, 9)
        (4,128,128,64,0,128)   7.005e-07 at (1, 15, 11, 94)
    This kernel's output is bit-identical to that one's and gave the same five figures; the bound is twice the largest,
    2.05e-6.  A mapping error is O(1)."""
    r = run_case(CASES[idx])
    print(f"w2d per-element {CASES[idx]}: max |got - ref| / S = {r['q']:.3e} at (b, y % 16, x % 16, channel) = {r['at']}; "
          f"rel-L2 {r['rel']:.3e}; route {r['route']}")
    assert r["route"] == "w2d"
    assert r["repeat"], "two runs differ"
    assert r["rel"] < TOL
    assert r["q"] < Q_BOUND, f"worst element at (b, y % 16, x % 16, channel) = {r['at']}"


# ---- B: the statistics through GroupNorm_1 of a ResnetBlock
BLOCKS = [("b8", (8, 128, 64, 64)),        # both convs as 64-channel-block launches
          ("b4", (4, 128, 64, 64))]        # ... as 32-channel-block launches


def run_block(tag, shp, bias_shift=0.0):
    """-> (block output, oracle output, labels of the launches, route of the last conv launch)"""
    import _gpu as G
    from flowmse_amd import _lib
    from oracle import ncsnpp_oracle as O
    wl = {k: torch.from_numpy(synth.synth_param(f"w2dep.{tag}." + k, s)) for k, s in C.resblock_keys(128, 128, 512)}
    if bias_shift:
        wl["Conv_0.bias"] = wl["Conv_0.bias"] + bias_shift
    blk = G.Block("resnet", 128, 128, temb_dim=512).load(wl)
    x = torch.from_numpy(synth.normal(19, 31, shp))
    temb = torch.from_numpy(synth.normal(19, 32, (shp[0], 512)))
    ref = O.resblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x, temb)
    _lib.check(_lib.lib.flowse_profile_begin(blk.h, 1))
    got = blk(x, temb=temb)
    buf = Ct.create_string_buffer(1 << 16)
    _lib.check(_lib.lib.flowse_profile_end(blk.h, buf, len(buf)))
    labels = [k for k in json.loads(buf.value.decode()) if not k.startswith("_")]
    route = G.last_route()
    again = blk(x, temb=temb)
    assert torch.equal(got, again), "two runs differ"
    return got, ref, labels, route


@pytest.mark.parametrize("shift", [0.0, 20.0])
@pytest.mark.parametrize("tag,shp", BLOCKS)
def test_w2d_statistics_through_resblock(tag, shp, shift):
    """Conv_0's epilogue statistics are GroupNorm_1's only source.  shift = 20: Conv_0.bias + 20, mean >> spread (the oracle's
    own fp32 evaluation stays within 1.5e-6 of an fp64 one for that shift: checked on the CPU)."""
    got, ref, labels, route = run_block(tag, shp, shift)
    err = C.rel_l2(got, ref)
    print(f"w2d resblock {tag} Conv_0.bias + {shift}: rel-L2 vs oracle {err:.3e}; route {route}; launches: {labels}")
    assert "conv0_3x3_gn@64x64:128>128" in labels and "conv1_3x3_gn@64x64:128>128" in labels, labels
    assert route == "w2d"
    assert got.shape == ref.shape and err < TOL
