"""GPU: fp32 up-sampling ResnetBlocks whose 1x1 shortcut runs BEFORE the upsampling.

ResnetBlockBigGANpp with up=True computes Conv_2(upsample_2d(x)) (layerspp.py:248, 268-269).  upsample_2d is the same FIR
on every channel and Conv_2 has no spatial extent, so W . up(x) = up(W . x): the plan runs the 1x1 at the low resolution
(a quarter of the pixels), upsamples its output, and adds Conv_2's bias in Conv_1's epilogue -- up(const) is not constant
at the image border (upsample_2d pads with zeros: a corner keeps 9/16 of a constant, an edge 3/4), so a bias upsampled with
the data would be wrong there.  Checked against the oracle's module, which keeps the reference's order, below the bound
test_gpu_blocks.py holds every fp32 ResnetBlock to."""
import ctypes as Ct
import json

import pytest
import torch

import _cases as C
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
TOL = 2e-5          # = test_gpu_blocks.TOL

# tag, cin, cout, (B, C, H, W) of the input: more than 2048 low-resolution pixels over the batch, where the plan reorders
UP = [("b8_256_32", 256, 256, (8, 256, 32, 32)),
      ("b2_128_64", 128, 128, (2, 128, 64, 64)),
      ("b4_256to128_32", 256, 128, (4, 256, 32, 32)),
      ("b1_128_64", 128, 128, (1, 128, 64, 64))]


def _weights(cin, cout, tag, bias_shift=0.0):
    wl = {k: torch.from_numpy(synth.synth_param(f"upsc.{tag}." + k, s)) for k, s in C.resblock_keys(cin, cout, 512, True)}
    if bias_shift:
        wl["Conv_2.bias"] = wl["Conv_2.bias"] + bias_shift
    return wl


def _run(tag, cin, cout, shp, bias_shift=0.0):
    """-> (block output, oracle output, labels of the launches the forward made)"""
    import _gpu as G
    from flowmse_amd import _lib
    from oracle import ncsnpp_oracle as O
    wl = _weights(cin, cout, tag, bias_shift)
    blk = G.Block("resnet", cin, cout, up=True, temb_dim=512).load(wl)
    x = torch.from_numpy(synth.normal(17, 31, shp))
    temb = torch.from_numpy(synth.normal(17, 32, (shp[0], 512)))
    ref = O.resblock(O._W({f"all_modules.0.{k}": v for k, v in wl.items()}), 0, x, temb, up=True)
    _lib.check(_lib.lib.flowse_profile_begin(blk.h, 1))
    got = blk(x, temb=temb)
    buf = Ct.create_string_buffer(1 << 16)
    _lib.check(_lib.lib.flowse_profile_end(blk.h, buf, len(buf)))
    labels = [k for k in json.loads(buf.value.decode()) if not k.startswith("_")]
    again = blk(x, temb=temb)
    assert torch.equal(got, again)
    return got, ref, labels


@pytest.mark.parametrize("tag,cin,cout,shp", UP)
def test_up_resblock_reordered_shortcut_vs_oracle(tag, cin, cout, shp):
    got, ref, labels = _run(tag, cin, cout, shp)
    err = C.rel_l2(got, ref)
    print(f"up resblock {tag}: rel-L2 vs oracle {err:.3e}; launches: {labels}")
    assert got.shape == ref.shape and err < TOL
    # the plan's own labels: the 1x1 runs at H x W and nowhere else, in particular not at 2H x 2W
    H, W = shp[2], shp[3]
    sc = [k for k in labels if k.startswith("conv2_1x1@")]
    assert sc == [f"conv2_1x1@{H}x{W}:{cin}>{cout}"], sc
    assert not any(k.startswith(f"conv2_1x1@{2 * H}x{2 * W}:") for k in labels)
    assert f"fir_up@{H}x{W}" in labels


def test_shortcut_bias_is_not_upsampled():
    """Conv_2's bias + 50: upsampled with the data it would lose 7/16 of 50 in the corners and 1/4 of 50 along the edges
    (rel-L2 of the order 1e-2 on this output), far outside the bound; added after the upsampling it is exact."""
    tag, cin, cout, shp = UP[1]
    got, ref, _ = _run(tag, cin, cout, shp, bias_shift=50.0)
    err = C.rel_l2(got, ref)
    d = (got - ref).abs()
    border = max(float(d[:, :, 0].max()), float(d[:, :, -1].max()), float(d[:, :, :, 0].max()), float(d[:, :, :, -1].max()))
    print(f"bias + 50: rel-L2 vs oracle {err:.3e}; max abs error on the border {border:.3e}, anywhere {float(d.max()):.3e}")
    assert err < TOL


def test_small_up_block_keeps_the_reference_order():
    """<= 2048 low-resolution pixels over the batch: the plan is unchanged (1x1 at the upsampled size)."""
    got, ref, labels = _run("b2_256_16", 256, 256, (2, 256, 16, 16))
    print(labels)
    assert C.rel_l2(got, ref) < TOL
    assert not any(k.startswith("conv2_1x1@16x16:") for k in labels)
