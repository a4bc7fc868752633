"""What conv_route names is what runs.

For each kernel family, the cheapest shape the predicates route to it (fewest pixels x channels on a grid of image sides
2 ... 256 and channel counts 16 ... 256, searched on the CPU with flowse_op_conv_route) goes through the per-op entry that
reaches the family, with the offer that entry makes.  The launcher's own record (flowse_op_last_conv_route, written next
to the launch) must start with the name the route query gives for the same shape and offer, and the result must be within
the bound the existing test of that entry uses: rel-L2 against torch's fp32 conv of 2e-5 in fp32, 4e-3 in bf16 and 5e-4 in
fp16.  test_cases_name_their_family needs no GPU: it holds every row of CASES to the family it is listed under.

Not here: halo_bf16x3 (and halo16 on fp32 storage) -- no per-op entry offers the 16-bit weight planes beside fp32
activations; only a model handle in the bf16x3 / bf16 / fp16 operand modes does (tests/test_gpu_model.py runs those,
tests/plan_pins.json pins their plan, tests/conv_route_pins.txt their route).  Error routes are checked on the CPU only
(tests/test_conv_route_host.py): nothing here asks for a shape no kernel takes.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _cases as C
from flowmse_amd.util import synth

WINO, WINO2, WSM, WFRAG, WQ, WQ3, WQF16, SLAB, GN = (1 << i for i in range(9))      # FLOWSE_OFFER_* of include/flowse_hip.h
BOUND = {0: 2e-5, 1: 4e-3, 2: 5e-4}

# family, entry, storage type (0 fp32, 1 bf16, 2 fp16), fp32 output of a 16-bit conv, (B, H, W, Cin, Cout, taps), offer.
# Entries: "conv2d" = flowse_op_conv2d without scratch (offers nothing), "conv2d+scratch" = with it (the fragment-order copy
# or the slab), "gn" = flowse_op_conv3x3_gn, "f43" / "w2d" = the Winograd entries, "16" = flowse_op_conv2d_16_ex (its
# scratch holds the 16-bit weights, their fragment-order copy and the slab)
O16 = WQ | WFRAG | SLAB
CASES = [
    ("flat", "conv2d", 0, False, (1, 2, 2, 16, 16, 1), 0),
    ("flat_splitk", "conv2d+scratch", 0, False, (1, 2, 2, 16, 16, 9), WSM | SLAB),
    ("smallm", "conv2d+scratch", 0, False, (1, 2, 2, 32, 32, 1), WSM | SLAB),
    ("1x1_stream", "conv2d+scratch", 0, False, (2, 128, 128, 32, 256, 1), WSM | SLAB),
    ("head4", "conv2d", 0, False, (1, 128, 128, 32, 4, 9), 0),
    ("halo", "gn", 0, False, (1, 24, 96, 128, 64, 9), GN),
    ("f43_splitk", "f43", 0, False, (1, 24, 96, 128, 64, 9), WINO | SLAB),
    ("f43", "f43", 0, False, (1, 128, 128, 32, 128, 9), WINO | SLAB),
    ("w2d", "w2d", 0, False, (1, 128, 128, 32, 128, 9), WINO2),
    ("flat16", "16", 1, False, (1, 2, 2, 32, 16, 1), O16),
    ("flat16_splitk", "16", 1, False, (1, 2, 2, 256, 16, 1), O16),
    ("smallm16b", "16", 1, False, (1, 2, 2, 32, 32, 1), O16),
    ("halo16", "16", 1, False, (8, 8, 128, 32, 256, 9), O16),
    ("pc16", "16", 1, False, (1, 64, 128, 32, 256, 9), O16),
    ("head4_16", "16", 1, True, (1, 128, 128, 32, 4, 9), O16),
    ("pc16", "16", 2, False, (1, 64, 128, 32, 256, 9), O16 | WQF16),
    ("flat16_splitk", "16", 2, False, (1, 2, 2, 256, 16, 1), O16 | WQF16),
    # a 4-channel fp32 input: the VALU kernel (3x3, 1x1), the matrix-core kernel (the smallest batch of whole 128-pixel
    # tiles that reaches 32768 pixels), and a width those kernels refuse (24 / 4 = 6 does not divide 256): the flat kernel
    ("cin4", "conv2d", 0, False, (1, 2, 2, 4, 16, 9), 0),
    ("cin4", "conv2d", 0, False, (1, 2, 2, 4, 16, 1), 0),
    ("cin4_mfma", "conv2d", 0, False, (2, 128, 128, 4, 128, 9), 0),
    ("flat", "conv2d", 0, False, (1, 2, 2, 4, 24, 9), 0),
]
IDS = [f"{c[0]}-{('f32', 'bf16', 'f16')[c[2]]}" for c in CASES]
IDS = [i if i not in IDS[:n] else f"{i}-{c[4][3]}to{c[4][4]}x{c[4][5]}" for n, (i, c) in enumerate(zip(IDS, CASES))]   # a family's further cases: + the shape


def route_of(case):
    from flowmse_amd import _lib
    family, entry, dt, out32, (B, H, W, Cin, Cout, taps), offer = case
    buf = ctypes.create_string_buffer(96)
    assert _lib.lib.flowse_op_conv_route(dt, 0 if out32 else dt, B, H, W, Cin, 0, Cout, taps, offer, buf, 96) == 0
    return buf.value.decode().split()[0]


def test_cases_name_their_family():
    assert [route_of(c) for c in CASES] == [c[0] for c in CASES]
    assert {c[0] for c in CASES} == {"head4", "head4_16", "smallm", "1x1_stream", "w2d", "f43", "f43_splitk", "halo", "halo16",
                                     "pc16", "smallm16b", "flat", "flat_splitk", "flat16", "flat16_splitk", "cin4", "cin4_mfma"}
    assert len(set(IDS)) == len(IDS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_route_is_what_runs(case):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import _gpu as G
    family, entry, dt, out32, (B, H, W, Cin, Cout, taps), offer = case
    k = 3 if taps == 9 else 1
    x = torch.from_numpy(synth.normal(83, 1, (B, Cin, H, W)))
    w = torch.from_numpy(synth.normal(83, 2, (Cout, Cin, k, k), (1.0 / (Cin * taps)) ** 0.5))
    bias = torch.from_numpy(synth.normal(83, 3, (Cout,), 0.1))
    if entry == "gn":                                     # the entry normalises its input: GroupNorm + SiLU, then the conv
        gamma = 1.0 + torch.from_numpy(synth.normal(83, 4, (Cin,), 0.1))
        beta = torch.from_numpy(synth.normal(83, 5, (Cin,), 0.1))
        ref = F.conv2d(F.silu(F.group_norm(x, min(Cin // 4, 32), gamma, beta, eps=1e-6)), w, bias, padding=1)
        got = G.conv3x3_gn(x, gamma, beta, w, bias)
    else:
        ref = F.conv2d(x, w, bias, padding=k // 2)
        if entry in ("f43", "w2d"):
            got = G.conv3x3_f43(x, w, bias=bias, form=entry)
        elif entry == "16":
            got = G.conv2d_16(x, w, dt, bias, out_f32=out32)
        else:
            got = G.conv2d(x, w, bias, splitk=entry == "conv2d+scratch")
    ran, want, err = G.last_route(), route_of(case), C.rel_l2(got, ref)
    print(f"{family:14s} {entry:15s} B{B} {H}x{W} {Cin}>{Cout}/{taps}: ran {ran!r}, route {want!r}, rel-L2 {err:.3e} (bound {BOUND[dt]:.0e})")
    # (the small-image launchers record their instance behind the family: "smallm<2>", "smallm16b<1, bf16, out16>")
    assert want == family and (ran == want or (want.startswith("smallm") and ran.startswith(want))), (ran, want)
    assert err < BOUND[dt], err
