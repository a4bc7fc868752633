"""CPU: the bounds of tests/_conv16_ref.py are attainable, four restated defects miss them, and the case table is what it
claims to be.

An fp32 torch restatement of every row of the large-image 16-bit convolution tests (same operands, same single roundings,
another summation order, the staging written with exp2 and a reciprocal as the kernels write it) has to meet every
assertion the GPU test makes; the restated staging has to agree with round_dt(a64) bit for bit outside the ambiguous set;
every GroupNorm row has to keep the ambiguous set below 5 % of its inputs and the median of amb / (u |ref|) below 1.
Restatements with (a) zero padding before GroupNorm, (b) the output rounded before the residual is added, (c) the previous
sample's per-sample bias row and (d) the staged value rounded twice have to FAIL.  The table check redoes each row's
chunk count, items per block (for 256 compute units, the MI355X's count), border class and K-slice count.
"""
import pytest
import torch

import _conv16_ref as R

ROWS = [(c, dt) for c in R.CONV_CASES for dt in R.DTS]
ROW_IDS = [f"{c.name}-{dt}" for c, dt in ROWS]


@pytest.mark.parametrize("c,dt", ROWS, ids=ROW_IDS)
def test_fp32_restatement_meets_the_bounds(c, dt):
    ref = R.reference(c, dt)
    fails, report, _ = R.check(c, dt, R.restate_fp32(c, dt), ref)
    line = f"{c.name:32s} {dt:4s} {c.route:14s} {report}"
    if c.gn:
        share, med = R.gn_conditions(c, dt, ref)
        line += f"  ambiguous {share:.2e}  median amb/(u|ref|) {med:.3f}"
        assert share <= R.AMBIGUOUS_CAP, (c.name, dt, share)
        assert med <= 1.0, (c.name, dt, med)
    print(line)
    assert not fails, fails


@pytest.mark.parametrize("c", R.PROBE_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("dt", R.DTS)
def test_restated_staging_is_exact_outside_the_ambiguous_set(c, dt):
    """what the probe rows assert of the kernels, asserted of the fp32 restatement: the one-hot conv is an exact shift"""
    x = R.inputs(c).x
    got = torch.cat([torch.nn.functional.pad(R.restate_staging(c, dt, x), (1, 1, 1, 1))[:, :, t // 3:t // 3 + c.H,
                                                                                         t % 3:t % 3 + c.W] for t in range(9)], 1)
    fails, report = R.check_probe(c, dt, got)
    print(f"{c.name:32s} {dt:4s} {report}")
    assert not fails, fails
    if c.gn:
        assert float(R.staged(c, dt).A.double().mean()) <= R.AMBIGUOUS_CAP


DEFECTS = {"pad_before_gn": ("pc-geo-64x16x16", "halo-8x8x256", "head4-64x16x16-gnsilu"),
           "round_before_res": ("pc-epi-plain", "halo-6x24x128-plain", "flat-3x3-64x64"),
           "bias2_next_sample": ("pc-geo-17x32x32", "halo-22x24x16-256", "flat-1x1-cat"),
           # (K = 288 rows: the accumulation allowance grows with K and the second rounding's error with sqrt(K) -- at K = 1152
           #  in fp16 the element bound no longer separates the two, max |d| / bound 0.80 on pc-chunks-128)
           "round_twice": ("pc-geo-1x128x128", "halo-6x24x128-32+0", "head4-4x64x64-32")}


@pytest.mark.parametrize("defect,name", [(d, n) for d, ns in DEFECTS.items() for n in ns])
@pytest.mark.parametrize("dt", R.DTS)
def test_restated_defects_miss_the_bounds(defect, name, dt):
    c = R.BY_NAME[name]
    fails, report, _ = R.check(c, dt, R.restate_fp32(c, dt, defect=defect))
    print(f"{defect:18s} {name:28s} {dt:4s} {report}")
    assert fails, (defect, name, dt, report)


def test_probe_catches_padding_before_groupnorm():
    """the probe's out-of-image zeros: a staging that pads first leaves act(b - m s) there"""
    c = R.BY_NAME["probe-pc16-one-gnsilu"]
    x = R.inputs(c).x
    padded = R.restate_staging(c, "bf16", torch.nn.functional.pad(x, (1, 1, 1, 1)))
    got = torch.cat([padded[:, :, t // 3:t // 3 + c.H, t % 3:t % 3 + c.W] for t in range(9)], 1)
    fails, _ = R.check_probe(c, "bf16", got)
    assert any("out-of-image" in f for f in fails), fails


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_row_sits_in_the_class_it_claims(c):
    assert c.route in R.ROUTES and c.C1 % 32 == 0 and c.C2 % 32 == 0 and c.k in (1, 3)
    assert c.chunks == (c.C1 + c.C2) // 32 and c.sc == (c.X1 + c.X2) // 32
    M = c.B * c.H * c.W
    if c.route == "pc16":
        assert c.k == 3 and c.H % 16 == 0 and c.W % 16 == 0 and c.Cout % 128 == 0 and not c.out32
        assert (M // 256) * (c.Cout // 128) >= 64                       # the persistent kernel's smallest launch
        assert c.ipb == (R.items_per_block(c, 2), R.items_per_block(c, 1)), (R.items_per_block(c, 2), R.items_per_block(c, 1))
        assert c.border == R.border_of(c)
        if c.kind == "fold":
            assert c.sc >= 3 and not c.bias2 and not c.res and c.C2 == 0
    elif c.route == "halo16":
        assert c.k == 3 and c.H % 16 == 8 and c.W % 16 == 0 and c.Cout % 128 == 0 and not c.out32
        assert (M // 128) * (c.Cout // 128) >= 128
        assert c.border == R.border_of(c)
    elif c.route == "head4_16":
        assert c.k == 3 and c.Cout == 4 and c.C2 == 0 and c.H % 16 == 0 and c.W % 16 == 0 and c.out32 and not c.bias2
        assert c.B * (c.H // 16) * (c.W // 16) >= 64
        assert c.border == R.border_of(c)
    else:
        assert c.gn == 0 and M > 2048                                    # above the small-image kernel's limit
        halo = c.k == 3 and c.H % 8 == 0 and c.W % 16 == 0 and c.Cout % 128 == 0 and (M // 128) * (c.Cout // 128) >= 128
        assert c.out32 or not halo
        assert c.ks == R.ksplit_of(c), R.ksplit_of(c)
        assert c.route == ("flat16_splitk" if c.ks > 1 else "flat16")
    if c.route not in ("flat16", "flat16_splitk"):
        assert c.ks == 0


def test_table_coverage():
    def has(pred):
        return any(pred(c) for c in R.CASES)
    assert {c.route for c in R.CASES} == set(R.ROUTES)
    for route in ("pc16", "halo16", "head4_16"):
        assert {c.gn for c in R.CASES if c.route == route and c.kind == "conv"} == {0, 1, 2}, route
    for route in ("pc16", "halo16"):
        assert {(c.gn, c.C2 != 0) for c in R.PROBE_CASES if c.route == route} == {(g, s) for g in (0, 1, 2) for s in (False, True)}
    assert {c.gn for c in R.CASES if c.kind == "fold"} == {0, 1, 2}
    # pc16: every residue of the three halo buffers / the three-entry B ring, one and several items per block, every border class
    pc = [c for c in R.CASES if c.route == "pc16" and c.kind == "conv"]
    assert {c.chunks for c in pc} >= {1, 2, 3, 4, 5, 8} and {c.chunks % 3 for c in pc} == {0, 1, 2}
    assert {c.border for c in pc} == set(R.BORDERS)
    assert {c.ipb[0] for c in pc} >= {(1, 1), (1, 2)} and {c.ipb[1] for c in pc} >= {(1, 1), (1, 2), (2, 3)}
    assert {(c.X1, c.X2) for c in R.CASES if c.kind == "fold"} == {(96, 0), (128, 0), (160, 0), (64, 32), (32, 64), (256, 256)}
    assert has(lambda c: c.kind == "fold" and c.ipb[1] == (2, 3))
    assert {c.border for c in R.CASES if c.route == "halo16"} >= {"strip_tb", "strip_lr", "interior"}
    assert has(lambda c: c.route == "halo16" and c.C2) and has(lambda c: c.route == "pc16" and c.kind == "conv" and c.C2)
    flat = [c for c in R.CASES if c.route.startswith("flat16")]
    assert {c.k for c in flat} == {1, 3} and {c.out32 for c in flat} == {False, True} and {c.ks > 1 for c in flat} == {False, True}
    assert has(lambda c: c in flat and (c.B * c.H * c.W) % 128 and c.k == 1) and has(lambda c: c in flat and (c.B * c.H * c.W) % 128 and c.k == 3)
    assert has(lambda c: c in flat and c.bias2) and has(lambda c: c in flat and c.C2)
    head = [c for c in R.CASES if c.route == "head4_16"]
    assert {c.C1 for c in head} == {32, 64, 96, 128} and {c.res for c in head} == {False, True}
    assert {(c.B, c.H, c.W) for c in head} == {(64, 16, 16), (1, 128, 128), (4, 64, 64)}
    for name in R.REPRO:
        assert name in R.BY_NAME
