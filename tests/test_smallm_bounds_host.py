"""CPU: the bounds of tests/_smallm_ref.py are attainable and the case table is what it claims to be.

An fp32 torch restatement of every case of the small-image convolution tests (same operands, same single rounding,
another summation order) has to meet every assertion the GPU test makes; every case has to sit in the ring class its row
claims, and every kernel instance needs a case in every class.  A restatement that rounds before the residual is added
has to FAIL -- the defect the 16-bit ceilings of test_conv2d_16bit_storage cannot see.
"""
import pytest
import torch

import _smallm_ref as R


def test_every_instance_has_every_ring_class():
    assert len(R.INSTANCES) == 11
    for inst in R.INSTANCES:
        claimed = set()
        for c in R.CASES:
            if c.inst == inst and c.ring:
                claimed |= set(c.ring.split("+"))
        assert claimed == set(R.RING_CLASSES), (inst, set(R.RING_CLASSES) - claimed)


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_case_geometry_and_ring_class(c):
    D = R.INSTANCES[c.inst]
    s_all, nstep = R.ring_numbers(c)
    M = c.B * c.H * c.W
    assert 1 <= M <= 2048 and c.C1 % 32 == 0 and c.C2 % 32 == 0 and c.Cout % 32 == 0 and c.k in (1, 3)
    for ring in filter(None, c.ring.split("+")):
        assert ring in R.ring_classes_of(c), (c.name, ring, D, s_all, nstep)
    # the tile form the row's instance stands for (the library reports the route itself: the GPU test asserts it)
    mtiles = -(-M // 32)
    wide = c.Cout % 64 == 0 and mtiles * (c.Cout // 64) >= 256
    if c.inst == "smallm_tile16":
        assert M <= 256 and (c.H * c.W) % 16 == 0
    else:
        assert wide == (c.inst == "smallm<2>" or c.inst.startswith("smallm16b<2"))
        if c.dt is None:
            assert not (M <= 256 and (c.H * c.W) % 16 == 0)
        else:
            pb = min(c.H * c.W, 32)
            assert 32 % pb == 0 and (c.H * c.W) % pb == 0


def test_geometry_coverage():
    def has(pred):
        return any(pred(c) for c in R.CASES)
    full = lambda c: c.k == 3 and c.bias2 and c.res and c.scale != 1.0
    for inst in R.INSTANCES:
        wide = inst == "smallm<2>" or inst.startswith("smallm16b<2")
        mine = lambda g, **kw: has(lambda c: c.inst == inst and (c.B, c.H, c.W) == g and full(c) and
                                   all(getattr(c, k) == v for k, v in kw.items()))
        if wide:
            assert mine((8, 16, 16), Cout=256) and mine((255, 2, 4), Cout=256) and mine((1, 32, 32), Cout=512)
            assert mine((8, 16, 16), C1=256, C2=256)
        elif inst == "smallm_tile16":
            assert mine((1, 4, 4)) and mine((16, 4, 4)) and mine((3, 4, 8)) and mine((3, 4, 8), C1=64, C2=32)
        else:
            assert mine((2, 32, 32), C1=64, Cout=32) and mine((2, 32, 32), C1=64, Cout=96)
            for g in ((24, 1, 1), (32, 1, 1), (16, 1, 2), (5, 2, 4)):
                assert mine(g), (inst, g)
            assert has(lambda c: c.inst == inst and c.C1 == 64 and c.C2 == 32 and full(c))
        assert has(lambda c: c.inst == inst and c.k == 1)
        assert has(lambda c: c.inst == inst and not c.bias and not c.bias2)
    assert has(lambda c: c.inst == "smallm<1>" and (c.B, c.H, c.W) == (3, 6, 6) and full(c))


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_fp32_restatement_meets_the_bounds(c):
    fails, report = R.check(c, R.restate_fp32(c))
    print(f"{c.name:28s} {c.inst:28s} {report}")
    assert not fails, fails


@pytest.mark.parametrize("name", ["s16b1_bf16_out16-Dp1", "s16b1_f16_out16-24x1x1", "s16b2_bf16_out16-D", "s16b2_f16_out16-cat256"])
def test_rounding_before_the_residual_is_caught(name):
    """rounded twice, the result differs from round(ref) in about a quarter of the elements: far above the 2e-2 cap"""
    c = R.BY_NAME[name]
    fails, report = R.check(c, R.restate_fp32(c, defect="round_before_res"))
    print(f"{name}: {report}")
    assert any("differ from round(ref)" in f for f in fails), (fails, report)
