"""GPU: every instance of the small-image split-K convolution kernels (conv_smallm.hip: smallm<1>, smallm<2>, smallm_tile16;
conv16_smallm.hip: smallm16b<NT2, bf16 | f16, out16 | out32>) against float64, at every edge of the register ring and of
the tile geometry.  Cases, reference and bounds: tests/_smallm_ref.py (tests/test_smallm_bounds_host.py shows on the CPU
that the bounds are attainable and that a kernel rounding twice misses them).

Every case first asserts that the launch ran the instance its row names (flowse_op_last_conv_route: recorded by the
launcher, not re-derived from the shape), then the element bound on every element and the second check (rel-L2 for fp32
output; the share of elements that differ from the once-rounded reference for 16-bit output).  The fused GroupNorm
statistics of these kernels are held to float64 in tests/test_gpu_fused_stats.py (here the statistics sink is not armed:
the op entries launch with stats = nullptr).
"""
import pytest
import torch

import _smallm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import _gpu
    return _gpu


def run_case(G, c):
    x, w, bias, bias2, res = R.inputs(c)
    x1 = x[:, :c.C1].contiguous()
    x2 = x[:, c.C1:].contiguous() if c.C2 else None
    if c.dt is None:
        got = G.conv2d(x1, w, bias, x2, bias2, res, c.scale, splitk=True)
    else:
        got = G.conv2d_16(x1, w, R.DT_CODE[c.dt], bias, x2, bias2, res, c.scale, out_f32=c.out32)
    return got, G.last_route()


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_smallm_against_float64(G, c):
    got, route = run_case(G, c)
    assert route == c.inst, f"{c.name}: ran {route!r}, the case is written for {c.inst!r}"
    fails, report = R.check(c, got)
    s_all, nstep = R.ring_numbers(c)
    print(f"{c.name:30s} route {route:28s} nstep {nstep:2d} S_all {s_all:3d}  {report}")
    assert not fails, fails


def test_every_instance_name_was_asserted():
    """the case table names all eleven instances (each case asserts its route above)"""
    assert {c.inst for c in R.CASES} == set(R.INSTANCES) and len(R.INSTANCES) == 11


def test_smallm_is_bit_reproducible(G):
    """the eight partial tiles are summed in a fixed order: two launches agree bit for bit"""
    for name in ("s1-Dp1", "s2-ragged", "s_tile16-cat96", "s16b1_bf16_out16-Dp1", "s16b2_f16_out32-cat256"):
        c = R.BY_NAME[name]
        a, _ = run_case(G, c)
        b, _ = run_case(G, c)
        assert torch.equal(a, b), name
