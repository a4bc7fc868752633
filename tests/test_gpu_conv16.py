"""GPU: the large-image 16-bit storage convolution kernels -- conv3x3_pc16_kernel (NJ = 1 and 2, GN variants 0 / 1 / 2,
with and without the folded 1x1 shortcut), conv3x3_halo_bf16_kernel<1, ...> in the storage modes, conv_flat16_kernel with
its K slices and the reduction launch, conv3x3_head4_16_kernel -- against float64, per element.  Cases, reference, tau and
the bounds: tests/_conv16_ref.py (tests/test_conv16_bounds_host.py shows on the CPU that the bounds are attainable, that
four restated defects miss them and that every row sits in the edge class it claims).

Every row first asserts that the launch ran the kernel its row names (flowse_op_last_conv_route: recorded by the
launcher), then the element bound on every element and, without fused GroupNorm, the second check.  pc16 rows run with
128- and with 64-channel blocks (flowse_op_pc16_channel_blocks(0) / (1)); every row runs in bf16 and fp16.  The probe rows
(one-hot weights: output block t = the staged operand of tap t) are compared bit for bit.  The fused GroupNorm
statistics of these kernels are held to float64 in tests/test_gpu_fused_stats.py (here the statistics sink is not armed:
the op entries launch with stats = nullptr).

Recorded on an MI355X (worst over the rows of a route and type: max |d| / bound, mismatch share of the rows without
fused GN; fp32-output rows: rel-L2):
    route           type  output  launches  max|d|/bound  excess/acc  mismatch or rel-L2 (rows without GN)
    flat16          bf16  out16          1         0.991       0.000  2.95e-05
    flat16          bf16  out32          1         0.021       0.021  5.03e-08
    flat16          f16   out16          1         0.977       0.000  2.62e-04
    flat16          f16   out32          1         0.022       0.022  5.46e-08
    flat16_splitk   bf16  out16          4         0.953       0.000  1.03e-04
    flat16_splitk   bf16  out32          3         0.002       0.002  8.39e-08
    flat16_splitk   f16   out16          4         0.812       0.000  7.55e-04
    flat16_splitk   f16   out32          3         0.002       0.002  9.30e-08
    halo16          bf16  out16         11         0.977       0.001  7.08e-05
    halo16          f16   out16         11         0.867       0.001  6.02e-04
    head4_16        bf16  out32         19         0.648       0.002  7.89e-08
    head4_16        f16   out32         19         0.509       0.003  1.11e-07
    pc16            bf16  out16         46         0.980       0.001  8.84e-05
    pc16            f16   out16         46         0.887       0.002  6.35e-04
    pc16 + fold     bf16  out16         52         0.936       0.001  1.50e-04
    pc16 + fold     f16   out16         52         0.679       0.001  1.13e-03
  (max |d| / bound close to 1 is the output rounding itself: half a storage step against u |ref|; excess/acc is what is
   left of |d| beyond u |ref| + amb, as a share of acc)
  probe rows: bit-exact outside the ambiguous set, exactly 0 at every out-of-image tap; inside the set (largest share
  of the staged inputs / elements rounded the other way):
    halo16  bf16  ambiguous <= 1.79e-03, 111 of 11379 ambiguous elements flipped
    halo16  f16   ambiguous <= 1.18e-02, 561 of 76555 ambiguous elements flipped
    pc16    bf16  ambiguous <= 1.97e-03, 306 of 22782 ambiguous elements flipped
    pc16    f16   ambiguous <= 1.29e-02, 1332 of 147254 ambiguous elements flipped
"""
import pytest
import torch

import _conv16_ref as R

pytestmark = pytest.mark.gpu

_ran = {}                                    # pc16 row name -> channel-block settings it ran under


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import _gpu
    return _gpu


def run_case(G, c, dt):
    i = R.inputs(c)
    x1 = i.x[:, :c.C1].contiguous()
    x2 = i.x[:, c.C1:].contiguous() if c.C2 else None
    gn = (i.mean, i.scl, i.beta) if c.gn else None
    if c.kind == "fold":
        xs1 = i.xs[:, :c.X1].contiguous()
        xs2 = i.xs[:, c.X1:].contiguous() if c.X2 else None
        got = G.resblock_tail_16(x1, i.w, R.DT_CODE[dt], i.bias, xs1, i.w2, i.bias_x, xs2, gn, c.gn == 2, c.scale)
    else:
        got = G.conv2d_16(x1, i.w, R.DT_CODE[dt], i.bias, x2, i.bias2, i.res, c.scale, out_f32=c.out32, gn=gn,
                          silu=c.gn == 2)
    return got, G.last_route()


def each_setting(c, fn):
    """pc16 rows: fn(blocks) under both channel-block widths, reset afterwards; other routes: fn(-1), the default"""
    from flowmse_amd import _lib
    if c.route != "pc16":
        fn(-1)
        return
    try:
        for blocks in (0, 1):
            _lib.check(_lib.lib.flowse_op_pc16_channel_blocks(blocks))
            _ran.setdefault(c.name, set()).add(blocks)
            fn(blocks)
    finally:
        _lib.check(_lib.lib.flowse_op_pc16_channel_blocks(-1))


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("c", R.CONV_CASES, ids=lambda c: c.name)
def test_conv16_against_float64(G, c, dt):
    ref = []

    def one(blocks):
        got, route = run_case(G, c, dt)
        assert route == c.route, f"{c.name}: ran {route!r}, the row is written for {c.route!r}"
        if not ref:
            ref.append(R.reference(c, dt))
        fails, report, _ = R.check(c, dt, got, ref[0])
        print(f"{c.name:32s} {dt:4s} route {route:14s} blocks {blocks:2d} gn {c.gn}  {report}")
        assert not fails, (blocks, fails)
    each_setting(c, one)


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("c", R.PROBE_CASES, ids=lambda c: c.name)
def test_staged_halo_probe_is_bit_exact(G, c, dt):
    def one(blocks):
        got, route = run_case(G, c, dt)
        assert route == c.route, f"{c.name}: ran {route!r}, the row is written for {c.route!r}"
        fails, report = R.check_probe(c, dt, got)
        print(f"{c.name:32s} {dt:4s} route {route:14s} blocks {blocks:2d}  {report}")
        assert not fails, (blocks, fails)
    each_setting(c, one)


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("name", R.REPRO)
def test_conv16_is_bit_reproducible(G, name, dt):
    """pc16 with several items per block, halo16, flat16 with K slices: two launches agree bit for bit"""
    c = R.BY_NAME[name]

    def one(blocks):
        a, _ = run_case(G, c, dt)
        b, _ = run_case(G, c, dt)
        assert torch.equal(a, b), (name, dt, blocks)
    each_setting(c, one)


def test_route_coverage():
    """the table names exactly the five routes (each row asserts its own above); pc16 rows cover the three GN modes and,
    where they ran in this session, both channel-block settings"""
    assert {c.route for c in R.CASES} == {"pc16", "halo16", "flat16", "flat16_splitk", "head4_16"}
    assert {c.gn for c in R.CASES if c.route == "pc16"} == {0, 1, 2}
    for name, blocks in _ran.items():
        assert blocks == {0, 1}, (name, blocks)
