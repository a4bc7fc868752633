"""GPU: the GroupNorm statistics every conv kernel fuses into its output stage, and the kernels that merge them, against float64.

Producers.  Almost every GroupNorm of the network normalises with statistics it never measured: the kernel that writes a
tensor leaves one (mean, M2) partial per sample, pixel block and channel, gn_finalize merges them.  Each route below is
launched ONCE through its per-op entry under the statistics sink (flowse_op_stats_sink: the entry sets ConvArgs::stats and
the stats_nblk of the route of exactly the arguments it launches).  The case asserts the kernel the launcher recorded
(flowse_op_last_conv_route; a case that lands elsewhere fails), that exactly B * nblk * Cout pairs were written, and that
the float64 Chan merge of the partials (tests/_stats_ref.py) reproduces the float64 statistics of the tensor the launch
stored, per (sample, group), G = min(C / 4, 32):
    e_mean = |mu - mu_ref| / sigma_ref,    e_var = |var / var_ref - 1|.
Only group statistics are specified (pc16 gives both channels of a pair the pair's joint values).

Data sets: (a) benign; (b) per-channel bias ramp, per-sample bias, residual and scale != 1 wherever the entry takes them
(statistics taken before the residual or the scale, or a wrong channel index, show here); (c) a large mean -- bias 50 and
1000 on a unit-variance output for fp32 storage, 8 for 16-bit storage -- which multiplies a wrong count or a dropped
element by mu / sigma.

Bounds.     e_mean <= 2^-22 |mu_ref| / sigma_ref + C_M,      e_var <= C_V
(2^-22 |mu|: the partial means are fp32 numbers).  C_M and C_V are 4 x the smallest constants with which the STAND-ALONE
gn_stats kernel (norm.hip; tested on its own in test_gpu_ops.py) meets the same two inequalities on the same stored tensors,
in blocks of the same count: the fused kernels sum the same fp32 values, at most 256 per partial, in another order.  For
fp32 storage the constants must also respect C_M <= 1e-5, C_V <= 6e-5 (a pivoted fp32 sum of n <= 256 terms cannot
legitimately exceed n 2^-24 by more), for 16-bit storage both errors additionally stay below 2^-13, a quarter of fp16's
rounding step.  Every case prints its figures (pytest -s) before it asserts.

Shapes: the smallest for which the host-side route query (flowse_op_conv_route) names the kernel under the entry's own
offer.  halo16 needs an image the producer / consumer kernel does not take (H = 8 mod 16: the 16-bit entry always offers
the fragment-order copy, so every pc16 shape runs pc16).  halo_bf16x3 is not here: no per-op entry offers the split bf16
planes.

Finalize.  flowse_op_gn_finalize on synthetic partials (and once on a real launch's) against the float64 merge of the same
partials: mean within 1 fp32 ulp, scale = rstd * gamma within 2^-22 relative (the kernel sums in fp64: the two final
roundings remain).  The cases drive every branch of gn_group_stats: items per (group, set) <= 256, 257-512, 513-768,
769-1024, 2048 and 1600 (full rounds and a remainder of two or three), a short last block, two sets with different block
counts and a straddling group, |mean| = 1000 sigma.  The finalize + apply form is held to float64 GroupNorm with
test_group_norm's bound.

Recorded on an MI355X (worst over the data sets of a route; c_mean = e_mean - 2^-22 |mu_ref| / sigma_ref):
    route               type  nblk    c_mean, all sets      e_var, (a) (b)      e_var, (c)
                                      fused     alone       fused    alone      fused    alone
    halo                f32      8   +3.87e-09 +1.58e-08   2.87e-08 6.00e-08   3.25e-06 1.62e-06
    f43                 f32      8   +4.83e-09 +1.59e-08   2.90e-08 6.65e-08   3.08e-06 1.77e-06
    f43_splitk          f32    128   +2.28e-09 +2.28e-09   9.28e-09 9.28e-09   2.27e-06 2.27e-06
    w2d                 f32     32   +2.93e-09 +4.65e-09   1.47e-08 2.33e-08   1.72e-06 1.61e-06
    w2d-concat          f32     32   +2.13e-09 +5.11e-09   1.42e-08 2.41e-08   1.37e-06 1.26e-06
    smallm-16px         f32     16   +1.84e-09 +3.15e-09   1.85e-08 2.38e-08   6.10e-06 4.62e-06
    smallm-32px         f32      8   +5.17e-09 +6.73e-09   3.55e-08 3.26e-08   8.68e-06 5.17e-06
    smallm-4x1          f32      1   +6.94e-09 +1.27e-08   7.53e-08 6.71e-08   3.30e-05 1.71e-05
    1x1_stream          f32     16   +4.02e-09 +1.28e-08   2.34e-08 8.30e-08   1.25e-06 1.00e-06
    flat                f32     32   +2.66e-09 +2.66e-09   2.06e-08 2.06e-08   2.12e-06 2.12e-06
    flat_splitk         f32    128   +1.33e-09 +1.33e-09   1.08e-08 1.08e-08   1.98e-06 1.98e-06
    cin4_stats          f32      8   +8.60e-09 +8.60e-09   5.48e-08 5.48e-08   5.24e-06 5.24e-06
    cin4_stats-inplace  f32      8   +1.14e-08 +1.14e-08   4.78e-08 4.78e-08   3.21e-06 3.21e-06
    cin4_mfma           f32    128   +2.20e-09 +2.20e-09   1.24e-08 1.24e-08   7.31e-07 7.31e-07
    halo16              bf16     3   +1.94e-09 +1.34e-09   6.87e-08 1.32e-07   5.33e-08 2.35e-08
    halo16              f16      3   +2.28e-09 +3.73e-09   8.21e-08 1.19e-07   7.52e-08 5.71e-08
    pc16                bf16     8   +2.16e-10 +7.25e-10   3.75e-08 9.70e-08   3.06e-08 1.72e-08
    pc16                f16      8   +2.80e-10 +1.94e-09   4.65e-08 1.16e-07   5.03e-08 2.91e-08
    pc16-fold           bf16     8   +4.09e-10 +4.88e-10   3.08e-08 1.02e-07   4.05e-08 2.75e-08
    pc16-fold           f16      8   +3.20e-10 +1.41e-09   4.63e-08 9.68e-08   5.10e-08 8.59e-08
    smallm16b           bf16     8   -1.13e-10 +5.51e-10   3.91e-08 1.65e-08   2.36e-07 1.51e-08
    smallm16b           f16      8   -1.97e-10 +4.61e-10   2.52e-08 3.33e-08   8.08e-08 2.63e-08
    flat16              bf16    32   +6.89e-10 +6.89e-10   4.10e-08 4.10e-08   1.53e-08 1.53e-08
    flat16              f16     32   +4.62e-10 +4.62e-10   4.20e-08 4.20e-08   3.24e-08 3.24e-08
    flat16_splitk       bf16   128   +2.60e-10 +2.60e-10   1.01e-08 1.01e-08   1.46e-08 1.46e-08
    flat16_splitk       f16    128   +3.05e-10 +3.05e-10   6.72e-09 6.72e-09   1.54e-08 1.54e-08
    worst stand-alone    f32           c_mean 1.592e-08           e_var 8.298e-08     e_var 1.713e-05
    worst stand-alone    bf16 / f16    c_mean 3.726e-09           e_var 1.315e-07     e_var 8.592e-08
(f32 (c): 4 x 1.713e-05 = 6.9e-05 is above the condition C_V <= 6e-05, which therefore is the bound: the 4 x 1 image, whose
partials hold four pixels each, at |mu| = 1000 sigma.)  Before the deviations of the half-precision drain of
conv3x3_pc16_kernel were taken in fp32 its rows read: pc16 f16 c_mean +1.24e-05, e_var 4.53e-05 / 2.51e-06; pc16-fold f16
+1.09e-05, 2.68e-05 / 8.94e-06 -- three orders above every other producer and above 4 x the stand-alone kernel.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cases as C
import _stats_ref as S

pytestmark = pytest.mark.gpu

# 4 x the stand-alone columns of the table above.  C_M: one per storage (its worst is in (a) / (b): on the large means the
# stand-alone kernel stays inside the 2^-22 term alone).  C_V: per storage and data class -- (a) / (b), and the large means
# (c), where the variance error of any fp32 partial mean grows with |mu| / sigma.
C_M = {"f32": 4 * 1.592e-08, "16": 4 * 3.726e-09}
C_V = {("f32", "ab"): 4 * 8.298e-08, ("f32", "c"): min(4 * 1.713e-05, 6e-5), ("16", "ab"): 4 * 1.315e-07, ("16", "c"): 4 * 8.592e-08}
CEIL16 = 2.0 ** -13
assert C_M["f32"] <= 1e-5 and max(C_V["f32", "ab"], C_V["f32", "c"]) <= 6e-5
assert max(C_M["16"], C_V["16", "ab"], C_V["16", "c"]) <= CEIL16


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import _gpu
    return _gpu


class Case:
    def __init__(self, name, route, entry, B, H, W, C1, Cout, taps, C2=0, inplace=False, X1=0):
        self.name, self.route, self.entry = name, route, entry
        self.B, self.H, self.W, self.C1, self.C2, self.Cout, self.taps = B, H, W, C1, C2, Cout, taps
        self.inplace, self.X1 = inplace, X1


# entry: conv2d (no scratch: nothing offered), conv2d+s (scratch: fragment-order copy or slab), f43, w2d, conv16 (flowse_op_conv2d_16_ex),
# tail16 (flowse_op_resblock_tail_16)
CASES32 = [
    Case("halo", "halo", "conv2d", 4, 32, 32, 256, 256, 9),
    Case("f43", "f43", "f43", 8, 32, 32, 256, 256, 9),                       # the smallest whole-K F(4,3) launch of the query
    Case("f43_splitk", "f43_splitk", "f43", 4, 32, 32, 256, 256, 9),
    Case("w2d", "w2d", "w2d", 4, 64, 32, 128, 256, 9),
    Case("w2d-concat", "w2d", "w2d", 4, 64, 32, 64, 256, 9, C2=64),
    Case("smallm-16px", "smallm_tile16", "conv2d+s", 1, 16, 16, 256, 256, 9),
    Case("smallm-32px", "smallm<", "conv2d+s", 2, 16, 16, 256, 256, 9),
    Case("smallm-4x1", "smallm<", "conv2d+s", 1, 4, 1, 256, 256, 9),
    Case("1x1_stream", "1x1_stream", "conv2d+s", 8, 64, 64, 128, 256, 1),
    Case("flat", "flat", "conv2d+s", 1, 64, 64, 128, 128, 1),
    Case("flat_splitk", "flat_splitk", "conv2d+s", 4, 32, 32, 256, 256, 1),
    Case("cin4_stats", "cin4_stats", "conv2d", 1, 64, 16, 4, 128, 1),
    Case("cin4_stats-inplace", "cin4_stats", "conv2d", 1, 64, 16, 4, 128, 1, inplace=True),
    Case("cin4_mfma", "cin4_mfma", "conv2d", 2, 256, 64, 4, 128, 9),
]
CASES16 = [
    Case("halo16", "halo16", "conv16", 22, 24, 16, 32, 256, 9),
    Case("pc16", "pc16", "conv16", 8, 32, 32, 256, 256, 9),
    Case("pc16-fold", "pc16", "tail16", 8, 32, 32, 256, 256, 9, X1=128),
    Case("smallm16b", "smallm16b<", "conv16", 1, 16, 16, 256, 256, 9),
    Case("flat16", "flat16", "conv16", 1, 64, 64, 128, 128, 1),
    Case("flat16_splitk", "flat16_splitk", "conv16", 4, 32, 32, 256, 256, 1),
]
DT = {"bf16": 1, "f16": 2}


def randn(seed, shape, std=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


@functools.lru_cache(maxsize=2)
def operands(c):
    """inputs and weights of a case, shared by its data sets.  The weights give a unit-variance output: a 3 x 3 window has
    (3 H - 2) (3 W - 2) / (H W) of its nine taps inside the image on average (2.5 at 4 x 1)"""
    Cin, k = c.C1 + c.C2, 3 if c.taps == 9 else 1
    taps_in = (3 * c.H - 2) * (3 * c.W - 2) / (c.H * c.W) if k == 3 else 1.0
    x1 = randn(1, (c.B, c.C1, c.H, c.W))
    x2 = randn(2, (c.B, c.C2, c.H, c.W)) if c.C2 else None
    w = randn(3, (c.Cout, Cin, k, k), (1.0 / (Cin * taps_in)) ** 0.5)
    xs = randn(4, (c.B, c.X1, c.H, c.W)) if c.X1 else None
    ws = randn(5, (c.Cout, c.X1, 1, 1), (1.0 / c.X1) ** 0.5) if c.X1 else None
    return x1, x2, w, xs, ws


def launch(G, c, data, dt):
    """one launch of the case's entry under the sink -> (stored tensor NHWC float64, partial [B, nblk, Cout, 2] float64)"""
    x1, x2, w, xs, ws = operands(c)
    bias = bias2 = res = None
    scale = 1.0
    if data == "b":
        bias = torch.linspace(-2.0, 2.0, c.Cout) + randn(6, (c.Cout,), 0.1)         # channel means differ inside a group
        bias2 = randn(7, (c.B, c.Cout + 8), 0.5)
        res = randn(8, (c.B, c.Cout, c.H, c.W))
        scale = 0.70710678
    elif data.startswith("c"):
        bias = torch.full((c.Cout,), float(data[1:]))
    if c.inplace and res is None:
        res = randn(8, (c.B, c.Cout, c.H, c.W), 0.5)
    with G.stats_sink(2 * c.B * c.H * c.W * c.Cout) as sink:                          # room for one-pixel blocks
        if c.entry in ("conv2d", "conv2d+s"):
            out = G.conv2d(x1, w, bias, x2, bias2, res, scale, splitk=c.entry == "conv2d+s", res_in_place=c.inplace)
        elif c.entry in ("f43", "w2d"):
            out = G.conv3x3_f43(x1, w, None, None, bias, x2, bias2, res, scale, form=c.entry)
        elif c.entry == "conv16":
            out = G.conv2d_16(x1, w, dt, bias, x2, bias2, res, scale)
        else:                                                                        # the folded shortcut: its bias instead of res / bias2
            out = G.resblock_tail_16(x1, w, dt, bias, xs, ws, randn(9, (c.Cout,), 0.5) if data == "b" else None, scale=scale)
    route = G.last_route()
    assert route == c.route or (c.route.endswith("<") and route.startswith(c.route)), f"ran {route}, not {c.route}"
    assert sink.blocks > 0, "the route writes no statistics"
    part = sink.partial(c.B, c.Cout)
    assert bool(torch.isfinite(part).all()), "partials the launch did not write"
    assert sink.clean_beyond(c.B, c.Cout), "the launch wrote past B * nblk * Cout pairs"
    return out.permute(0, 2, 3, 1).double().numpy(), part.double().numpy()


def measure(G, c, data, dt):
    """(fused, stand-alone) figures (e_mean, e_var, c_mean) of one case, printed"""
    o, part = launch(G, c, data, dt)
    HW, Gn = c.H * c.W, S.groups(c.Cout)
    mu_ref, var_ref = S.tensor_stats(o, Gn)
    fused = S.errors(*S.merge_partials([part], HW, Gn), mu_ref, var_ref)
    # the stand-alone kernel on the same stored values (16-bit: they round to themselves), same number of blocks
    alone_p = G.gn_stats(torch.from_numpy(o).float().permute(0, 3, 1, 2), part.shape[1], dt=dt).double().numpy()
    alone = S.errors(*S.merge_partials([alone_p], HW, Gn), mu_ref, var_ref)
    off = float((np.abs(mu_ref) / np.sqrt(var_ref)).max())
    print(f"\nSTATS {c.name:20s} {['f32', 'bf16', 'f16'][dt]:5s} {data:6s} nblk={part.shape[1]:4d} |mu|/sigma={off:9.3e}  "
          f"fused e_mean={fused[0]:.3e} e_var={fused[1]:.3e} c_mean={fused[2]:+.3e}  "
          f"alone e_mean={alone[0]:.3e} e_var={alone[1]:.3e} c_mean={alone[2]:+.3e}")
    return fused, alone


def check_producer(G, c, data, dt, st):
    fused, alone = measure(G, c, data, dt)
    c_m, c_v = C_M[st], C_V[st, "c" if data.startswith("c") else "ab"]
    assert alone[2] <= c_m and alone[1] <= c_v, ("stand-alone gn_stats", alone)
    assert fused[2] <= c_m and fused[1] <= c_v, fused
    return fused


@pytest.mark.parametrize("data", ["a", "b", "c50", "c1000"])
@pytest.mark.parametrize("c", CASES32, ids=lambda c: c.name)
def test_producer_fp32(G, c, data):
    check_producer(G, c, data, 0, "f32")


@pytest.mark.parametrize("data", ["a", "b", "c8"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("c", CASES16, ids=lambda c: c.name)
def test_producer_16(G, c, dt, data):
    fused = check_producer(G, c, data, DT[dt], "16")
    assert fused[0] <= CEIL16 and fused[1] <= CEIL16, fused


# ---------------------------------------------------------------------------------------------------------- finalize
def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def check_finalize(G, sets, HW, Gn, eps=1e-6):
    """flowse_op_gn_finalize of fp32 partial sets against the float64 merge of the same partials"""
    Cc = sum(p.shape[2] for p in sets)
    gamma = 1.0 + randn(31, (Cc,), 0.2)
    mean, scl = G.gn_finalize(sets[0], HW, Gn, gamma, sets[1] if len(sets) > 1 else None, eps)
    mu, var = S.merge_partials([p.double().numpy() for p in sets], HW, Gn)
    cpg = Cc // Gn
    mu_c, var_c = np.repeat(mu, cpg, axis=1), np.repeat(var, cpg, axis=1)
    scl_ref = gamma.double().numpy()[None] / np.sqrt(var_c + eps)
    d_mean = np.abs(mean.double().numpy() - mu_c) / ulp32(mu_c)
    d_scl = np.abs(scl.double().numpy() / scl_ref - 1.0)
    print(f"\nFINALIZE HW={HW} sets={[tuple(p.shape) for p in sets]} mean {d_mean.max():.3f} ulp, scale {d_scl.max():.3e}")
    assert d_mean.max() <= 1.0 and d_scl.max() <= 2.0 ** -22, (d_mean.max(), d_scl.max())


def synth_partials(seed, B, HW, nblk, Cc, offset=0.0):
    """fp32 partials of a random tensor (exact in float64, then rounded: finalize is handed arbitrary fp32 pairs)"""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((B, HW, Cc)) * (0.5 + rng.random(Cc)) + rng.standard_normal(Cc) + offset
    return torch.from_numpy(S.partials_of(o, nblk)).float()


# C = 128 over 32 groups: 4 channels per group, items per group = 4 nblk.  HW = 3 nblk - 1: a short last block everywhere.
@pytest.mark.parametrize("nblk", [8, 64, 65, 100, 128, 160, 192, 250, 256, 400, 512])
def test_finalize_items_per_group(G, nblk):
    """<= 256 items (8, 64: one request per thread), 257-512 (65, 100, 128: the two-item remainder), 513-768 (160, 192:
    three), 769-1024 (250, 256: one full round), 1600 (400: a round and two or three more), 2048 (512: two rounds)"""
    check_finalize(G, [synth_partials(nblk, 2, 3 * nblk - 1, nblk, 128, 3.0)], 3 * nblk - 1, 32)


def test_finalize_short_last_block(G):
    check_finalize(G, [synth_partials(41, 2, 257, 2, 64)], 257, 16)            # blocks of 129 and 128 pixels


def test_finalize_large_mean(G):
    p = synth_partials(42, 2, 1024, 8, 64, offset=1000.0)
    check_finalize(G, [p], 1024, 16)


@pytest.mark.parametrize("HW,nblk1,nblk2", [(256, 16, 1), (1024, 128, 4), (257, 2, 5)])
def test_finalize_two_sets_straddle(G, HW, nblk1, nblk2):
    """C = 256 + 128 over 32 groups of 12 channels: group 21 takes 4 channels from set 1 and 8 from set 2"""
    check_finalize(G, [synth_partials(43, 2, HW, nblk1, 256, 2.0), synth_partials(44, 2, HW, nblk2, 128, -1.0)], HW, 32)


def test_finalize_real_launch_and_gn_stats(G):
    """set 1: what the small-image kernel left for its 256 output channels (16-pixel blocks); set 2: flowse_op_gn_stats of a
    128-channel skip tensor (one block): the concat GroupNorm of the up path (ncsnpp.py:337), group 21 straddling"""
    c = CASES32[5]
    assert c.name == "smallm-16px"
    o, part = launch(G, c, "b", 0)
    skip = randn(45, (c.B, 128, c.H, c.W)) * 3.0 - 0.5
    p2 = G.gn_stats(skip, 1)
    sets = [torch.from_numpy(part).float(), p2]
    assert sets[0].shape[1] == 16 and sets[1].shape[1] == 1
    check_finalize(G, sets, c.H * c.W, 32)
    # and the whole chain against the two stored tensors themselves
    both = np.concatenate([o, skip.permute(0, 2, 3, 1).double().numpy()], axis=3)
    e = S.errors(*S.merge_partials([p.double().numpy() for p in sets], c.H * c.W, 32), *S.tensor_stats(both, 32))
    assert e[2] <= C_M["f32"] and e[1] <= C_V["f32", "ab"], e


@pytest.mark.parametrize("shape", ["quads", "straddle"])
def test_finalize_apply(G, shape):
    """the one-launch finalize + apply: groups of whole channel quads in one tensor (the 16-byte path), and 256 + 128 channels
    whose 12-channel groups take the element path (group 21 from both tensors) on 256 pixels, two pixel slices per group"""
    B, H, W, c1, c2 = (2, 8, 8, 64, 0) if shape == "quads" else (1, 16, 16, 256, 128)
    x1 = randn(51, (B, c1, H, W)) * 2.0 + 0.7
    x2 = randn(52, (B, c2, H, W)) * 3.0 - 0.5 if c2 else None
    Cc = c1 + c2
    g, b = 1.0 + randn(53, (Cc,), 0.2), randn(54, (Cc,), 0.2)
    p1 = G.gn_stats(x1, 4)
    p2 = G.gn_stats(x2, 1) if c2 else None
    xin = torch.cat([x1, x2], 1) if c2 else x1
    for silu in (False, True):
        got = G.gn_finalize(p1, H * W, S.groups(Cc), g, p2, x1=x1, x2=x2, beta=b, silu=silu)
        ref = F.group_norm(xin.double(), S.groups(Cc), g.double(), b.double(), eps=1e-6)
        ref = (F.silu(ref) if silu else ref).float()
        assert C.rel_l2(got, ref) < 2e-5


@pytest.mark.parametrize("offset", [50.0, 1000.0])
def test_group_norm_large_mean_fused(G, offset):
    """test_group_norm_large_mean's chain with the statistics the FIRST conv's output stage leaves (there: the stand-alone
    kernel recomputes them): y = conv_b(GN(conv_a(x0))), conv_a producing a large-mean tensor under the sink, its partials
    merged and applied by flowse_op_gn_finalize.  (No fp32 per-op entry normalises on load with outside mean / scale: the
    finalize + apply kernel normalises, the plain conv follows.)  Same float64 reference and bound."""
    x0 = randn(20, (2, 32, 128, 128))
    wa = randn(21, (128, 32, 3, 3), (1.0 / (32 * 9)) ** 0.5)
    ba = torch.full((128,), float(offset))
    wb = randn(22, (128, 128, 3, 3), (1.0 / (128 * 9)) ** 0.5)
    g2 = 1.0 + randn(23, (128,), 0.2)
    b2 = randn(24, (128,), 0.2)
    with G.stats_sink(2 * 128 * 128 * 128 * 2) as sink:
        mid = G.conv2d(x0, wa, ba)
    assert G.last_route() == "halo" and sink.blocks == 128 * 128 // 128
    normed = G.gn_finalize(sink.partial(2, 128), 128 * 128, 32, g2, x1=mid, beta=b2, silu=False)
    got = G.conv2d(normed, wb)
    ref_mid = F.conv2d(x0, wa, ba, padding=1)
    ref = F.conv2d(F.group_norm(ref_mid.double(), 32, g2.double(), b2.double(), eps=1e-6).float(), wb, None, padding=1)
    assert C.rel_l2(got, ref) < 5e-5
