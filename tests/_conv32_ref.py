"""Rows, float64 reference and bounds for the large-image fp32 convolution kernels: conv3x3_halo_kernel ("halo"),
conv3x3_head4_kernel ("head4"), conv3x3_f43_kernel whole K and sliced ("f43", "f43_splitk"), conv_mfma_kernel /
conv_mfma_fast_kernel ("flat", "flat_splitk") with the two plain reduction kernels of conv_reduce.hip,
conv1x1_stream_kernel ("1x1_stream") and the kernels of a 4-channel input ("cin4", "cin4_stats", "cin4_mfma").

Shared by tests/test_conv32_bounds_host.py (CPU: every row's route and form, an fp32 restatement of every row meets the
bounds, restated defects miss them) and tests/test_gpu_conv32.py (the kernels themselves).  Nothing here touches the
library.  Out of scope: "w2d" (tests/test_gpu_w2d_epilogue.py), "halo_bf16x3" and splitk_reduce_gn_kernel (reachable only
through a model handle), "smallm" (tests/_smallm_ref.py).

Reference: the kernel's expression in float64 on the fp32 operands, `scale` the float32 value.  Rows with fused
GroupNorm (+ SiLU) take (mean, scale) per (sample, channel) AS DATA -- on the GPU the pair the entry's prologue left in
the caller's scratch, on the CPU the float64 statistics rounded to fp32 -- and stage
    y = (x - m) s + beta,   a64 = y sigmoid(y)  (GroupNorm only: a64 = y),   0 outside the image (AFTER the activation).
stats_guard() holds the pair to the float64 statistics of the input to 1e-4: their accuracy is other tests' subject.

Bounds, eps = 2^-23, every operation charged a full ulp of a partial result (as _smallm_ref.py and _conv16_ref.py):
    direct kernels   |got - ref| <= (K + ks + 16) eps S + gn      K = taps Cin, ks = K slices (0: whole K),
                     S = (conv(|a64|, |w|) + |bias| + |bias2| + |res|) |scale|,   gn = conv(tau, |w|) |scale|
    F(4,3) kernels   |got - ref| <= (3 Cin + ks + 32) eps S_w + gn_w
                     S_w = (Wabs(a64, w) + |bias| + |bias2| + |res|) |scale|,  gn_w = Wabs(tau, w) |scale|
                     Wabs = the pipeline v = B^T d, u = G g, out = A^T (sum of 3 Cin products v u) of the header of
                     conv_f43.hip with |B^T|, |G|, |A^T| applied to |d|, |w| in float64 (4-row quads aligned to the image)
    tau              GroupNorm only 2 eps P, GroupNorm + SiLU 4 eps (P + |a64|), P = |x s| + |m s| + |beta|: the
                     derivation of _conv16_ref.py for y = fma(x - m, s, b), a = y rcp(1 + exp2(-L y)), which is what gn_quad
                     (conv_common.h) and the head kernel evaluate
Second check, every row: rel-L2 < 2e-5.  Probe rows (one-hot weights, no epilogue terms): bit-exact / exactly 0 outside the
image without GN, within tau of a64 with it.  Rows above 8M output elements ("sparse") have four non-zero (tap, ci) weights
per output channel: reference, S_w and gn_w are gathers.  Nothing here is fitted to a device's output.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

SCALE = 0.70710678
EPS = 2.0 ** -23
REL_L2 = 2e-5
GN_EPS = 1e-6
ROUTES = ("halo", "head4", "f43", "f43_splitk", "flat", "flat_splitk", "1x1_stream", "cin4", "cin4_stats", "cin4_mfma")
WINO_ROUTES = ("f43", "f43_splitk")
# GN modes a route's entry can reach (0 plain, 1 GroupNorm, 2 GroupNorm + SiLU)
GN_MODES = {r: ((0, 1, 2) if r in ("halo", "head4", "f43", "f43_splitk") else (0,)) for r in ROUTES}
TILE = {"halo": (8, 16), "head4": (16, 16), "f43": (8, 16), "f43_splitk": (8, 16)}
GN_TAG = {0: "plain", 1: "gn", 2: "gnsilu"}
# FLOWSE_OFFER_* of include/flowse_hip.h
WINO, WINO2, WSM, WFRAG, WQ, WQ3, WQF16, SLAB, GN, BIAS2, STATS, FOLD = (1 << i for i in range(12))
ENTRY_BITS = {"c": 0, "cs": WSM | SLAB, "g": GN, "f": WINO | SLAB}

# entry: "c" flowse_op_conv2d, "cs" the same with scratch, "g" flowse_op_conv3x3_gn, "f" flowse_op_conv3x3_f43; sink: inside
# the statistics sink; kind: "conv", "probe" (one-hot weights), "sparse" (four weights per output channel); ks: slices
# (0 = whole K); form: the claims about the launch, restated by form_of(); inplace: the residual sits in the output buffer
Row = namedtuple("Row", "name route entry sink B H W C1 C2 Cout k gn bias bias2 res scale kind ks form inplace")


def _r(name, route, entry, geom, C1, Cout, *, C2=0, k=3, gn=0, bias=True, bias2=True, res=True, scale=SCALE, kind="conv",
       ks=0, sink=False, inplace=False, **form):
    B, H, W = geom
    if route == "head4":
        bias2 = False                                    # the dispatch's condition
    if kind == "probe":
        bias = bias2 = res = False
        scale = 1.0
    return Row(name, route, entry, sink, B, H, W, C1, C2, Cout, k, gn, bias, bias2, res, scale, kind, ks,
               tuple(sorted(form.items())), inplace)


EPI = (("nobias", dict(bias=False)), ("nobias2", dict(bias2=False)), ("nores", dict(res=False)), ("scale1", dict(scale=1.0)))


def _build():
    rows = []
    add = lambda *a, **k: rows.append(_r(*a, **k))
    # ------------------------------------------------------------------------------------------- halo (8 x 16 tiles)
    for gn in (0, 1, 2):
        add(f"halo-bn32-{GN_TAG[gn]}", "halo", "g" if gn else "c", (2, 128, 128), 32, 32, gn=gn, bn=32, border="interior")
    add("halo-bn32-live4", "halo", "c", (64, 16, 16), 32, 4, bn=32, live=4, border="strip_lr")
    add("halo-bn64-partial", "halo", "c", (2, 128, 128), 32, 40, bn=64, live=40)
    add("halo-bn128-last32", "halo", "c", (2, 128, 128), 32, 160, bn=128, ntiles=2, live=32)
    add("halo-bn128-full", "halo", "c", (2, 128, 128), 32, 256, bn=128, ntiles=2, live=128)
    add("halo-bn64-2n", "halo", "c", (1, 24, 96), 128, 128, bn=64, ntiles=2)
    for gn in (0, 1, 2):
        add(f"halo-3x6-{GN_TAG[gn]}", "halo", "g" if gn else "c", (1, 24, 96), 128, 64, gn=gn, bn=64, border="interior")
    add("halo-cat-64+64", "halo", "g", (1, 24, 96), 64, 64, C2=64, gn=2, bn=64)
    add("halo-cat-96+32", "halo", "g", (1, 24, 96), 96, 64, C2=32, gn=2, bn=64)
    add("halo-row", "halo", "c", (3, 8, 112), 128, 64, bn=64, border="strip_tb")
    add("halo-col", "halo", "c", (1, 152, 16), 128, 64, bn=64, border="strip_lr")
    add("halo-all4", "halo", "c", (17, 8, 16), 128, 64, bn=64, border="all4")
    for tag, kw in EPI:
        add(f"halo-epi-{tag}", "halo", "c", (1, 24, 96), 128, 64, bn=64, **kw)
    for gn in (0, 1, 2):
        add(f"halo-probe-{GN_TAG[gn]}", "halo", "g" if gn else "c", (2, 128, 128), 32, 288, gn=gn, kind="probe", bn=128)
    # ------------------------------------------------------- head4 (16 x 16 tiles, >= 64 of them, no per-sample bias)
    for gn in (0, 1, 2):
        add(f"head4-all4-{GN_TAG[gn]}", "head4", "g" if gn else "c", (64, 16, 16), 32, 4, gn=gn, border="all4")
    add("head4-1x128x128", "head4", "c", (1, 128, 128), 32, 4, border="interior")
    for cin in (64, 96, 128):
        add(f"head4-4x64x64-{cin}", "head4", "c", (4, 64, 64), cin, 4, border="interior")
    add("head4-nores", "head4", "c", (4, 64, 64), 32, 4, res=False)
    add("head4-nobias", "head4", "g", (4, 64, 64), 32, 4, gn=1, bias=False)
    # ------------------------------------------------------------------------------------------------- f43, whole K
    add("f43-all4", "f43", "f", (32, 8, 16), 32, 512, gn=2, wide=False, tpb=1, border="all4")
    for gn in (0, 1, 2):
        add(f"f43-strip-{GN_TAG[gn]}", "f43", "f", (1, 128, 128), 32, 128, gn=gn, wide=False, tpb=1, walk="strip")
    add("f43-rowmajor", "f43", "f", (2, 72, 48), 32, 320, gn=2, wide=False, tpb=1, walk="row")
    add("f43-wide-odd", "f43", "f", (2, 128, 128), 32, 256, gn=2, wide=True, tpb=1, chunks=1)
    add("f43-wide-8x64x128", "f43", "f", (8, 64, 128), 32, 128, gn=2, wide=True, tpb=1)
    add("f43-wide-cat-32+32", "f43", "f", (2, 128, 128), 32, 256, C2=32, gn=2, wide=True, tpb=1, chunks=2)
    add("f43-wide-cat-64+32", "f43", "f", (2, 128, 128), 64, 256, C2=32, gn=2, wide=True, tpb=1, chunks=3)
    for tag, geom, tpb, walk in (("tpb2", (8, 128, 128), 2, "strip"), ("tpb4", (16, 128, 128), 4, "strip"),
                                 ("tpb2row", (43, 64, 48), 2, "row")):
        f = dict(kind="sparse", wide=True, tpb=tpb, walk=walk)
        add(f"f43-{tag}-plain", "f43", "f", geom, 64, 256, gn=0, **f)
        add(f"f43-{tag}-gnsilu", "f43", "f", geom, 64, 256, gn=2, **f)
        add(f"f43-{tag}-cat-gn", "f43", "f", geom, 32, 256, C2=32, gn=1, **f)
    for tag, kw in EPI:
        add(f"f43-wide-epi-{tag}", "f43", "f", (2, 128, 128), 32, 256, gn=0, wide=True, tpb=1, **kw)
    # --------------------------------------------------------------------------------- f43_splitk + the reduction
    for tag, geom, cin, ks, slices in (("ks2-4", (1, 24, 96), 128, 2, (2, 2)), ("ks2-5", (2, 24, 48), 160, 2, (3, 2)),
                                       ("ks3-7", (1, 40, 64), 224, 3, (3, 3, 1))):
        for gn in (0, 1, 2):
            add(f"f43sk-{tag}-{GN_TAG[gn]}", "f43_splitk", "f", geom, cin, 64, gn=gn, ks=ks, slices=slices)
        add(f"f43sk-{tag}-sink", "f43_splitk", "f", geom, cin, 64, gn=2, ks=ks, slices=slices, sink=True, stats=True)
    add("f43sk-cat-64+64", "f43_splitk", "f", (1, 24, 96), 64, 64, C2=64, gn=2, ks=2, slices=(2, 2))
    # ------------------------------------------------------------------------------------------------ flat, whole K
    for k in (3, 1):
        add(f"flat-46x46-k{k}", "flat", "c", (1, 46, 46), 32, 128, k=k, tiling="2222", fast=True, ragged=True)
    add("flat-generic-bn32", "flat", "c", (1, 47, 47), 36, 20, tiling="4111", fast=False, ragged=True)
    add("flat-generic-bn64", "flat", "c", (1, 47, 47), 36, 60, k=1, tiling="2221", fast=False, ragged=True)
    add("flat-smallm-generic", "flat", "c", (3, 5, 4), 36, 128, tiling="1411", fast=False, ragged=True)
    add("flat-smallm-fast", "flat", "c", (1, 8, 8), 256, 128, tiling="1411", fast=True)
    add("flat-h1", "flat", "c", (1, 1, 60), 36, 128, tiling="1411", fast=False)
    add("flat-cout132", "flat", "cs", (1, 47, 47), 128, 132, k=1, tiling="2222", fast=True, ragged=True)
    add("flat-probe", "flat", "c", (1, 46, 46), 32, 288, kind="probe", tiling="2222", fast=True)
    # ------------------------------------------------------------------------------- flat_splitk + the reduction
    sk = lambda name, geom, c1, cout, ks, **kw: add(name, "flat_splitk", "cs", geom, c1, cout, ks=ks, **kw)
    sk("flatsk-ks2", (1, 46, 46), 32, 128, 2, fast=True, slices=(5, 4))
    sk("flatsk-ks9", (1, 46, 46), 128, 128, 9, fast=True, slices=(4,) * 9)
    sk("flatsk-generic", (1, 46, 46), 36, 128, 4, fast=False, slices=(5, 5, 5, 3))
    sk("flatsk-cat-48+16", (1, 46, 46), 48, 128, 4, C2=16, fast=False, slices=(5, 5, 5, 3))
    sk("flatsk-1x1", (1, 50, 50), 256, 128, 2, k=1, fast=True, slices=(4, 4))
    sk("flatsk-bn32", (1, 47, 47), 64, 32, 4, tiling="4111", slices=(5, 5, 5, 3))
    sk("flatsk-bn64", (1, 47, 47), 64, 64, 4, tiling="2221", slices=(5, 5, 5, 3))
    sk("flatsk-1x1-cat", (2, 32, 64), 256, 128, 3, C2=128, k=1, slices=(4, 4, 4))
    sk("flatsk-64x64", (1, 64, 64), 256, 256, 4, slices=(18,) * 4)
    sk("flatsk-1x1-cat-sink", (2, 32, 64), 256, 128, 3, C2=128, k=1, sink=True, stats=True)
    sk("flatsk-64x64-sink", (1, 64, 64), 256, 256, 4, sink=True, stats=True)
    # ----------------------------------------------------------------------------------------------- 1x1_stream
    st = lambda name, geom, c1, cout, **kw: add(name, "1x1_stream", "cs", geom, c1, cout, k=1, **kw)
    st("stream-ring4", (256, 16, 16), 32, 128, kblocks=4, nblocks=1)
    st("stream-12kb", (128, 16, 16), 96, 256, kblocks=12, nblocks=2)
    st("stream-cat-32+32", (128, 16, 16), 32, 256, C2=32, kblocks=8, nblocks=2)
    st("stream-2x128x128", (2, 128, 128), 32, 256, kblocks=4, nblocks=2)
    for tag, kw in EPI:
        st(f"stream-epi-{tag}", (256, 16, 16), 32, 128, kblocks=4, **kw)
    st("stream-probe", (256, 16, 16), 128, 128, kind="probe", kblocks=16)
    st("stream-sink", (2, 128, 128), 32, 256, sink=True, stats=True)
    # ---------------------------------------------------------------------------------------------- cin4 family
    add("cin4-2x2", "cin4", "c", (1, 2, 2), 4, 16, Q=4, ppb=64, ragged=True)
    add("cin4-5x7-k3", "cin4", "c", (3, 5, 7), 4, 128, Q=32, ppb=8, ragged=True)
    add("cin4-5x7-k1", "cin4", "c", (3, 5, 7), 4, 256, k=1, Q=64, ppb=4, ragged=True)
    c4s = lambda name, geom, cout, **kw: add(name, "cin4_stats", "c", geom, 4, cout, k=1, sink=True, stats=True, **kw)
    c4s("cin4stats-1of4", (2, 16, 8), 8, Q=2, rounds=1, last=1)
    c4s("cin4stats-2of4", (2, 16, 8), 16, Q=4, rounds=1, last=2)
    c4s("cin4stats-2of4-8x8", (2, 8, 8), 32, Q=8, rounds=1, last=2)
    c4s("cin4stats-3of4", (2, 8, 12), 32, Q=8, rounds=1, last=3)
    c4s("cin4stats-4rounds", (2, 16, 8), 128, Q=32, rounds=4, last=4)
    c4s("cin4stats-q256", (2, 16, 16), 1024, Q=256, rounds=32, last=4)
    c4s("cin4stats-inplace", (2, 16, 8), 128, Q=32, inplace=True)
    add("cin4mfma-all4", "cin4_mfma", "c", (256, 8, 16), 4, 128, border="all4")
    add("cin4mfma-2x128x128", "cin4_mfma", "c", (2, 128, 128), 4, 128)
    add("cin4mfma-1x256x128", "cin4_mfma", "c", (1, 256, 128), 4, 128)
    names = [r.name for r in rows]
    assert len(set(names)) == len(names)
    return rows


ROWS = _build()
BY_NAME = {r.name: r for r in ROWS}
CONV_ROWS = [r for r in ROWS if r.kind != "probe"]
PROBE_ROWS = [r for r in ROWS if r.kind == "probe"]
REPRO = ("f43-tpb2-plain", "f43sk-ks3-7-gnsilu", "flatsk-ks9", "stream-12kb", "cin4stats-4rounds")
BIG = 8 << 20                                            # output elements above which a row has sparse weights


def offer_bits(r):
    """the offer the row's entry makes to conv_route (the issue's table of entries)"""
    bits = ENTRY_BITS[r.entry] | (BIAS2 if r.bias2 else 0) | (STATS if r.sink else 0)
    if r.entry == "f" and r.gn:
        bits |= GN
    return bits


# ----------------------------------------------------------------------------- the launchers' arithmetic, restated
def border_of(H, W, th, tw):
    ty, tx = H // th, W // tw
    if ty == 1 and tx == 1:
        return "all4"
    if tx == 1:
        return "strip_lr"
    if ty == 1:
        return "strip_tb"
    return "edges" if ty == 2 or tx == 2 else "interior"


def _flat_tiling(M, Cout):
    """(WM, WN, TM, TN) of launch_flat_fp32"""
    if Cout <= 32:
        return (4, 1, 1, 1)
    if Cout <= 64:
        return (2, 2, 2, 1)
    return (1, 4, 1, 1) if M <= 64 and Cout > 64 else (2, 2, 2, 2)


def _slices(steps, ks):
    per = -(-steps // ks)
    return tuple(min(steps, (i + 1) * per) - i * per for i in range(ks))


def form_of(r):
    """what the launcher of the row's route does with its shape: {claim: value}"""
    M, Cin, HW = r.B * r.H * r.W, r.C1 + r.C2, r.H * r.W
    f = {}
    if r.route == "halo":                                   # launch_halo_fp32
        tiles128 = (M // 128) * -(-r.Cout // 128)
        bn = 32 if r.Cout <= 32 else 64 if r.Cout <= 64 or tiles128 < 512 else 128
        nt = -(-r.Cout // bn)
        f = dict(bn=bn, ntiles=nt, live=r.Cout - (nt - 1) * bn, border=border_of(r.H, r.W, 8, 16))
    elif r.route == "head4":
        f = dict(border=border_of(r.H, r.W, 16, 16))
    elif r.route in WINO_ROUTES:                            # launch_f43, conv3x3_f43_body's make_tile and slices
        chunks = Cin // 32
        wide = r.ks == 0 and r.Cout % 128 == 0 and (M // 128) * (r.Cout // 128) >= 512
        tpb = 1
        if wide and chunks % 2 == 0:
            blocks1 = (M // 128) * (r.Cout // 128)
            for t in (4, 2):
                if (HW // 128) % t == 0 and blocks1 // t >= 1024:
                    tpb = t
                    break
        f = dict(wide=wide, tpb=tpb, chunks=chunks, walk="strip" if (r.W // 16) % 4 == 0 else "row",
                 border=border_of(r.H, r.W, 8, 16))
        if r.ks:
            f["slices"] = _slices(chunks, r.ks)
    elif r.route in ("flat", "flat_splitk"):                # launch_flat_fp32 / launch_cfg, the kernels' step ranges
        t = _flat_tiling(M, r.Cout)
        bm = t[0] * t[2] * 32
        f = dict(tiling="%d%d%d%d" % t, fast=r.C1 % 32 == 0 and r.C2 % 32 == 0, ragged=M % bm != 0)
        if r.ks:
            f["slices"] = _slices(-(-Cin // 32) * r.k * r.k, r.ks)
    elif r.route == "1x1_stream":                           # 256 pixels x 128 channels per block, k-blocks of 8 channels
        f = dict(kblocks=Cin // 8, nblocks=r.Cout // 128)
    elif r.route in ("cin4", "cin4_stats"):                 # launch_cin4, conv_cin4_stats_kernel's rounds
        Q = r.Cout // 4
        f = dict(Q=Q, ppb=256 // Q, ragged=M % (256 // Q) != 0)
        if r.route == "cin4_stats":
            PB, R = min(HW, 128), 256 // Q
            n = PB // R                                      # pixels per thread, walked four per round
            f.update(rounds=-(-n // 4), last=n - 4 * (-(-n // 4) - 1))
    elif r.route == "cin4_mfma":                            # 128 flat pixels per block
        f = dict(border="all4" if HW == 128 else "flat")
    return f


# ------------------------------------------------------------------------------------------------------------ inputs
Inputs = namedtuple("Inputs", "x w bias bias2 res gamma beta sparse")
_inputs = {}


def inputs(r):
    """fp32 tensors of a row (NCHW; bias2 [B, Cout + 4]: a row stride that is not Cout), seeded by shape -- rows that differ
    only in the epilogue terms or the GN mode share them.  sparse: (tap, ci, value) [Cout, 4] each, or None."""
    key = (r.B, r.H, r.W, r.C1, r.C2, r.Cout, r.k, r.kind)
    if key not in _inputs:
        seed = 0
        for v in key[:-1] + (len(r.kind),):
            seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
        g = torch.Generator().manual_seed(seed)
        cin, taps = r.C1 + r.C2, r.k * r.k
        x = 1.5 * torch.randn(r.B, cin, r.H, r.W, generator=g) + 0.3
        sparse = None
        if r.kind == "probe":
            assert r.Cout == taps * cin
            w = torch.zeros(r.Cout, cin, r.k, r.k)
            ch = torch.arange(cin)
            for t in range(taps):
                w[cin * t + ch, ch, t // r.k, t % r.k] = 1.0
        elif r.kind == "sparse":
            flat = torch.stack([torch.randperm(taps * cin, generator=g)[:4] for _ in range(r.Cout)])
            val = 0.5 * torch.randn(r.Cout, 4, generator=g)
            sparse = (flat // cin, flat % cin, val)
            w = torch.zeros(r.Cout, cin, r.k, r.k)
            co = torch.arange(r.Cout)[:, None].expand(-1, 4)
            w[co, sparse[1], sparse[0] // r.k, sparse[0] % r.k] = val
        else:
            w = torch.randn(r.Cout, cin, r.k, r.k, generator=g) / (cin * taps) ** 0.5
        bias = 0.1 * torch.randn(r.Cout, generator=g)
        bias2 = 0.1 * torch.randn(r.B, r.Cout + 4, generator=g)
        res = torch.randn(r.B, r.Cout, r.H, r.W, generator=g)
        gamma = 1 + 0.2 * torch.randn(cin, generator=g)
        beta = 0.2 * torch.randn(cin, generator=g)
        _inputs[key] = Inputs(x, w, bias, bias2, res, gamma, beta, sparse)
        if len(_inputs) > 2:
            _inputs.pop(next(iter(_inputs)))
    i = _inputs[key]
    return i._replace(bias=i.bias if r.bias else None, bias2=i.bias2 if r.bias2 else None, res=i.res if r.res else None)


# ------------------------------------------------------------------------------------- GroupNorm statistics as data
def gn_stats64(r):
    """(mean, scale = gamma rstd, sigma) [B, C] in float64: GroupNorm over cat[x1, x2] with min(C / 4, 32) groups"""
    i = inputs(r)
    B, C = r.B, r.C1 + r.C2
    G = min(C // 4, 32)
    xg = i.x.double().reshape(B, G, -1)
    m = xg.mean(2)
    var = xg.var(2, unbiased=False)
    rep = C // G
    mean = m.repeat_interleave(rep, 1)
    sig = var.sqrt().repeat_interleave(rep, 1)
    scl = i.gamma.double()[None] / (var + GN_EPS).sqrt().repeat_interleave(rep, 1)
    return mean, scl, sig


def gn_data(r, stats=None):
    """the (mean, scale) [B, C] fp32 pair the row is staged with: `stats` (from the device) or float64's, rounded"""
    if not r.gn:
        return None
    if stats is not None:
        return stats[0].float().reshape(r.B, -1), stats[1].float().reshape(r.B, -1)
    m, s, _ = gn_stats64(r)
    return m.float(), s.float()


def stats_guard(r, stats):
    """the staged pair agrees with the float64 statistics to 1e-4 -- of |mean| + sigma for the mean (its natural scale: a
    group's mean may be near 0), of the scale itself for the scale.  Returns a list of complaints."""
    m64, s64, sig = gn_stats64(r)
    m, s = gn_data(r, stats)
    fails = []
    em = float(((m.double() - m64).abs() / (m64.abs() + sig)).max())
    es = float(((s.double() - s64).abs() / s64.abs()).max())
    if not em <= 1e-4:
        fails.append(f"staged mean off the float64 statistics by {em:.2e}")
    if not es <= 1e-4:
        fails.append(f"staged scale off the float64 statistics by {es:.2e}")
    return fails


def staged(r, gnd):
    """(a64, tau): the conv's operand as the kernel stages it, in float64, and the allowance of its fp32 evaluation"""
    i = inputs(r)
    x = i.x.double()
    if not r.gn:
        return x, None
    m, s = gnd[0].double()[:, :, None, None], gnd[1].double()[:, :, None, None]
    b = i.beta.double()[None, :, None, None]
    y = (x - m) * s + b
    P = (x * s).abs() + (m * s).abs() + b.abs()
    if r.gn == 2:
        a64 = y * torch.sigmoid(y)
        return a64, 4 * EPS * (P + a64.abs())
    return y, 2 * EPS * P


def stage_fp32(r, gnd, x):
    """the staging in torch fp32 as gn_quad writes it: y = (x - m) s + b (unfused), a = y rcp(1 + exp2(-L y))"""
    if not r.gn:
        return x
    i = inputs(r)
    m, s, b = gnd[0][:, :, None, None], gnd[1][:, :, None, None], i.beta[None, :, None, None]
    y = (x - m) * s + b
    if r.gn == 2:
        L = torch.tensor(-1.44269504088896341, dtype=torch.float32)
        y = y * torch.reciprocal(1 + torch.exp2(y * L))
    return y


# ------------------------------------------------------------------------------------------- the F(4,3) pipeline
BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                   [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
GM = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                   [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)


def _mats(dtype, absolute):
    ms = (BT, GM, AT)
    return tuple((m.abs() if absolute else m).to(dtype) for m in ms)


def wino_v(a, absolute=False):
    """v = B^T d of every 4-row quad: [6, B, C, H / 4, W] from a [B, C, H, W] (0 above and below the image)"""
    Bt = _mats(a.dtype, absolute)[0]
    H = a.shape[2]
    assert H % 4 == 0
    ap = F.pad(a, (0, 0, 1, 1))
    d = torch.stack([ap[:, :, i:i + H - 3:4] for i in range(6)])
    return (Bt @ d.reshape(6, -1)).reshape(d.shape)


def _rows_back(o):
    """[4, B, C, H / 4, W] output rows of the quads -> [B, C, H, W]"""
    _, B, C, Hq, W = o.shape
    return o.permute(1, 2, 3, 0, 4).reshape(B, C, 4 * Hq, W)


def wino(a, w, absolute=False):
    """The pipeline of conv_f43.hip's header in a's type: v = B^T d over six input rows, u = G g, m = sum over (kx, ci) of
    v u, out = A^T m over four output rows.  absolute: |B^T|, |G|, |A^T| (the caller passes |a|, |w|) = Wabs."""
    _, Gm, At = _mats(a.dtype, absolute)
    v = wino_v(a, absolute)
    u = torch.einsum("ck,oikx->coix", Gm, w)                 # [6, Cout, Cin, 3]
    m = torch.stack([F.conv2d(v[c], u[c][:, :, None, :], padding=(0, 1)) for c in range(6)])
    return _rows_back((At @ m.reshape(6, -1)).reshape((4,) + m.shape[1:]))


def _gather(src3, sparse, W, absolute):
    """sum over a row's four weights of value * src3[ky][:, ci, :, kx : kx + W]; src3: per ky a [B, C, H, W + 2] tensor"""
    tap, ci, val = sparse
    B, _, H, _ = src3[0].shape
    out = torch.zeros(B, tap.shape[0], H, W, dtype=src3[0].dtype)
    for co in range(tap.shape[0]):
        for j in range(4):
            ky, kx = divmod(int(tap[co, j]), 3)
            v = float(val[co, j])
            out[:, co].add_(src3[ky][:, int(ci[co, j]), :, kx:kx + W], alpha=abs(v) if absolute else v)
    return out


def sparse_direct(a, sparse):
    """the 3x3 convolution of a [B, C, H, W] with a row's sparse weights, as gathers"""
    H, W = a.shape[2:]
    ap = F.pad(a, (1, 1, 1, 1))
    return _gather([ap[:, :, ky:ky + H] for ky in range(3)], sparse, W, False)


def sparse_wino(a, sparse, absolute=False):
    """wino() for sparse weights: out rows k of a weight at vertical tap ky = sum_c A^T[k, c] G[c, ky] v_c (the horizontal
    tap is a shift), gathered per weight"""
    _, Gm, At = _mats(a.dtype, absolute)
    v = wino_v(a, absolute)
    W = a.shape[3]
    src3 = []
    for ky in range(3):
        coef = At * Gm[:, ky][None, :]                        # [4, 6]
        src3.append(F.pad(_rows_back((coef @ v.reshape(6, -1)).reshape((4,) + v.shape[1:])), (1, 1)))
    return _gather(src3, sparse, W, absolute)


# -------------------------------------------------------------------------------------------------------- reference
Ref = namedtuple("Ref", "ref bound a64 tau")


def k_of(r):
    return r.k * r.k * (r.C1 + r.C2)


def reference(r, stats=None):
    """Ref(ref, bound, a64, tau) of a conv or sparse row: the float64 result and the per-element bound"""
    i = inputs(r)
    a64, tau = staged(r, gn_data(r, stats))
    w = i.w.double()
    pad = r.k // 2
    wino_row = r.route in WINO_ROUTES
    if r.kind == "sparse":
        ref = sparse_direct(a64, i.sparse)
        mag = sparse_wino(a64.abs(), i.sparse, True)
        gn = sparse_wino(tau, i.sparse, True) if r.gn else 0.0
    else:
        ref = F.conv2d(a64, w, padding=pad)
        if wino_row:
            mag = wino(a64.abs(), w.abs(), True)
            gn = wino(tau, w.abs(), True) if r.gn else 0.0
        else:
            mags = F.conv2d(torch.cat([a64.abs()] + ([tau] if r.gn else []), 0), w.abs(), padding=pad)
            mag = mags[:r.B].clone()
            gn = mags[r.B:].clone() if r.gn else 0.0
    for t in (i.bias[None, :, None, None] if r.bias else None, i.bias2[:, :r.Cout, None, None] if r.bias2 else None,
              i.res if r.res else None):
        if t is not None:
            ref += t.double()
            mag += t.double().abs()
    s = float(torch.tensor(r.scale, dtype=torch.float32))
    ops = (3 * (r.C1 + r.C2) + r.ks + 32) if wino_row else (k_of(r) + r.ks + 16)
    return Ref(ref * s, ops * EPS * mag * abs(s) + gn * abs(s), a64, tau)


DEFECTS = ("pad_before_act", "drop_last_chunk", "second_from_first", "tile_shift", "swap_quads", "bias2_sample0", "slice_twice",
           "bf16_operand")


def restate_fp32(r, defect=None):
    """The row's arithmetic restated in torch fp32 on the CPU (another summation order, the same operations): direct rows an
    fp32 conv, F(4,3) rows the transform pipeline, GN rows the gn_quad form.  Defects (restated, not kernels):
      pad_before_act      the zero padding is applied before the activation (border pixels become act(beta - m s))
      drop_last_chunk     the last 32-channel chunk of the first K slice (whole K: of the sum) is missing in ONE tile's first
                          32 output channels
      second_from_first   the second source's first chunk is read from the first source
      tile_shift          one tile's output is shifted by a pixel
      swap_quads          two channel quads of one tile are swapped
      bias2_sample0       sample 0's per-sample bias row serves every sample
      slice_twice         the first K slice is summed twice
      bf16_operand        the input is rounded to bf16"""
    i = inputs(r)
    gnd = gn_data(r)
    pad = r.k // 2
    cin = r.C1 + r.C2
    x, w = i.x, i.w
    if defect == "bf16_operand":
        x = x.bfloat16().float()
    if defect == "second_from_first":
        assert r.C2
        x = x.clone()
        n = min(32, r.C2)
        x[:, r.C1:r.C1 + n] = x[:, :n]

    def conv(a, w):
        if r.route in WINO_ROUTES:
            return sparse_wino(a, i.sparse) if r.kind == "sparse" else wino(a, w)
        return F.conv2d(a, w, padding=pad)
    if defect == "pad_before_act":
        assert r.gn and r.k == 3 and r.kind != "sparse"
        a = stage_fp32(r, gnd, F.pad(x, (1, 1, 1, 1)))
        if r.route in WINO_ROUTES:
            v = wino(F.pad(a, (0, 0, 3, 3)), w)[:, :, 4:-4, 1:-1]       # (quads stay aligned: 4 rows of padding above)
        else:
            v = F.conv2d(a, w)
    else:
        a = stage_fp32(r, gnd, x)
        v = conv(a, w)
    th, tw = TILE.get(r.route, (1, 128))
    ty, tx = (r.H // th - 1) * th, (r.W // tw - 1) * tw if r.W >= tw else 0
    tile = (slice(r.B - 1, r.B), slice(0, min(32, r.Cout)), slice(ty, ty + th), slice(tx, tx + tw))
    nch = -(-cin // 32)                                      # slices of whole chunks: the F(4,3) kernel, and 1x1 flat launches
    first = _slices(nch, r.ks)[0] if r.ks and (r.route in WINO_ROUTES or r.k == 1) else nch
    assert defect != "slice_twice" or first < nch
    if defect == "drop_last_chunk":
        lo = 32 * (first - 1)
        v[tile] -= F.conv2d(a[tile[0], lo:lo + 32], w[tile[1], lo:lo + 32], padding=pad)[:, :, tile[2], tile[3]]
    if defect == "slice_twice":
        v = v + F.conv2d(a[:, :32 * first], w[:, :32 * first], padding=pad)
    if r.bias:
        v = v + i.bias[None, :, None, None]
    if r.bias2:
        b2 = i.bias2[:, :r.Cout]
        if defect == "bias2_sample0":
            b2 = b2[:1].expand(r.B, -1)
        v = v + b2[:, :, None, None]
    if r.res:
        v = v + i.res
    v = v * torch.tensor(r.scale, dtype=torch.float32)
    if defect == "tile_shift":
        v = v.clone()
        v[tile] = v[tile].roll(1, 3)
    if defect == "swap_quads":
        v = v.clone()
        t = (tile[0], slice(0, 8), tile[2], tile[3])
        v[t] = v[t].roll(4, 1)
    return v


def where(r, idx, shape):
    """the element `idx` (flat) named by its place in the kernel's tile"""
    n, co, y, x = (int(v) for v in torch.unravel_index(torch.tensor(idx), shape))
    if r.route in TILE:
        th, tw = TILE[r.route]
        return f"(b, y % {th}, x % {tw}, channel) = ({n}, {y % th}, {x % tw}, {co})  [y {y}, x {x}]"
    m = (n * r.H + y) * r.W + x
    return f"(b, y, x, channel) = ({n}, {y}, {x}, {co})  [flat pixel {m}, {m % 128} of its 128]"


def check(r, got, R):
    """Both checks on `got` (fp32 NCHW cpu).  Returns (fails, report, (max |d| / bound, rel-L2))."""
    g = got.double()
    d = (g - R.ref).abs()
    fails = []
    if not bool(torch.isfinite(g).all()):
        fails.append("non-finite output")
    rel = float((g - R.ref).norm() / R.ref.norm())
    q = d / R.bound
    q[R.bound == 0] = (d[R.bound == 0] != 0).double() * float("inf")
    q = torch.nan_to_num(q, nan=0.0)
    ratio = float(q.max())
    if not ratio <= 1.0:
        idx = int(q.argmax())
        fails.append(f"max |d| / bound = {ratio:.3g} at {where(r, idx, q.shape)}: got {float(g.reshape(-1)[idx])!r} ref "
                     f"{float(R.ref.reshape(-1)[idx])!r} ({int((q > 1).sum())} elements over)")
    if not rel < REL_L2:
        fails.append(f"rel-L2 {rel:.3e} >= {REL_L2}")
    return fails, f"max|d|/bound {ratio:.2e}  rel-L2 {rel:.2e}", (ratio, rel)


# ------------------------------------------------------------------------------------------------------- probe rows
def probe_expected(r, stats=None):
    """(want, tol, inside), each [B, taps Cin, H, W]: block t = the staged operand of tap t shifted by the tap's offset, 0
    where the tap leaves the image; tol = tau there (0 without GN: bit for bit)"""
    a64, tau = staged(r, gn_data(r, stats))
    if tau is None:
        tau = torch.zeros_like(a64)
    p = r.k // 2
    parts = [[], [], []]
    for t in range(r.k * r.k):
        ky, kx = t // r.k, t % r.k
        for lst, src in zip(parts, (a64, tau, torch.ones_like(a64))):
            lst.append(F.pad(src, (p, p, p, p))[:, :, ky:ky + r.H, kx:kx + r.W])
    want, tol, inside = (torch.cat(q, 1) for q in parts)
    return want, tol, inside.bool()


def check_probe(r, got, stats=None):
    want, tol, inside = probe_expected(r, stats)
    g = got.double()
    fails = []
    n_out = int((g[~inside] != 0).sum())
    if n_out:
        fails.append(f"{n_out} out-of-image taps are not exactly 0")
    bad = ((g - want).abs() > tol) & inside
    if int(bad.sum()):
        idx = int(bad.reshape(-1).double().argmax())
        cin = r.C1 + r.C2
        co = (idx // (r.H * r.W)) % r.Cout
        fails.append(f"{int(bad.sum())} elements differ{' by more than tau' if r.gn else ''}; first at {where(r, idx, bad.shape)} "
                     f"= tap {co // cin} input channel {co % cin}: got {float(g.reshape(-1)[idx])!r} want "
                     f"{float(want.reshape(-1)[idx])!r}")
    worst = float(((g - want).abs() / tol)[inside & (tol > 0)].max()) if r.gn else 0.0
    return fails, f"{'max |d| / tau %.3f' % worst if r.gn else 'bit-exact'}"
