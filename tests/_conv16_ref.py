"""Cases, float64 reference and bounds for the large-image 16-bit storage convolution kernels: conv3x3_pc16_kernel
(conv16_pc.hip, route "pc16", with and without the folded 1x1 shortcut), conv3x3_halo_bf16_kernel<1, ...> in the storage
modes ("halo16"), conv_flat16_kernel ("flat16" / "flat16_splitk") and conv3x3_head4_16_kernel ("head4_16").

Shared by tests/test_conv16_bounds_host.py (CPU: an fp32 restatement of every case meets the bounds, four restated
defects miss them, every row sits in the edge class it claims) and tests/test_gpu_conv16.py (the kernels themselves).
Nothing here touches the library.

Reference: the kernel's expression in float64 on the operands AS THE KERNEL SEES THEM -- x, w and the folded shortcut's
x and w2 rounded once to the storage type; res rounded for 16-bit output, fp32 for out_f32 and head4; bias, bias2, bias_x
and the GroupNorm parameters fp32 (mean, scale per (sample, channel), beta per channel: GnParams); scale the float32
value.  16-bit x 16-bit products are exact in fp32: what is left is the fp32 accumulation, ONE output rounding and the
fp32 evaluation of the fused staging.

Fused GroupNorm (+ SiLU) input.  The kernels evaluate, in fp32,
    pc16            sh = fma(-m, s, b);  y = fma(x, s, sh);  z = fma(x, -L s, -L sh);  a = y * rcp(1 + exp2(z))
    halo16, head4   y = fma(x - m, s, b);                     z = -L y;                 a = y * rcp(1 + exp2(z))
(L = log2 e as a float), round a ONCE to the operand type and zero the out-of-image halo AFTER the activation.  The
reference operand is a_ref = round_dt(a64), a64 = y sigmoid(y) (or y) of the rounded x in float64.  The kernel may round
the other way only where a64 lies within tau of a midpoint between two storage values: the ambiguous set A =
{round_dt(a64 - tau) != round_dt(a64 + tau)}.

tau, counted from the code above with eps = 2^-23 per operation (a full ulp where round-to-nearest gives half of one, so
an unfused restatement with twice the roundings fits as well) and P = |x s| + |m s| + |b|, which bounds every
intermediate of the affine part:
    y      2 operations (pc16: the fma for sh, the fma for y; halo16 / head4: the subtraction -- eps (|x| + |m|) |s| -- and
           the fma), each <= eps P                                                              -> 2 eps P
    GroupNorm only:                                                                    tau = 2 eps P
    z      pc16: -L s, sh, -L sh, the fma, the float constant L: 5 operations, each <= eps L P; halo16 / head4: y's two,
           the product, the constant: 4.  An error dz of the exponent moves a = y sigmoid(y) by |y| sigma (1 - sigma) ln2 dz
           and |y| sigma (1 - sigma) < 1/4 for every y                                          -> 5/4 eps P
    sigma  v_exp_f32, the addition of 1, v_rcp_f32 and the final product: 4 operations, each one ulp of a value whose
           effect on a is <= |a|                                                                -> 4 eps |a64|
    y's own error reaches a through sigma + y sigma (1 - sigma) <= 1.1: with the above < 3.5 eps P + 4 eps |a64|
    GroupNorm + SiLU:                                                                  tau = 4 eps (P + |a64|)
tau is derived here and nowhere fitted to a device's output.

Per-element bound:  |got - ref| <= u |ref| + acc + amb  (+ 2^-25 for fp16 output: half a subnormal step); fp32 output
(head4, out_f32) drops the u term.  u = 2^-8 (bf16) / 2^-11 (fp16).
  acc = (K + ks + 16) 2^-23 S:  K products per output (taps Cin, plus the shortcut's channels in the fold), ks the flat
        kernel's slice count (else 0), S = (conv(|a_ref|, |w|) + |bias| + |bias2| + |bias_x| + |res|) |scale| in float64.  As
        in _smallm_ref.py every operation is charged a full ulp of a partial result that S bounds, which also covers a
        matrix-core adder that truncates.
  amb = conv(1_A ulp_dt(a_ref), |w|) |scale|: every ambiguous input may sit one storage step away (computed as
        round_dt(a64 + tau) - round_dt(a64 - tau), which IS 1_A ulp_dt(a_ref) except next to zero, where the storage step is
        below tau and the kernel may land several steps away).  Zero without GN.
Second check, rows without fused GN: got != round_dt(ref) for at most MISMATCH_CAP = 2e-2 of the elements (16-bit
output), rel-L2 < 2e-5 (fp32 output).

Conditions on the inputs (the host test verifies them for every GN row): A holds at most 5 % of the staged inputs, and the
median over the outputs of amb / (u |ref|) is at most 1, so the fused-GN bound stays within 2 x of the plain one.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

SCALE = 0.70710678
EPS = 2.0 ** -23
REL_L2_F32 = 2e-5
MISMATCH_CAP = 2e-2
AMBIGUOUS_CAP = 0.05
DTS = ("bf16", "f16")
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
DT_CODE = {"bf16": 1, "f16": 2}
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
ROUTES = ("pc16", "halo16", "flat16", "flat16_splitk", "head4_16")
BORDERS = ("all4", "strip_lr", "strip_tb", "edges", "interior")
CUS = 256                                    # compute units assumed by the tiles-per-block claims (MI355X)

# kind: "conv" (flowse_op_conv2d_16_ex), "fold" (flowse_op_resblock_tail_16), "probe" (staged-halo probe, section a)
# gn: 0 none, 1 GroupNorm only, 2 GroupNorm + SiLU.  Claims: chunks = 32-channel chunks of the 3x3, sc = shortcut steps,
# ipb = ((min, max) items per block with 128-channel blocks, the same with 64-channel blocks), border, ks.
Case = namedtuple("Case", "name route kind B H W C1 C2 Cout k gn bias bias2 res scale out32 X1 X2 chunks sc ipb border ks")

ONE = ((1, 1), (1, 1))


def _mk(name, route, geom, C1, Cout, *, chunks, border=None, ipb=None, ks=0, sc=0, k=3, C2=0, gn=2, bias=True, bias2=True,
        res=True, scale=SCALE, out32=False, X1=0, X2=0, kind="conv"):
    B, H, W = geom
    return Case(name, route, kind, B, H, W, C1, C2, Cout, k, gn, bias, bias2, res, scale, out32, X1, X2, chunks, sc, ipb,
                border, ks)


GN_TAG = {0: "plain", 1: "gn", 2: "gnsilu"}


def _build():
    cs = []
    # ---- a. staged-halo probe: Cout = 9 x 128, block t of the output = the staged operand of tap t
    for route, geom, border in (("pc16", (2, 32, 32), "edges"), ("halo16", (3, 24, 32), "edges")):
        for c1, c2 in ((128, 0), (64, 64)):
            for gn in (0, 1, 2):
                cs.append(_mk(f"probe-{route}-{'cat' if c2 else 'one'}-{GN_TAG[gn]}", route, geom, c1, 1152, C2=c2, gn=gn,
                              bias=False, bias2=False, res=False, scale=1.0, kind="probe", chunks=4, border=border,
                              ipb=ONE if route == "pc16" else None))
    # ---- b. pc16 geometry, Cin 32 -> Cout 128, all epilogue terms
    cs.append(_mk("pc-geo-64x16x16", "pc16", (64, 16, 16), 32, 128, chunks=1, border="all4", ipb=ONE))
    cs.append(_mk("pc-geo-16x64x16", "pc16", (16, 64, 16), 32, 128, chunks=1, border="strip_lr", ipb=ONE))
    cs.append(_mk("pc-geo-16x16x64", "pc16", (16, 16, 64), 32, 128, chunks=1, border="strip_tb", ipb=ONE))
    cs.append(_mk("pc-geo-1x128x128", "pc16", (1, 128, 128), 32, 128, chunks=1, border="interior", ipb=ONE))
    cs.append(_mk("pc-geo-17x32x32", "pc16", (17, 32, 32), 32, 128, chunks=1, border="edges", ipb=((1, 2), (1, 1))))
    cs.append(_mk("pc-geo-1x128x272", "pc16", (1, 128, 272), 32, 128, chunks=1, border="interior", ipb=((1, 1), (1, 2))))
    cs.append(_mk("pc-geo-3x112x128-256", "pc16", (3, 112, 128), 32, 256, chunks=1, border="interior", ipb=((1, 2), (2, 3))))
    # ---- c. pc16 chunk counts: every residue of the three halo buffers and of the three-entry B ring
    for cin in (32, 64, 96, 128, 160, 256):
        if cin != 32:
            cs.append(_mk(f"pc-chunks-{cin}", "pc16", (16, 32, 32), cin, 128, chunks=cin // 32, border="edges", ipb=ONE))
    cs.append(_mk("pc-chunks-32", "pc16", (16, 32, 32), 32, 128, chunks=1, border="edges", ipb=ONE))
    for c1, c2, n in ((32, 32, 2), (64, 32, 3), (32, 64, 3), (256, 128, 12)):
        cs.append(_mk(f"pc-cat-{c1}+{c2}", "pc16", (16, 32, 32), c1, 128, C2=c2, chunks=n, border="edges", ipb=ONE))
    # ---- d. pc16 epilogue terms one by one
    e = dict(chunks=1, border="edges", ipb=((1, 2), (1, 1)))
    cs.append(_mk("pc-epi-nobias", "pc16", (17, 32, 32), 32, 128, bias=False, **e))
    cs.append(_mk("pc-epi-nobias2", "pc16", (17, 32, 32), 32, 128, bias2=False, **e))
    cs.append(_mk("pc-epi-nores", "pc16", (17, 32, 32), 32, 128, res=False, **e))
    cs.append(_mk("pc-epi-scale1", "pc16", (17, 32, 32), 32, 128, scale=1.0, **e))
    cs.append(_mk("pc-epi-gnonly", "pc16", (17, 32, 32), 32, 128, gn=1, **e))
    cs.append(_mk("pc-epi-plain", "pc16", (17, 32, 32), 32, 128, gn=0, **e))
    # ---- e. folded 1x1 shortcut (no bias2, no residual: the launcher's contract)
    widths = ((96, 0, 3), (128, 0, 4), (160, 0, 5), (64, 32, 3), (32, 64, 3), (256, 256, 16))
    for x1, x2, n in widths:
        for gn in (0, 1, 2):
            cs.append(_mk(f"fold-{x1}+{x2}-{GN_TAG[gn]}", "pc16", (16, 32, 32), 64, 128, gn=gn, bias2=False, res=False, X1=x1,
                          X2=x2, kind="fold", chunks=2, sc=n, border="edges", ipb=ONE))
    for i, (x1, x2, n) in enumerate(widths + ((64, 32, 3), (64, 32, 3))):
        gn = (2, 1, 0, 0, 2, 1, 1, 2)[i]                     # 64+32 in all three modes, the other widths in one each
        cs.append(_mk(f"fold-big-{x1}+{x2}-{GN_TAG[gn]}", "pc16", (3, 112, 128), 64, 256, gn=gn, bias2=False, res=False,
                      X1=x1, X2=x2, kind="fold", chunks=2, sc=n, border="interior", ipb=((1, 2), (2, 3))))
    # ---- f. halo16: H = 8 (mod 16)
    cs.append(_mk("halo-8x8x256", "halo16", (8, 8, 256), 32, 128, chunks=1, border="strip_tb"))
    cs.append(_mk("halo-22x24x16-256", "halo16", (22, 24, 16), 32, 256, chunks=1, border="strip_lr"))
    for c1, c2 in ((32, 0), (64, 0), (96, 0), (64, 32)):
        cs.append(_mk(f"halo-6x24x128-{c1}+{c2}", "halo16", (6, 24, 128), c1, 128, C2=c2, chunks=(c1 + c2) // 32,
                      border="interior"))
    for gn in (0, 1):
        cs.append(_mk(f"halo-6x24x128-{GN_TAG[gn]}", "halo16", (6, 24, 128), 32, 128, gn=gn, chunks=1, border="interior"))
    for gn in (0, 1, 2):
        cs.append(_mk(f"halo-6x24x128-bare-{GN_TAG[gn]}", "halo16", (6, 24, 128), 32, 128, gn=gn, bias2=False, res=False,
                      chunks=1, border="interior"))
    # ---- g. flat16 (no fused GN on this route)
    for o32 in (False, True):
        t = "-f32" if o32 else ""
        cs.append(_mk(f"flat-3x3-64x64{t}", "flat16_splitk", (1, 64, 64), 256, 256, gn=0, out32=o32, chunks=8, ks=8))
        cs.append(_mk(f"flat-1x1-cat{t}", "flat16_splitk", (2, 32, 64), 256, 128, C2=128, k=1, gn=0, out32=o32, chunks=12, ks=3))
        cs.append(_mk(f"flat-1x1-46x46{t}", "flat16", (1, 46, 46), 32, 128, k=1, gn=0, out32=o32, chunks=1, ks=1))
        cs.append(_mk(f"flat-3x3-46x46{t}", "flat16_splitk", (1, 46, 46), 32, 128, gn=0, out32=o32, chunks=1, ks=2))
    cs.append(_mk("flat-3x3-64x64-nobias2", "flat16_splitk", (1, 64, 64), 256, 256, gn=0, bias2=False, chunks=8, ks=8))
    # ---- h. head4_16: Cout 4, fp32 residual and output, no per-sample bias (the dispatch's condition)
    h = dict(bias2=False, out32=True)
    for cin in (32, 64, 96, 128):
        cs.append(_mk(f"head4-4x64x64-{cin}", "head4_16", (4, 64, 64), cin, 4, chunks=cin // 32, border="interior", **h))
    for geom, border in (((64, 16, 16), "all4"), ((1, 128, 128), "interior")):
        for cin in (64, 96, 128):
            cs.append(_mk(f"head4-{geom[0]}x{geom[1]}x{geom[2]}-{cin}", "head4_16", geom, cin, 4, chunks=cin // 32,
                          border=border, **h))
        for gn in (0, 1, 2):
            cs.append(_mk(f"head4-{geom[0]}x{geom[1]}x{geom[2]}-{GN_TAG[gn]}", "head4_16", geom, 32, 4, gn=gn, chunks=1,
                          border=border, **h))
    for gn in (0, 1, 2):
        cs.append(_mk(f"head4-4x64x64-nores-{GN_TAG[gn]}", "head4_16", (4, 64, 64), 32, 4, gn=gn, res=False, chunks=1,
                      border="interior", **h))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
CONV_CASES = [c for c in CASES if c.kind != "probe"]
PROBE_CASES = [c for c in CASES if c.kind == "probe"]
REPRO = ("pc-geo-3x112x128-256", "halo-6x24x128-64+32", "flat-3x3-64x64")


# ------------------------------------------------------------------------------------------ the table's claims, restated
def border_of(c):
    """border class of the row's tiling: 16 x 16-pixel tiles (pc16, head4_16) or 8 x 16 (halo16)"""
    ty, tx = c.H // (8 if c.route == "halo16" else 16), c.W // 16
    if ty == 1 and tx == 1:
        return "all4"
    if tx == 1:
        return "strip_lr"
    if ty == 1:
        return "strip_tb"
    return "edges" if ty == 2 or tx == 2 else "interior"


def items_per_block(c, nj, cus=CUS):
    """(min, max) work items of a block of the persistent kernel: items dealt over min(items, CUs) & ~7 blocks"""
    items = (c.B * c.H * c.W // 256) * (c.Cout // 128) * (2 if nj == 1 else 1)
    grid = min(items, cus) & ~7
    return items // grid, -(-items // grid)


def ksplit_of(c):
    """K slices of the flat kernel for the row's shape (the policy's arithmetic, restated)"""
    M = c.B * c.H * c.W
    tiles = -(-M // 128) * -(-c.Cout // 128)
    stages = ((c.C1 + c.C2) // 32 * c.k * c.k + 1) // 2
    if tiles >= 256 or stages < 4:
        return 1
    ks = max(1, min(-(-512 // tiles), stages // 2))
    per = -(-stages // ks)
    return -(-stages // per)


def k_of(c):
    return c.k * c.k * (c.C1 + c.C2) + c.X1 + c.X2


# ------------------------------------------------------------------------------------------------------------- inputs
Inputs = namedtuple("Inputs", "x w bias bias2 res mean scl beta xs w2 bias_x")
_inputs = {}


def rnd_dt(t, dt):
    """t (any float type) rounded once to the storage type, widened to float64"""
    return t.to(DT[dt]).double() if dt else t.double()


def inputs(c):
    """fp32 tensors of a row (NCHW; bias2 [B, Cout + 8]: a row stride that is not Cout), seeded by shape -- rows that
    differ only in the epilogue terms, the GN mode or the types share them.  Probe rows: the one-hot weights."""
    key = (c.B, c.H, c.W, c.C1, c.C2, c.Cout, c.k, c.X1, c.X2, c.kind == "probe")
    if key not in _inputs:
        seed = 0
        for v in key:
            seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
        g = torch.Generator().manual_seed(seed)
        cin = c.C1 + c.C2
        x = torch.randn(c.B, cin, c.H, c.W, generator=g)
        if c.kind == "probe":
            w = torch.zeros(c.Cout, cin, 3, 3)
            ch = torch.arange(cin)
            for t in range(9):
                w[cin * t + ch, ch, t // 3, t % 3] = 1.0
        else:
            w = torch.randn(c.Cout, cin, c.k, c.k, generator=g) / (cin * c.k * c.k) ** 0.5
        bias = 0.5 * torch.randn(c.Cout, generator=g)
        bias2 = 0.5 * torch.randn(c.B, c.Cout + 8, generator=g)
        res = torch.randn(c.B, c.Cout, c.H, c.W, generator=g)
        mean = 0.2 * torch.randn(c.B, cin, generator=g)
        scl = 1 + 0.2 * torch.randn(c.B, cin, generator=g)
        beta = 0.2 * torch.randn(cin, generator=g)
        xs = w2 = bias_x = None
        if c.X1:
            xc = c.X1 + c.X2
            xs = torch.randn(c.B, xc, c.H, c.W, generator=g)
            w2 = torch.randn(c.Cout, xc, 1, 1, generator=g) / xc ** 0.5
            bias_x = 0.5 * torch.randn(c.Cout, generator=g)
        _inputs[key] = Inputs(x, w, bias, bias2, res, mean, scl, beta, xs, w2, bias_x)
        if len(_inputs) > 6:
            _inputs.pop(next(iter(_inputs)))
    i = _inputs[key]
    return i._replace(bias=i.bias if c.bias else None, bias2=i.bias2 if c.bias2 else None, res=i.res if c.res else None)


# ------------------------------------------------------------------------------------------------- the staged operand
Staged = namedtuple("Staged", "a64 a A step lo hi")


def staged(c, dt, x=None):
    """The conv's 3x3 operand as the kernel stages it, in float64: a64 (exact expression on the rounded x), a = a_ref =
    round_dt(a64), lo / hi = round_dt(a64 -/+ tau): the storage values an fp32 evaluation within tau of a64 can round to, A =
    the ambiguous set (lo != hi: a64 within tau of a midpoint), step = hi - lo (the storage step at a_ref wherever that
    step exceeds 2 tau -- all but values next to zero, where several storage values lie within tau)"""
    i = inputs(c)
    xr = rnd_dt(i.x if x is None else x, dt)
    if not c.gn:
        return Staged(xr, xr, None, None, xr, xr)
    m, s = i.mean.double()[:, :, None, None], i.scl.double()[:, :, None, None]
    b = i.beta.double()[None, :, None, None]
    y = xr * s + (b - m * s)
    P = (xr * s).abs() + (m * s).abs() + b.abs()
    if c.gn == 2:
        a64 = y * torch.sigmoid(y)
        tau = 4 * EPS * (P + a64.abs())
    else:
        a64 = y
        tau = 2 * EPS * P
    lo, hi = rnd_dt(a64 - tau, dt), rnd_dt(a64 + tau, dt)
    return Staged(a64, rnd_dt(a64, dt), lo != hi, hi - lo, lo, hi)


def restate_staging(c, dt, x, defect=None):
    """The staging in torch fp32 as the kernel writes it (exp2 and a reciprocal; unfused multiplies and adds), rounded
    once to the storage type.  defect "round_twice": the affine result is rounded to the storage type before SiLU."""
    i = inputs(c)
    xr = x.to(DT[dt]).float()
    if not c.gn:
        return xr
    L = torch.tensor(-1.44269504088896341, dtype=torch.float32)
    m, s, b = i.mean[:, :, None, None], i.scl[:, :, None, None], i.beta[None, :, None, None]
    sh = b - m * s
    y = xr * s + sh
    if defect == "round_twice":
        y = y.to(DT[dt]).float()
        z = L * y
    else:
        z = xr * (L * s) + L * sh
    if c.gn == 2:
        y = y * torch.reciprocal(1 + torch.exp2(z))
    return y.to(DT[dt]).float()


# -------------------------------------------------------------------------------------------------------- reference
Ref = namedtuple("Ref", "ref acc amb")
_refs = {}


def reference(c, dt):
    """Ref(ref, acc, amb): the float64 result, the accumulation allowance and the ambiguity allowance per element"""
    key = (c, dt)
    if key in _refs:
        return _refs[key]
    i = inputs(c)
    st = staged(c, dt)
    w = rnd_dt(i.w, dt)
    pad = c.k // 2
    ref = F.conv2d(st.a, w, padding=pad)
    stack = [st.a.abs()] + ([st.step] if c.gn else [])
    mags = F.conv2d(torch.cat(stack, 0), w.abs(), padding=pad)
    mag = mags[:c.B].clone()
    amb = mags[c.B:].clone() if c.gn else torch.zeros_like(mag)
    if c.X1:
        xs, w2 = rnd_dt(i.xs, dt), rnd_dt(i.w2, dt)
        ref += F.conv2d(xs, w2)
        mag += F.conv2d(xs.abs(), w2.abs())
        ref += i.bias_x.double()[None, :, None, None]
        mag += i.bias_x.double().abs()[None, :, None, None]
    if i.bias is not None:
        ref += i.bias.double()[None, :, None, None]
        mag += i.bias.double().abs()[None, :, None, None]
    if i.bias2 is not None:
        b2 = i.bias2[:, :c.Cout].double()[:, :, None, None]
        ref += b2
        mag += b2.abs()
    if i.res is not None:
        r = rnd_dt(i.res, None if c.out32 else dt)
        ref += r
        mag += r.abs()
    s = float(torch.tensor(c.scale, dtype=torch.float32))
    out = Ref(ref * s, (k_of(c) + c.ks + 16) * EPS * mag * abs(s), amb * abs(s))
    _refs.clear()                                            # one row at a time: the tensors are large
    _refs[key] = out
    return out


def restate_fp32(c, dt, defect=None):
    """The kernel's arithmetic restated with torch fp32 on the CPU (another summation order, the same roundings).
    Defects: "pad_before_gn" (out-of-image halo pixels become act(b - m s)), "round_before_res" (the output is rounded before
    the residual is added and again after), "bias2_next_sample" (sample n's tiles take sample n - 1's row), "round_twice"
    (see restate_staging)."""
    i = inputs(c)
    pad = c.k // 2
    store = (lambda t: t) if c.out32 else (lambda t: t.to(DT[dt]).float())
    w = i.w.to(DT[dt]).float()
    if defect == "pad_before_gn":
        v = F.conv2d(restate_staging(c, dt, F.pad(i.x, (pad,) * 4)), w)
    else:
        v = F.conv2d(restate_staging(c, dt, i.x, defect), w, padding=pad)
    if c.X1:
        v = v + F.conv2d(i.xs.to(DT[dt]).float(), i.w2.to(DT[dt]).float()) + i.bias_x[None, :, None, None]
    if i.bias is not None:
        v = v + i.bias[None, :, None, None]
    if i.bias2 is not None:
        b2 = i.bias2[:, :c.Cout]
        if defect == "bias2_next_sample":
            b2 = b2.roll(1, 0)
        v = v + b2[:, :, None, None]
    if i.res is not None:
        if defect == "round_before_res":
            v = store(v)
        v = v + store(i.res)
    return store(v * torch.tensor(c.scale, dtype=torch.float32))


def check(c, dt, got, R=None):
    """Applies the bounds of the module docstring to `got` (fp32 NCHW cpu).  Returns (fails, report, figures): a list of
    strings (empty = pass), the line to print and (max |d| / bound, mismatch share or rel-L2)."""
    R = R or reference(c, dt)
    ref, acc, amb = R
    g = got.double()
    d = (g - ref).abs()
    fails = []
    if not bool(torch.isfinite(g).all()):
        fails.append("non-finite output")
    if c.out32:
        tight = torch.zeros_like(acc)
        second = float((g - ref).norm() / ref.norm())
        text = f"rel-L2 {second:.2e}"
        if not c.gn and not second < REL_L2_F32:
            fails.append(f"rel-L2 {second:.3e} >= {REL_L2_F32}")
    else:
        tight = UNIT[dt] * ref.abs() + (2.0 ** -25 if dt == "f16" else 0.0)
        second = float((g != rnd_dt(ref, dt)).double().mean())
        text = f"mismatch {second:.2e}"
        if not c.gn and not second <= MISMATCH_CAP:
            fails.append(f"{second:.3e} of the elements differ from round(ref) (cap {MISMATCH_CAP})")
    bound = tight + acc + amb
    q = d / bound
    ratio = float(q.max())
    if not ratio <= 1.0:
        idx = int(q.argmax())
        n, co, y, x = (int(v) for v in torch.unravel_index(torch.tensor(idx), q.shape))
        fails.append(f"max |d| / bound = {ratio:.3f} at (sample {n}, channel {co}, y {y}, x {x}): got "
                     f"{float(g.reshape(-1)[idx])!r} ref {float(ref.reshape(-1)[idx])!r}")
    acc_ratio = float(((d - tight - amb).clamp_min(0) / acc).max())
    return fails, f"max|d|/bound {ratio:.3f}  excess/acc {acc_ratio:.3f}  {text}", (ratio, second)


def gn_conditions(c, dt, R=None):
    """(share of the staged inputs in A, median over the outputs of amb / (u |ref|)) of a GN row"""
    R = R or reference(c, dt)
    share = float(staged(c, dt).A.double().mean())
    med = float((R.amb / (UNIT[dt] * R.ref.abs())).median())
    return share, med


# ------------------------------------------------------------------------------------------------------ probe rows
def probe_expected(c, dt):
    """Output of a probe row, exactly: (want, lo, hi, inside), each [B, 9 Cin, H, W] -- block t = the staged operand of
    tap t shifted by the tap's offset, 0 where the tap leaves the image (inside = False there)"""
    st = staged(c, dt)
    parts = [[], [], [], []]
    for t in range(9):
        ky, kx = t // 3, t % 3
        for lst, src in zip(parts, (st.a, st.lo, st.hi, torch.ones_like(st.a))):
            lst.append(F.pad(src, (1, 1, 1, 1))[:, :, ky:ky + c.H, kx:kx + c.W])
    want, lo, hi, inside = (torch.cat(p, 1) for p in parts)
    return want, lo, hi, inside.bool()


def check_probe(c, dt, got):
    """bit-exact outside the ambiguous set, one of the neighbouring storage values [lo, hi] inside it, exactly 0 outside
    the image"""
    want, lo, hi, inside = probe_expected(c, dt)
    A = lo != hi
    g = got.double()
    fails = []
    n_out = int((g[~inside] != 0).sum())
    if n_out:
        fails.append(f"{n_out} out-of-image taps are not exactly 0")
    bad = (g != want) & ~A & inside
    if int(bad.sum()):
        idx = int(bad.reshape(-1).double().argmax())
        n, co, y, x = (int(v) for v in torch.unravel_index(torch.tensor(idx), bad.shape))
        fails.append(f"{int(bad.sum())} elements outside the ambiguous set differ; first at (sample {n}, channel {co} = tap "
                     f"{co // (c.C1 + c.C2)} input channel {co % (c.C1 + c.C2)}, y {y}, x {x}): got "
                     f"{float(g.reshape(-1)[idx])!r} want {float(want.reshape(-1)[idx])!r}")
    bad_a = A & inside & ((g < lo) | (g > hi))
    if int(bad_a.sum()):
        fails.append(f"{int(bad_a.sum())} ambiguous elements are neither neighbouring storage value")
    flipped = int((A & inside & (g != want)).sum())
    return fails, f"ambiguous {float(A.double().mean()):.2e}  flipped {flipped} of {int((A & inside).sum())}"
