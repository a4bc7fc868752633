"""Cases, float64 reference and bounds for the small-image split-K convolution kernels (conv_smallm.hip, conv16_smallm.hip).

Shared by tests/test_smallm_bounds_host.py (CPU: an fp32 restatement of every case meets the bounds, every case sits in the
ring class its row claims) and tests/test_gpu_smallm.py (the kernels themselves).  Nothing here touches the library.

The kernels: a block owns a 32 x (32 | 64) (or 16 x 16) output tile, its eight waves each take every eighth K step (tap,
32-channel chunk) through a branch-free register ring D steps deep, the eight fp32 partial tiles are summed in a fixed
order, bias + per-sample bias + residual are added, the sum is scaled and rounded to the storage type ONCE.

Reference: the same expression in float64 on the operands AS THE KERNEL SEES THEM -- for the 16-bit kernels x, w and (16-bit
output only) res rounded to the storage type; bias, bias2 stay fp32, scale is the float32 value.  bf16 x bf16 and fp16 x fp16
products are exact in fp32, so what is left is the fp32 accumulation and, for 16-bit output, exactly one rounding.

Accumulation allowance per element:  acc = (32 nstep + 16) 2^-23 S,  nstep = ceil(taps Cin / 32 / 8) (K steps of the
busiest wave), S = (conv(|x|, |w|) + |bias| + |bias2| + |res|) |scale| in float64: an output is eight per-wave chains of at
most 32 nstep products, then the eight-way sum, bias, bias2, residual and scale (<= 16 operations); every operation is
charged one full ulp (2^-23) of a partial result that |.| <= S bounds, which also covers a matrix-core adder that
truncates instead of rounding to nearest.

  fp32 output  : |got - ref| <= acc for every element, and rel-L2 < 2e-5 (the project's fp32 figure)
  16-bit output: |got - ref| <= u |ref| + acc (+ 2^-25 for fp16: half a subnormal step) with u = 2^-8 (bf16) / 2^-11 (fp16),
                 and got != round(ref) for at most 2e-2 of the elements (a condition: one rounding differs from round(ref)
                 only where acc moves the sum across a rounding boundary, about acc / ulp_dt of the elements -- 1e-3 and
                 less here; rounding twice or truncating gives 0.25 and more)
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

SCALE = 0.70710678
REL_L2_F32 = 2e-5
MISMATCH_CAP = 2e-2
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
DT_CODE = {"bf16": 1, "f16": 2}
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}

# instance -> ring depth D and the route string the library reports for it (flowse_op_last_conv_route)
F32_INSTANCES = {"smallm<1>": 4, "smallm<2>": 2, "smallm_tile16": 8}


def inst16(nt2, dt, out32):
    return f"smallm16b<{nt2}, {dt}, {'out32' if out32 else 'out16'}>"


INSTANCES = dict(F32_INSTANCES)
for _nt2, _d in ((1, 8), (2, 6)):
    for _dt in ("bf16", "f16"):
        for _o in (False, True):
            INSTANCES[inst16(_nt2, _dt, _o)] = _d

RING_CLASSES = ("n1", "Dm1", "D", "Dp1", "3Dm1", "few", "ragged")

Case = namedtuple("Case", "name inst dt out32 ring B H W C1 C2 Cout k bias bias2 res scale")


def _mk(name, inst, ring, geom, C1, Cout, k=3, C2=0, bias=True, bias2=True, res=True, scale=SCALE):
    dt, out32 = None, True
    if inst.startswith("smallm16b"):
        dt = "bf16" if ", bf16" in inst else "f16"
        out32 = inst.endswith("out32>")
    B, H, W = geom
    return Case(name, inst, dt, out32, ring, B, H, W, C1, C2, Cout, k, bias, bias2, res, scale)


# 3x3 input widths that land nstep on D - 1, D, D + 1 and 2 D + (D - 1); one more with S_all % 8 != 0 off those lengths
_RING_CIN = {8: {"Dm1": 192, "D": 224, "Dp1": 256, "3Dm1": 640, "ragged": 320},
             6: {"Dm1": 128, "D": 160, "Dp1": 192, "3Dm1": 480, "ragged": 320},
             4: {"Dm1": 64, "D": 96, "Dp1": 128, "3Dm1": 288, "ragged": 160},
             2: {"D": 32, "Dp1": 64, "3Dm1": 128, "ragged": 96}}


def _build():
    cases = []
    for inst, D in INSTANCES.items():
        wide = inst == "smallm<2>" or inst.startswith("smallm16b<2")
        is16 = inst.startswith("smallm16b")
        tag = inst.replace("smallm16b<", "s16b").replace("smallm", "s").replace(", ", "_").replace("<", "").replace(">", "")
        if wide:
            base, cout = (8, 16, 16), 256                  # 64 tiles x 4 channel blocks = one block per CU
        elif inst == "smallm_tile16":
            base, cout = (3, 4, 8), 32                     # six 16-pixel tiles x two 16-channel blocks
        elif inst == "smallm<1>":
            base, cout = (3, 6, 6), 64                     # 108 pixels: last tile 12 of 32 rows, tiles span samples
        else:
            base, cout = (5, 2, 4), 64                     # 40 pixels: last tile 8 of 32 rows, four samples per tile
        # ---- ring classes
        n1 = "n1+Dm1" if D == 2 else "n1"                  # D = 2: nstep = D - 1 IS nstep = 1
        cases.append(_mk(f"{tag}-n1", inst, n1, base, 256, cout, k=1))                 # S_all = 8: every wave one live step
        cases.append(_mk(f"{tag}-few", inst, "few", base, 96 if is16 else 32, cout, k=1))   # S_all = 3 / 1: idle waves
        for ring, cin in _RING_CIN[D].items():
            cases.append(_mk(f"{tag}-{ring}", inst, ring, base, cin, cout))
        # ---- geometry
        cases.append(_mk(f"{tag}-nobias", inst, "", base, 32, cout, bias=False, bias2=False))
        if wide:
            cases.append(_mk(f"{tag}-255x2x4", inst, "", (255, 2, 4), 256, 256))        # last tile 24 of 32 rows, 4 samples per tile
            cases.append(_mk(f"{tag}-1x32x32", inst, "", (1, 32, 32), 512, 512))
            cases.append(_mk(f"{tag}-cat256", inst, "", base, 256, cout, C2=256))
        elif inst == "smallm_tile16":
            cases.append(_mk(f"{tag}-1x4x4", inst, "", (1, 4, 4), 64, 32))
            cases.append(_mk(f"{tag}-16x4x4", inst, "", (16, 4, 4), 64, 32))
            cases.append(_mk(f"{tag}-cat96", inst, "", base, 64, cout, C2=32))
        else:
            cases.append(_mk(f"{tag}-2x32x32-n32", inst, "", (2, 32, 32), 64, 32))      # the 2048-pixel limit, narrow tiles
            cases.append(_mk(f"{tag}-2x32x32-n96", inst, "", (2, 32, 32), 64, 96))
            for g in ((24, 1, 1), (32, 1, 1), (16, 1, 2), (5, 2, 4)):
                if g != base:
                    cases.append(_mk(f"{tag}-{g[0]}x{g[1]}x{g[2]}", inst, "", g, 64, 64))
            cases.append(_mk(f"{tag}-cat96", inst, "", base, 64, cout, C2=32))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def ring_numbers(c):
    """(S_all, nstep) of a case: K steps in all and per wave (the busiest one)"""
    s_all = c.k * c.k * (c.C1 + c.C2) // 32
    return s_all, (s_all + 7) // 8


def ring_classes_of(c):
    """every ring class the case's K falls into for its instance's ring depth"""
    D = INSTANCES[c.inst]
    s_all, nstep = ring_numbers(c)
    out = set()
    if nstep == 1:
        out.add("n1")
    for name, n in (("Dm1", D - 1), ("D", D), ("Dp1", D + 1), ("3Dm1", 3 * D - 1)):
        if nstep == n:
            out.add(name)
    if s_all < 8:
        out.add("few")
    if s_all % 8:
        out.add("ragged")
    return out


def rnd_dt(t, dt):
    """t (any float type) rounded once to the storage type, widened to float64"""
    return t.to(DT[dt]).double() if dt else t.double()


_inputs, _convs = {}, {}


def inputs(c):
    """fp32 tensors of a case (NCHW; bias2 [B, Cout + 8]: a row stride that is not Cout), seeded by shape -- cases that
    differ only in the storage / output type share them"""
    key = (c.B, c.H, c.W, c.C1, c.C2, c.Cout, c.k)
    if key not in _inputs:
        seed = 0
        for v in key:
            seed = (seed * 1000003 + v) % (2 ** 31 - 1)
        g = torch.Generator().manual_seed(seed)
        cin = c.C1 + c.C2
        x = torch.randn(c.B, cin, c.H, c.W, generator=g)
        w = torch.randn(c.Cout, cin, c.k, c.k, generator=g) / (cin * c.k * c.k) ** 0.5
        bias = 0.5 * torch.randn(c.Cout, generator=g)
        bias2 = 0.5 * torch.randn(c.B, c.Cout + 8, generator=g)
        res = torch.randn(c.B, c.Cout, c.H, c.W, generator=g)
        _inputs[key] = (x, w, bias, bias2, res)
    x, w, bias, bias2, res = _inputs[key]
    return x, w, (bias if c.bias else None), (bias2 if c.bias2 else None), (res if c.res else None)


def _conv64(c):
    """float64 conv(x, w) and conv(|x|, |w|) on the operands as the kernel sees them; computed once per (shape, type)"""
    key = (c.B, c.H, c.W, c.C1, c.C2, c.Cout, c.k, c.dt)
    if key not in _convs:
        x, w = inputs(c)[:2]
        xd, wd = rnd_dt(x, c.dt), rnd_dt(w, c.dt)
        _convs[key] = (F.conv2d(xd, wd, padding=c.k // 2), F.conv2d(xd.abs(), wd.abs(), padding=c.k // 2))
        if len(_convs) > 40:
            _convs.pop(next(iter(_convs)))
    return _convs[key]


def reference(c):
    """(ref, acc): the float64 result and the per-element accumulation allowance"""
    _, _, bias, bias2, res = inputs(c)
    conv, mag = _conv64(c)
    ref, mag = conv.clone(), mag.clone()
    if bias is not None:
        ref += bias.double()[None, :, None, None]
        mag += bias.double().abs()[None, :, None, None]
    if bias2 is not None:
        b2 = bias2[:, :c.Cout].double()[:, :, None, None]
        ref += b2
        mag += b2.abs()
    if res is not None:
        r = rnd_dt(res, None if c.out32 else c.dt)
        ref += r
        mag += r.abs()
    s = float(torch.tensor(c.scale, dtype=torch.float32))
    _, nstep = ring_numbers(c)
    return ref * s, (32 * nstep + 16) * 2.0 ** -23 * mag * abs(s)


def restate_fp32(c, defect=None):
    """The kernel's arithmetic restated with torch fp32 on the CPU (another summation order, the same roundings).
    defect "round_before_res": rounds to the storage type before the residual is added and again after."""
    x, w, bias, bias2, res = inputs(c)
    if c.dt:
        x, w = x.to(DT[c.dt]).float(), w.to(DT[c.dt]).float()
    v = F.conv2d(x, w, padding=c.k // 2)
    if bias is not None:
        v = v + bias[None, :, None, None]
    if bias2 is not None:
        v = v + bias2[:, :c.Cout, None, None]
    store = (lambda t: t) if c.out32 else (lambda t: t.to(DT[c.dt]).float())
    if res is not None:
        if defect == "round_before_res":
            v = store(v)
        v = v + store(res)
    return store(v * torch.tensor(c.scale, dtype=torch.float32))


def check(c, got, ref=None, acc=None):
    """Applies the bounds of the module docstring to `got` (fp32 NCHW cpu).  Returns (failures, report): a list of strings
    (empty = pass) and the figures to print: max |d| / bound, max |d| / acc where acc alone binds, mismatch share or rel-L2."""
    if ref is None:
        ref, acc = reference(c)
    g = got.double()
    d = (g - ref).abs()
    fails = []
    if not bool(torch.isfinite(g).all()):
        fails.append("non-finite output")
    if c.out32:
        bound = acc
        rel = float((g - ref).norm() / ref.norm())
        second = f"rel-L2 {rel:.2e}"
        if not rel < REL_L2_F32:
            fails.append(f"rel-L2 {rel:.3e} >= {REL_L2_F32}")
    else:
        bound = UNIT[c.dt] * ref.abs() + acc + (2.0 ** -25 if c.dt == "f16" else 0.0)
        want = ref.to(DT[c.dt]).double()
        share = float((g != want).double().mean())
        second = f"mismatch {share:.2e}"
        if not share <= MISMATCH_CAP:
            fails.append(f"{share:.3e} of the elements differ from round(ref) (cap {MISMATCH_CAP})")
    ratio = float((d / bound).max())
    if not ratio <= 1.0:
        i = int((d / bound).argmax())
        fails.append(f"max |d| / bound = {ratio:.3f} at flat index {i}: got {float(g.reshape(-1)[i])!r} "
                     f"ref {float(ref.reshape(-1)[i])!r}")
    acc_ratio = float(((d - (bound - acc)).clamp_min(0) / acc).max())
    return fails, f"max|d|/bound {ratio:.3f}  excess/acc {acc_ratio:.3f}  {second}"
