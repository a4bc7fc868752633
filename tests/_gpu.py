"""Helpers for the -m gpu tests: ctypes calls into libflowse_hip.so on torch 'cuda' tensors."""
import ctypes as C

import torch

from flowmse_amd import _lib

L = _lib.lib


def nhwc(x):
    """NCHW cpu/any -> NHWC contiguous cuda float32"""
    return x.permute(0, 2, 3, 1).contiguous().cuda().float()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def stream():
    return _lib.current_stream()


def conv_operands(x1, x2, w, taps, bias, bias2, res):
    """What every conv entry takes, on the device: the NHWC inputs (x2 may be None), w [Cout, Cin, k, k] packed as
    [Cout][taps][Cin], the bias, the per-sample bias table and the NHWC residual (each may be None)."""
    Cout, Cin = w.shape[:2]
    a1 = nhwc(x1)
    a2 = nhwc(x2) if x2 is not None else None
    wp = w.permute(0, 2, 3, 1).reshape(Cout, taps, Cin).contiguous().cuda()
    bb = bias.contiguous().cuda() if bias is not None else None
    b2 = bias2.contiguous().cuda() if bias2 is not None else None
    rr = nhwc(res) if res is not None else None
    return a1, a2, wp, bb, b2, rr


def conv2d(x1, w, bias=None, x2=None, bias2=None, res=None, scale=1.0, padding=None, splitk=False, res_in_place=False):
    """x*: NCHW cpu tensors; w: [Cout, Cin, k, k] (reference layout). Returns NCHW cpu.  res_in_place: the residual sits in
    the output buffer (res aliases out, as the Combine 1x1 runs)."""
    Cout, Cin, k, _ = w.shape
    taps = k * k
    a1, a2, wp, bb, b2, rr = conv_operands(x1, x2, w, taps, bias, bias2, res)
    B, H, W, C1 = a1.shape
    C2 = a2.shape[3] if a2 is not None else 0
    out = rr if res_in_place else torch.empty(B, H, W, Cout, device="cuda")
    scratch = None
    if splitk:
        n = L.flowse_op_conv2d_scratch_floats(B, H, W, C1 + C2, Cout, taps)
        scratch = torch.empty(max(n, 1), device="cuda")
        conv2d.last_split = n > 0
    _lib.check(L.flowse_op_conv2d(_lib.ptr(a1), C1, _lib.ptr(a2), C2, _lib.ptr(wp), _lib.ptr(bb), _lib.ptr(b2),
                                  b2.shape[1] if b2 is not None else 0, _lib.ptr(rr), _lib.ptr(out), B, H, W, Cout,
                                  taps, float(scale), _lib.ptr(scratch), stream()))
    torch.cuda.synchronize()
    return nchw(out)


class stats_sink:
    """Context manager around flowse_op_stats_sink: every per-op conv entry called inside leaves the fused GroupNorm partials
    of its output in a device buffer of `floats` floats (filled with NaN before).  After the block: .blocks = the launch's
    blocks per sample (0: its route writes none), .partial(B, Cout) = the [B, nblk, Cout, 2] (mean, M2) tensor on the cpu,
    .clean_beyond(B, Cout) = nothing was written past it."""

    def __init__(self, floats):
        self.buf = torch.full((int(floats),), float("nan"), device="cuda")
        self.blocks = 0

    def __enter__(self):
        _lib.check(L.flowse_op_stats_sink(_lib.ptr(self.buf), self.buf.numel()))
        return self

    def __exit__(self, *exc):
        self.blocks = int(L.flowse_op_stats_sink_blocks())
        _lib.check(L.flowse_op_stats_sink(None, 0))
        torch.cuda.synchronize()
        return False

    def partial(self, B, Cout):
        return self.buf[:B * self.blocks * Cout * 2].view(B, self.blocks, Cout, 2).cpu()

    def clean_beyond(self, B, Cout):
        return bool(torch.isnan(self.buf[B * self.blocks * Cout * 2:]).all())


def gn_stats(x1, nblk, x2=None, dt=0):
    """The stand-alone statistics kernel (flowse_op_gn_stats) on NCHW cpu tensors (rounded to dt inside: 1 = bf16, 2 = half):
    partial [B, nblk, C1 + C2, 2] on the cpu"""
    a1 = nhwc(x1)
    a2 = nhwc(x2) if x2 is not None else None
    B, H, W, C1 = a1.shape
    C2 = a2.shape[3] if a2 is not None else 0
    part = torch.full((B, nblk, C1 + C2, 2), float("nan"), device="cuda")
    scratch = torch.empty(2 * B * H * W * (C1 + C2) + 512, dtype=torch.uint8, device="cuda") if dt else None
    _lib.check(L.flowse_op_gn_stats(_lib.ptr(a1), C1, _lib.ptr(a2), C2, B, H * W, dt, _lib.ptr(scratch),
                                    scratch.numel() if dt else 0, _lib.ptr(part), nblk, stream()))
    torch.cuda.synchronize()
    return part.cpu()


def gn_finalize(p1, HW, G, gamma, p2=None, eps=1e-6, x1=None, x2=None, beta=None, silu=False):
    """flowse_op_gn_finalize on partial sets [B, nblk, C, 2] (cpu).  Without x1: (mean, scale) [B, C1 + C2] on the cpu; with
    x1 (x2), beta (NCHW cpu): the normalised tensor of the finalize + apply kernel, NCHW cpu."""
    d1 = p1.contiguous().cuda().float()
    d2 = p2.contiguous().cuda().float() if p2 is not None else None
    B, nblk1, C1, _ = d1.shape
    nblk2, C2 = (d2.shape[1], d2.shape[2]) if d2 is not None else (0, 0)
    g = gamma.contiguous().cuda().float()
    mean = scl = a1 = a2 = be = out = None
    if x1 is None:
        mean = torch.full((B, C1 + C2), float("nan"), device="cuda")
        scl = torch.full((B, C1 + C2), float("nan"), device="cuda")
    else:
        a1, a2 = nhwc(x1), nhwc(x2) if x2 is not None else None
        be = beta.contiguous().cuda().float()
        out = torch.full((B, a1.shape[1], a1.shape[2], C1 + C2), float("nan"), device="cuda")
    _lib.check(L.flowse_op_gn_finalize(_lib.ptr(d1), nblk1, C1, _lib.ptr(d2), nblk2, C2, B, HW, G, _lib.ptr(g), eps,
                                       _lib.ptr(mean), _lib.ptr(scl), _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(be), int(silu),
                                       _lib.ptr(out), stream()))
    torch.cuda.synchronize()
    return (mean.cpu(), scl.cpu()) if x1 is None else nchw(out)


def last_route():
    """which kernel the last convolution launch of this thread ran (flowse_op_last_conv_route)"""
    return L.flowse_op_last_conv_route().decode()


def conv2d_16(x1, w, dt, bias=None, x2=None, bias2=None, res=None, scale=1.0, out_f32=False, gn=None, silu=True):
    """The 16-bit storage op entry with per-sample bias and optional fp32 output (flowse_op_conv2d_16_ex; dt 1 = bf16,
    2 = half): fp32 NCHW cpu tensors in, rounded to dt inside; fp32 NCHW cpu out.  gn: (mean [B, C], scale [B, C],
    beta [C]) or None; silu: SiLU behind the fused GroupNorm."""
    Cout, Cin, k, _ = w.shape
    taps = k * k
    a1, a2, wp, bb, b2, rr = conv_operands(x1, x2, w, taps, bias, bias2, res)
    B, H, W, C1 = a1.shape
    C2 = a2.shape[3] if a2 is not None else 0
    mean, scl, beta = (t.contiguous().cuda() for t in gn) if gn is not None else (None, None, None)
    out = torch.empty(B, H, W, Cout, device="cuda")
    M = B * H * W
    ksmax = max(1, (Cin // 32 * taps + 1) // 4)            # K slices: at most half the two-step stages (flat16_ksplit)
    nbytes = 2 * (M * Cin + 2 * Cout * taps * Cin + 2 * M * Cout) + 4 * ksmax * M * Cout + 4096
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.flowse_op_conv2d_16_ex(_lib.ptr(a1), C1, _lib.ptr(a2), C2, _lib.ptr(wp), _lib.ptr(bb), _lib.ptr(b2),
                                        b2.shape[1] if b2 is not None else 0, _lib.ptr(rr), _lib.ptr(mean), _lib.ptr(scl),
                                        _lib.ptr(beta), int(silu), _lib.ptr(out), int(out_f32), B, H, W, Cout, taps, float(scale), dt,
                                        _lib.ptr(scratch), scratch.numel(), stream()))
    torch.cuda.synchronize()
    return nchw(out)


def resblock_tail_16(h, w1, dt, b1, x1, w2, b2, x2=None, gn=None, silu=True, scale=1.0):
    """Tail of a residual block in 16-bit storage as one launch (flowse_op_resblock_tail_16; dt 1 = bf16, 2 = half):
    (conv3x3(act(GN(h)); w1) + b1 + conv1x1(cat[x1, x2]; w2) + b2) * scale.  fp32 NCHW cpu tensors in, rounded to dt inside;
    fp32 NCHW cpu out.  w1 [Cout, C, 3, 3], w2 [Cout, X1 + X2, 1, 1]; gn: (mean [B, C], scale [B, C], beta [C]) or None."""
    Cout, Cc = w1.shape[:2]
    hd, a1 = nhwc(h), nhwc(x1)
    a2 = nhwc(x2) if x2 is not None else None
    B, H, W, X1 = a1.shape
    X2 = a2.shape[3] if a2 is not None else 0
    w1p = w1.permute(0, 2, 3, 1).reshape(Cout, 9, Cc).contiguous().cuda()
    w2p = w2.reshape(Cout, 1, X1 + X2).contiguous().cuda()
    b1d = b1.contiguous().cuda() if b1 is not None else None
    b2d = b2.contiguous().cuda() if b2 is not None else None
    mean, scl, beta = (t.contiguous().cuda() for t in gn) if gn is not None else (None, None, None)
    out = torch.empty(B, H, W, Cout, device="cuda")
    M = B * H * W
    up = lambda b: (b + 255) & ~255                       # the entry's own `need`
    nw1, nw2 = (Cout * 9 * Cc + 3) & ~3, (Cout * (X1 + X2) + 3) & ~3
    need = up(2 * M * Cc) + up(2 * M * X1) + up(2 * M * X2) + 2 * up(2 * nw1) + 2 * up(2 * nw2) + up(2 * M * Cout)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(L.flowse_op_resblock_tail_16(_lib.ptr(hd), Cc, _lib.ptr(mean), _lib.ptr(scl), _lib.ptr(beta), int(silu),
                                            _lib.ptr(w1p), _lib.ptr(b1d), _lib.ptr(a1), X1, _lib.ptr(a2), X2, _lib.ptr(w2p),
                                            _lib.ptr(b2d), _lib.ptr(out), B, H, W, Cout, float(scale), dt, _lib.ptr(scratch),
                                            scratch.numel(), stream()))
    torch.cuda.synchronize()
    return nchw(out)


def group_norm(x1, gamma, beta, x2=None, silu=True, eps=1e-6):
    a1 = nhwc(x1)
    a2 = nhwc(x2) if x2 is not None else None
    B, H, W, C1 = a1.shape
    C2 = a2.shape[3] if a2 is not None else 0
    n = L.flowse_op_group_norm_scratch_floats(B, H * W, C1 + C2)
    scratch = torch.empty(n, device="cuda")
    out = torch.empty(B, H, W, C1 + C2, device="cuda")
    g, b = gamma.cuda().contiguous(), beta.cuda().contiguous()
    _lib.check(L.flowse_op_group_norm(_lib.ptr(a1), C1, _lib.ptr(a2), C2, _lib.ptr(g), _lib.ptr(b), eps, int(silu),
                                      _lib.ptr(out), B, H, W, _lib.ptr(scratch), stream()))
    torch.cuda.synchronize()
    return nchw(out)


def fir(x, up):
    a = nhwc(x)
    B, H, W, Cc = a.shape
    out = torch.empty((B, 2 * H, 2 * W, Cc) if up else (B, H // 2, W // 2, Cc), device="cuda")
    fn = L.flowse_op_fir_up if up else L.flowse_op_fir_down
    _lib.check(fn(_lib.ptr(a), _lib.ptr(out), B, H, W, Cc, stream()))
    torch.cuda.synchronize()
    return nchw(out)


def upfirdn2d(x, kernel, up=1, down=1, pad=(0, 0)):
    N, Cc, H, W = x.shape
    kh, kw = kernel.shape
    oh = (H * up + pad[0] + pad[1] - kh) // down + 1
    ow = (W * up + pad[0] + pad[1] - kw) // down + 1
    a = x.contiguous().cuda().float()
    k = torch.as_tensor(kernel, dtype=torch.float32).contiguous().cuda()
    out = torch.empty(N, Cc, oh, ow, device="cuda")
    _lib.check(L.flowse_upfirdn2d(_lib.ptr(a), _lib.ptr(k), N * Cc, H, W, kh, kw, up, up, down, down, pad[0], pad[1],
                                  pad[0], pad[1], _lib.ptr(out), oh, ow, stream()))
    torch.cuda.synchronize()
    return out.cpu()


def attention(q, k, v):
    """q,k,v: [B, C, L] cpu -> [B, C, L] cpu"""
    B, Cc, Lt = q.shape
    qkv = torch.cat([q.permute(0, 2, 1), k.permute(0, 2, 1), v.permute(0, 2, 1)], dim=2).contiguous().cuda()
    out = torch.empty(B, Lt, Cc, device="cuda")
    _lib.check(L.flowse_op_attention(_lib.ptr(qkv), _lib.ptr(out), B, Lt, Cc, stream()))
    torch.cuda.synchronize()
    return out.permute(0, 2, 1).contiguous().cpu()


def attention16(q, k, v, dt):
    """The same through the 16-bit kernel (dt 1 = bf16, 2 = half): q, k, v are rounded to dt inside"""
    B, Cc, Lt = q.shape
    qkv = torch.cat([q.permute(0, 2, 1), k.permute(0, 2, 1), v.permute(0, 2, 1)], dim=2).contiguous().cuda()
    out = torch.empty(B, Lt, Cc, device="cuda")
    scratch = torch.empty(8 * B * Lt * Cc + 512, dtype=torch.uint8, device="cuda")
    _lib.check(L.flowse_op_attention_16(_lib.ptr(qkv), _lib.ptr(out), B, Lt, Cc, dt, _lib.ptr(scratch), scratch.numel(),
                                        stream()))
    torch.cuda.synchronize()
    return out.permute(0, 2, 1).contiguous().cpu()


def gfp(t, W):
    B, E = t.numel(), W.numel()
    td, Wd = t.cuda().contiguous(), W.cuda().contiguous()
    out = torch.empty(B, 2 * E, device="cuda")
    _lib.check(L.flowse_op_gfp(_lib.ptr(td), _lib.ptr(Wd), _lib.ptr(out), B, E, stream()))
    torch.cuda.synchronize()
    return out.cpu()


def staged_gn(scratch, B, HW, C):
    """The (mean, scale) [B, C] pair (cpu) that op_gn_prologue left in an entry's scratch: floats [n - 2BC, n - BC) and
    [n - BC, n) with n = flowse_op_group_norm_scratch_floats(B, HW, C) -- what the conv that followed normalised with."""
    n = L.flowse_op_group_norm_scratch_floats(B, HW, C)
    return scratch[n - 2 * B * C:n - B * C].view(B, C).cpu(), scratch[n - B * C:n].view(B, C).cpu()


def conv3x3_gn(x1, gamma, beta, w, bias=None, x2=None, bias2=None, res=None, scale=1.0, silu=True, eps=1e-6, staged=None):
    """(conv3x3(act(GN(cat[x1,x2]))) + bias + bias2 + res) * scale through the fused halo kernel.  staged: a list that
    receives the (mean, scale) pair the kernel normalised with (staged_gn)."""
    Cout, Cin, k, _ = w.shape
    a1, a2, wp, bb, b2, rr = conv_operands(x1, x2, w, 9, bias, bias2, res)
    B, H, W, C1 = a1.shape
    C2 = a2.shape[3] if a2 is not None else 0
    g, be = gamma.cuda().contiguous(), beta.cuda().contiguous()
    scratch = torch.empty(L.flowse_op_group_norm_scratch_floats(B, H * W, C1 + C2), device="cuda")
    out = torch.empty(B, H, W, Cout, device="cuda")
    _lib.check(L.flowse_op_conv3x3_gn(_lib.ptr(a1), C1, _lib.ptr(a2), C2, _lib.ptr(g), _lib.ptr(be), eps, int(silu),
                                      _lib.ptr(wp), _lib.ptr(bb), _lib.ptr(b2), b2.shape[1] if b2 is not None else 0,
                                      _lib.ptr(rr), _lib.ptr(out), B, H, W, Cout, float(scale), _lib.ptr(scratch),
                                      stream()))
    torch.cuda.synchronize()
    if staged is not None:
        staged.extend(staged_gn(scratch, B, H * W, C1 + C2))
    return nchw(out)


def conv3x3_f43(x1, w, gamma=None, beta=None, bias=None, x2=None, bias2=None, res=None, scale=1.0, silu=True,
                eps=1e-6, form="f43", staged=None):
    """Same contract as conv3x3_gn (gamma None: no normalisation; staged as there) through the F(4,3) Winograd kernel
    (form "f43") or the two-dimensional F(4,3) x F(2,3) kernel (form "w2d")."""
    Cout, Cin, k, _ = w.shape
    a1, a2, wp, bb, b2, rr = conv_operands(x1, x2, w, 9, bias, bias2, res)
    B, H, W, C1 = a1.shape
    C2 = a2.shape[3] if a2 is not None else 0
    g = gamma.cuda().contiguous() if gamma is not None else None
    be = beta.cuda().contiguous() if beta is not None else None
    scratch = torch.empty(getattr(L, f"flowse_op_conv3x3_{form}_scratch_floats")(B, H, W, C1 + C2, Cout), device="cuda")
    out = torch.empty(B, H, W, Cout, device="cuda")
    fn = getattr(L, f"flowse_op_conv3x3_{form}")
    _lib.check(fn(_lib.ptr(a1), C1, _lib.ptr(a2), C2, _lib.ptr(g), _lib.ptr(be), eps, int(silu),
                                       _lib.ptr(wp), _lib.ptr(bb), _lib.ptr(b2),
                                       b2.shape[1] if b2 is not None else 0, _lib.ptr(rr), _lib.ptr(out), B, H, W, Cout,
                                       float(scale), _lib.ptr(scratch), stream()))
    torch.cuda.synchronize()
    if staged is not None and gamma is not None:
        staged.extend(staged_gn(scratch, B, H * W, C1 + C2))
    return nchw(out)


def stft_compress(sig, scale=1.0, factor=0.15, exponent=0.5, pad_multiple=64):
    B, Ls = sig.shape
    T = Ls // 128 + 1
    Tpad = ((T + pad_multiple - 1) // pad_multiple) * pad_multiple
    a = sig.contiguous().cuda().float()
    out = torch.empty(B, 1, 256, Tpad, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_stft_compress(_lib.ptr(a), B, Ls, float(scale), _lib.ptr(out), T, Tpad, factor, exponent,
                                      stream()))
    torch.cuda.synchronize()
    return out.cpu(), T


def istft_decompress(spec, T, length, scale=1.0, factor=0.15, exponent=0.5):
    a = spec.contiguous().cuda()
    B, _, F, Tpad = a.shape
    out = torch.empty(B, length, device="cuda")
    _lib.check(L.flowse_istft_decompress(_lib.ptr(a), B, T, Tpad, factor, exponent, _lib.ptr(out), length,
                                         float(scale), stream()))
    torch.cuda.synchronize()
    return out.cpu()


class Block:
    """One reference module (ResnetBlockBigGANpp / AttnBlockpp / Combine) behind a single-module C-ABI handle."""
    KINDS = {"resnet": 0, "attn": 1, "combine": 2}

    def __init__(self, kind, in_ch, out_ch, up=False, down=False, temb_dim=64):
        from flowmse_amd.backbones.structure import handle_param_table
        self.h = C.c_void_p()
        _lib.check(L.flowse_block_create(self.KINDS[kind], in_ch, out_ch, int(up), int(down), temb_dim, C.byref(self.h)))
        self.names, self.shapes, self.offsets = handle_param_table(self.h)
        self.kind, self.out_ch, self.up, self.down = kind, out_ch, up, down

    def load(self, weights, precision="fp32"):
        """weights: {module-local reference key (e.g. 'Conv_0.weight'): tensor}; precision as NCSNpp.set_precision"""
        _lib.check(L.flowse_model_set_precision(self.h, {"fp32": 0, "bf16x3": 1, "bf16": 2, "fp16": 3}[precision]))
        blob = torch.zeros(int(L.flowse_model_blob_numel(self.h)))
        for n, shp, off in zip(self.names, self.shapes, self.offsets):
            w = weights[n[len("all_modules.0."):]].float()
            assert list(w.shape) == shp, (n, tuple(w.shape), shp)
            blob[off:off + w.numel()] = w.reshape(-1)
        _lib.check(L.flowse_model_load_weights(self.h, C.c_void_p(blob.data_ptr()), blob.numel()))
        return self

    def __call__(self, x1, x2=None, temb=None):
        """NCHW cpu tensors in, NCHW cpu out.  temb: raw time embedding [B, temb_dim] (SiLU applied here, as plumbing)."""
        a1 = nhwc(x1)
        a2 = nhwc(x2) if x2 is not None else None
        B, H, W, C1 = a1.shape
        ta = torch.nn.functional.silu(temb.float()).contiguous().cuda() if temb is not None else None
        Ho, Wo = (2 * H, 2 * W) if self.up else (H // 2, W // 2) if self.down else (H, W)
        out = torch.empty(B, Ho, Wo, self.out_ch, device="cuda")
        _lib.check(L.flowse_block_forward(self.h, _lib.ptr(a1), C1, _lib.ptr(a2), _lib.ptr(ta), _lib.ptr(out), B, H, W,
                                          stream()))
        torch.cuda.synchronize()
        return nchw(out)

    def __del__(self):
        try:
            if self.h:
                L.flowse_model_destroy(self.h)
                self.h = None
        except Exception:
            pass
