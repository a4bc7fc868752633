// Per-op entries of the C ABI (include/flowse_hip.h: flowse_upfirdn2d, flowse_op_*): single kernels and fused ops behind
// plain pointers, for the unit tests and for callers that build their own network.  No entry takes a flowse_model, and
// this file does not see the handle's types (no model.h).  No kernels here.
#include <algorithm>
#include <cstdio>
#include <string>

#include "../../include/flowse_hip.h"
#include "common.h"

namespace flowse {

// ------------------------------------------------------------------------------------- shared by the per-op test entries
// the fields every conv entry fills
static ConvArgs conv_args(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                          const float* bias2, int bias2_stride, const float* res, float* out, int B, int H, int W, int Cout,
                          int taps, float scale) {
    ConvArgs c;
    c.in1 = in1; c.in2 = in2; c.C1 = C1; c.C2 = C2;
    c.w = w; c.bias = bias; c.bias2 = bias2; c.bias2_stride = bias2_stride; c.res = res; c.out = out;
    c.B = B; c.H = H; c.W = W; c.Cout = Cout; c.taps = taps; c.scale = scale;
    return c;
}

// Statistics and finalize of GroupNorm over cat[in1, in2], in `scratch` as flowse_op_group_norm_scratch_floats sizes it:
// partials [B][nblk][C][2], mean [B][C], scale [B][C].  *gn: what the consumer normalises with.
static int op_gn_prologue(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta, float eps,
                          int B, int HW, float* scratch, hipStream_t s, GnParams* gn) {
    const int C = C1 + C2, nblk = gn_partial_blocks(HW, C);
    float* mean = scratch + (int64_t)B * nblk * C * 2;
    float* scl = mean + (int64_t)B * C;
    *gn = GnParams{mean, scl, beta};
    const int rc = launch_gn_stats(in1, C1, in2, C2, B, HW, scratch, nblk, s);
    if (rc != OK) return rc;
    return launch_gn_finalize(scratch, nblk, C, nullptr, 0, 0, B, HW, std::min(C / 4, 32), gamma, eps, mean, scl, s);
}

// The statistics sink (flowse_op_stats_sink): while armed, every per-op conv entry has its launch leave the fused GroupNorm
// partials of its output there -- a thread-local test hook in the style of conv_last_route.  op_sink_stats is called on the
// ConvArgs as they will be launched (weights, slab, GroupNorm input all set): the geometry is the route's of exactly those
// arguments, and a route that writes no statistics launches without.
static thread_local struct { float* buf; int64_t floats; int blocks; } g_sink = {nullptr, 0, 0};
static int op_sink_stats(ConvArgs& c, const char* entry, bool w2d_named = false) {
    if (!g_sink.buf) return OK;
    g_sink.blocks = 0;
    const ConvShape q{c.in_dt, c.out_dt, c.B, c.H, c.W, c.C1, c.C2, c.Cout, c.taps};
    if ((c.in2 == nullptr && c.C2 != 0) || conv_shape_check(q) != OK) return OK;      // launch_conv's error to report
    c.stats = g_sink.buf;
    const ConvRoute r = conv_route_of(c);
    // (flowse_op_conv3x3_w2d names its kernel whatever the policy would run: that kernel's 64-pixel strips)
    const int nblk = r.err != OK ? 0 : w2d_named ? c.H * c.W / 64 : r.stats_nblk;
    if (nblk <= 0) {
        c.stats = nullptr;
        return OK;
    }
    if ((int64_t)c.B * nblk * c.Cout * 2 > g_sink.floats) {
        set_error("%s: the statistics sink holds %lld floats, this launch writes %lld", entry, (long long)g_sink.floats,
                  (long long)c.B * nblk * c.Cout * 2);
        return ERR_ARG;
    }
    c.stats_nblk = g_sink.blocks = nblk;
    return OK;
}

// Copy k of conv_copy of c's weights (`w16`: their 16-bit twin, for the 16-bit copies), made at dst; c then points at it
static int op_make_copy(ConvArgs& c, int k, const void* w16, void* dst, hipStream_t s) {
    const int rc = conv_copy(k).make(c.w, w16, c.Cout, c.taps, c.C1 + c.C2, dst, s);
    if (rc == OK) conv_set_weight(c, k, dst);
    return rc;
}
// elements of the derived copies a route reads
static int64_t op_copies_numel(const ConvRoute& r, int Cout, int taps, int Cin) {
    int64_t n = 0;
    for (int k = 0; k < CW_COPIES; ++k)
        if (r.reads_weight(k)) n += conv_copy(k).numel(Cout, taps, Cin);
    return n;
}

// the caller's scratch of a 16-bit entry, handed out in sub-buffers rounded up to 256 bytes
struct Carver {
    char* p;
    static int64_t up(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
    void* take(int64_t bytes) {
        char* q = p;
        p += up(bytes);
        return q;
    }
};

}  // namespace flowse

using namespace flowse;

extern "C" {

int flowse_upfirdn2d(const float* input, const float* kernel, int planes, int in_h, int in_w, int kh, int kw, int up_x,
                     int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, float* out,
                     int out_h, int out_w, void* stream) {
    if (!input || !kernel || !out || pad_x0 < 0 || pad_x1 < 0 || pad_y0 < 0 || pad_y1 < 0) {
        set_error("flowse_upfirdn2d: bad argument (null pointer or negative pad)");
        return ERR_ARG;
    }
    return launch_upfirdn2d_nchw(input, kernel, planes, in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1,
                                 pad_y0, pad_y1, out, out_h, out_w, static_cast<hipStream_t>(stream));
}

// The route of an fp32 conv for a per-op entry whose scratch can hold what `o` names (a view of conv_route)
static ConvRoute op_route_f32(int B, int H, int W, int C1, int C2, int Cout, int taps, ConvOffer o) {
    return conv_route(ConvShape{DT_F32, DT_F32, B, H, W, C1, C2, Cout, taps}, o);
}
static ConvOffer op_offer_scratch() {            // flowse_op_conv2d's scratch: the fragment-order weight copy, or the slab
    ConvOffer o;
    o.wsm = o.slab = true;
    return o;
}
static ConvOffer op_offer_f43() {                // flowse_op_conv3x3_f43's scratch: the F(4,3) weights and the slab
    ConvOffer o;
    o.wino = o.slab = true;
    return o;
}

int64_t flowse_op_conv2d_scratch_floats(int B, int H, int W, int Cin, int Cout, int taps) {
    const ConvRoute r = op_route_f32(B, H, W, Cin, 0, Cout, taps, op_offer_scratch());
    // the fragment-order weight copy of a kernel that splits K inside the block, or the slab: never both
    return op_copies_numel(r, Cout, taps, Cin) + (r.ksplit > 1 ? (int64_t)r.ksplit * B * H * W * Cout : 0);
}

int flowse_op_conv2d(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                     const float* bias2, int bias2_stride, const float* res, float* out, int B, int H, int W, int Cout,
                     int taps, float scale, float* splitk_scratch, void* stream) {
    if (!in1 || !w || !out) {
        set_error("flowse_op_conv2d: null argument");
        return ERR_ARG;
    }
    ConvArgs c = conv_args(in1, C1, in2, in2 ? C2 : 0, w, bias, bias2, bias2_stride, res, out, B, H, W, Cout, taps, scale);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (splitk_scratch) {                            // the model handle's kernel for this shape
        const ConvRoute r = op_route_f32(B, H, W, c.C1, c.C2, Cout, taps, op_offer_scratch());
        c.ksplit = r.ksplit;
        c.partial = c.ksplit > 1 ? splitk_scratch : nullptr;
        for (int k = 0; k < CW_COPIES; ++k)           // (at most one: the offer names one fragment-order copy)
            if (r.reads_weight(k))
                if (const int rc = op_make_copy(c, k, nullptr, splitk_scratch, s)) return rc;
    }
    if (const int rc = op_sink_stats(c, "flowse_op_conv2d")) return rc;
    return launch_conv(c, s);
}

int64_t flowse_op_group_norm_scratch_floats(int B, int HW, int C) {
    const int nblk = gn_partial_blocks(HW, C);
    return (int64_t)B * nblk * C * 2 + 2 * (int64_t)B * C;
}

int flowse_op_group_norm(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                         float eps, int silu, float* out, int B, int H, int W, float* scratch, void* stream) {
    if (!in1 || !gamma || !beta || !out || !scratch) {
        set_error("flowse_op_group_norm: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!in2) C2 = 0;
    GnParams p;
    const int rc = op_gn_prologue(in1, C1, in2, C2, gamma, beta, eps, B, H * W, scratch, s, &p);
    if (rc != OK) return rc;
    return launch_gn_apply(in1, C1, in2, C2, B, H * W, p, silu, out, s);
}

int flowse_op_conv3x3_gn(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                         float eps, int silu, const float* w, const float* bias, const float* bias2, int bias2_stride,
                         const float* res, float* out, int B, int H, int W, int Cout, float scale, float* scratch,
                         void* stream) {
    if (!in1 || !gamma || !beta || !w || !out || !scratch) {
        set_error("flowse_op_conv3x3_gn: null argument");
        return ERR_ARG;
    }
    if (!in2) C2 = 0;
    if (!op_route_f32(B, H, W, C1, C2, Cout, 9, ConvOffer()).gn_on_load) {
        set_error("flowse_op_conv3x3_gn: shape B=%d H=%d W=%d C=%d+%d Cout=%d not covered by the halo kernel", B, H, W,
                  C1, C2, Cout);
        return ERR_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    ConvArgs c = conv_args(in1, C1, in2, C2, w, bias, bias2, bias2_stride, res, out, B, H, W, Cout, 9, scale);
    c.gn_silu = silu;
    int rc = op_gn_prologue(in1, C1, in2, C2, gamma, beta, eps, B, H * W, scratch, s, &c.gn);
    if (rc == OK) rc = op_sink_stats(c, "flowse_op_conv3x3_gn");
    return rc != OK ? rc : launch_conv(c, s);
}

static int op_conv3x3_winograd(const float* in1, int C1, const float* in2, int C2, const float* gamma,
                               const float* beta, float eps, int silu, const float* w, const float* bias,
                               const float* bias2, int bias2_stride, const float* res, float* out, int B, int H, int W,
                               int Cout, float scale, float* scratch, void* stream, bool two_d = false) {
    if (!in1 || !w || !out || !scratch || (gamma && !beta)) {
        set_error("flowse_op_conv3x3_%s: null argument", two_d ? "w2d" : "f43");
        return ERR_ARG;
    }
    if (!in2) C2 = 0;
    const ConvRoute r = op_route_f32(B, H, W, C1, C2, Cout, 9, op_offer_f43());
    const int copy = two_d ? CW_WINO2 : CW_WINO;        // the entry names its kernel, and so the copy it reads
    if (two_d ? !conv_w2d_shape_ok(B, H, W, C1, C2, Cout, 9) : !r.reads_weight(copy)) {
        set_error("flowse_op_conv3x3_%s: shape B=%d H=%d W=%d C=%d+%d Cout=%d not covered by the Winograd kernel",
                  two_d ? "w2d" : "f43", B, H, W, C1, C2, Cout);
        return ERR_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = C1 + C2, HW = H * W;
    float* wf = scratch + flowse_op_group_norm_scratch_floats(B, HW, C);
    ConvArgs c = conv_args(in1, C1, in2, C2, w, bias, bias2, bias2_stride, res, out, B, H, W, Cout, 9, scale);
    int rc = op_make_copy(c, copy, nullptr, wf, s);
    if (rc != OK) return rc;
    const int ks = two_d ? 1 : r.ksplit;
    if (ks > 1) {                           // same split plan as the model handle uses for this shape
        c.ksplit = ks;
        c.partial = wf + conv_copy(CW_WINO).numel(Cout, 9, C);
    }
    if (gamma) {
        c.gn_silu = silu;
        rc = op_gn_prologue(in1, C1, in2, C2, gamma, beta, eps, B, HW, scratch, s, &c.gn);
        if (rc != OK) return rc;
    }
    rc = op_sink_stats(c, two_d ? "flowse_op_conv3x3_w2d" : "flowse_op_conv3x3_f43", two_d);
    if (rc != OK) return rc;
    // the 2-D entry names its kernel: every shape conv_w2d_shape_ok admits runs it (launch_conv's policy would hand images of
    // up to 2048 pixels to another kernel, or refuse their fused GroupNorm input)
    return two_d ? launch_w2d(c, s) : launch_conv(c, s);
}

int64_t flowse_op_conv3x3_f43_scratch_floats(int B, int H, int W, int C, int Cout) {
    const int ks = op_route_f32(B, H, W, C, 0, Cout, 9, op_offer_f43()).ksplit;   // > 1: F(4,3) runs split over K (small images)
    return flowse_op_group_norm_scratch_floats(B, H * W, C) + conv_copy(CW_WINO).numel(Cout, 9, C) +
           (ks > 1 ? (int64_t)ks * B * H * W * Cout : 0);
}

int64_t flowse_op_conv3x3_w2d_scratch_floats(int B, int H, int W, int C, int Cout) {
    return flowse_op_group_norm_scratch_floats(B, H * W, C) + conv_copy(CW_WINO2).numel(Cout, 9, C);
}

int flowse_op_conv3x3_w2d(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                          float eps, int silu, const float* w, const float* bias, const float* bias2, int bias2_stride,
                          const float* res, float* out, int B, int H, int W, int Cout, float scale, float* scratch,
                          void* stream) {
    return op_conv3x3_winograd(in1, C1, in2, C2, gamma, beta, eps, silu, w, bias, bias2, bias2_stride, res, out, B, H,
                               W, Cout, scale, scratch, stream, true);
}

int flowse_op_conv3x3_f43(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                          float eps, int silu, const float* w, const float* bias, const float* bias2, int bias2_stride,
                          const float* res, float* out, int B, int H, int W, int Cout, float scale, float* scratch,
                          void* stream) {
    return op_conv3x3_winograd(in1, C1, in2, C2, gamma, beta, eps, silu, w, bias, bias2, bias2_stride, res, out, B, H,
                               W, Cout, scale, scratch, stream);
}

// 16-bit storage per-op entry: fp32 NHWC tensors at the boundary, rounded to bf16 (dt 1) / half (dt 2) inside, conv on
// the 16-bit matrix cores (LDS-halo kernel when it applies, else the flat kernel), result widened back.  Optional fused
// GroupNorm(+SiLU) on the input (halo shapes only) from caller-supplied per-(sample, channel) mean / scale and beta.
// (bias2 / out_f32: the additions of flowse_op_conv2d_16_ex; out_f32 = `res` and `out` are fp32 tensors the conv reads and
// writes directly, out_dt = DT_F32, as the model does for the few convs that leave the 16-bit domain)
static int op_conv2d_16(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                        const float* bias2, int bias2_stride, const float* res, const float* gn_mean, const float* gn_scale,
                        const float* gn_beta, int silu, float* out, int out_f32, int B, int H, int W, int Cout, int taps,
                        float scale, int dt, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!in1 || !w || !out || !scratch || (dt != DT_BF16 && dt != DT_F16) || (taps != 1 && taps != 9)) {
        set_error("flowse_op_conv2d_16: bad argument");
        return ERR_ARG;
    }
    if (!in2) C2 = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t M = (int64_t)B * H * W, C = C1 + C2;
    // the progressive-output heads (C -> 4, ncsnpp.py:345-366): 16-bit input, fp32 residual (the pyramid) and fp32 output, as
    // in the model -- conv3x3_head4_16_kernel
    const bool head = Cout == 4 && taps == 9 && !in2 && conv_supports_head4(B, H, W, C1, 0, Cout, taps);
    const bool direct = head || out_f32;                   // fp32 res / out, used in place
    // (the LDS-halo kernels store the operands' type only: an fp32-output launch of their shapes runs the flat kernel)
    ConvOffer offer;                                       // the scratch holds the 16-bit weights, their fragment-order copy, the slab
    offer.wq = offer.wfrag = offer.slab = true;
    offer.terms = 1;
    offer.wq_f16 = dt == DT_F16;
    offer.bias2 = bias2 != nullptr;
    const ConvRoute r = conv_route(ConvShape{dt, direct ? DT_F32 : dt, B, H, W, C1, C2, Cout, taps}, offer);
    const int ks = r.ksplit;
    const int64_t nw = ((int64_t)Cout * taps * C + 3) & ~(int64_t)3;
    // the carver's round-up per sub-buffer, upper bound over the optional ones
    const auto up = Carver::up;
    const int64_t need = up(2 * M * C1) + up(2 * M * C2) + 2 * up(2 * nw) + 2 * up(2 * M * Cout) +
                         (ks > 1 ? up(4 * (int64_t)ks * M * Cout) : 0);
    if (scratch_bytes < need) {
        set_error("flowse_op_conv2d_16: scratch needs %lld bytes", (long long)need);
        return ERR_ARG;
    }
    if (gn_mean && !r.gn_on_load) {
        set_error("flowse_op_conv2d_16: fused GroupNorm input only on LDS-halo shapes");
        return ERR_SHAPE;
    }
    Carver cv{static_cast<char*>(scratch)};
    void* a1 = cv.take(2 * M * C1);
    void* a2 = C2 ? cv.take(2 * M * C2) : nullptr;
    void* wq = cv.take(2 * nw);
    void* wfrag = r.reads_weight(CW_WFRAG) ? cv.take(2 * nw) : nullptr;
    void* r16 = res && !direct ? cv.take(2 * M * Cout) : nullptr;
    void* o16 = direct ? nullptr : cv.take(2 * M * Cout);
    float* part = ks > 1 ? static_cast<float*>(cv.take(4 * (int64_t)ks * M * Cout)) : nullptr;
    if ((size_t)(cv.p - static_cast<char*>(scratch)) > (size_t)scratch_bytes) {
        set_error("flowse_op_conv2d_16: scratch too small");
        return ERR_ARG;
    }
    ConvArgs c = conv_args(static_cast<const float*>(a1), C1, static_cast<const float*>(a2), C2, w, bias, bias2,
                           bias2 ? bias2_stride : 0, static_cast<const float*>(r16), static_cast<float*>(o16), B, H, W, Cout,
                           taps, scale);
    int rc = launch_convert(in1, DT_F32, a1, dt, M * C1, s);
    if (rc == OK && C2) rc = launch_convert(in2, DT_F32, a2, dt, M * C2, s);
    if (rc == OK && r.reads_weight(CW_WQ)) {
        rc = launch_convert(w, DT_F32, wq, dt, nw, s);
        conv_set_weight(c, CW_WQ, wq);
    }
    if (rc == OK && wfrag) rc = op_make_copy(c, CW_WFRAG, wq, wfrag, s);
    if (rc == OK && r16) rc = launch_convert(res, DT_F32, r16, dt, M * Cout, s);
    if (rc != OK) return rc;
    c.ksplit = ks; c.partial = part;
    c.terms = 1; c.wq_f16 = dt == DT_F16 ? 1 : 0;
    c.in_dt = dt; c.out_dt = dt;
    if (gn_mean) {
        c.gn = GnParams{gn_mean, gn_scale, gn_beta};
        c.gn_silu = silu;
    }
    if (direct) {
        c.res = res;
        c.out = out;
        c.out_dt = DT_F32;
    }
    rc = op_sink_stats(c, "flowse_op_conv2d_16");
    if (rc == OK) rc = launch_conv(c, s);
    if (rc != OK || direct) return rc;
    return launch_convert(o16, dt, out, DT_F32, M * Cout, s);
}

int flowse_op_conv2d_16(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                        const float* res, const float* gn_mean, const float* gn_scale, const float* gn_beta, int silu,
                        float* out, int B, int H, int W, int Cout, int taps, float scale, int dt, void* scratch,
                        int64_t scratch_bytes, void* stream) {
    return op_conv2d_16(in1, C1, in2, C2, w, bias, nullptr, 0, res, gn_mean, gn_scale, gn_beta, silu, out, 0, B, H, W, Cout,
                        taps, scale, dt, scratch, scratch_bytes, stream);
}

int flowse_op_conv2d_16_ex(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                           const float* bias2, int bias2_stride, const float* res, const float* gn_mean,
                           const float* gn_scale, const float* gn_beta, int silu, float* out, int out_f32, int B, int H,
                           int W, int Cout, int taps, float scale, int dt, void* scratch, int64_t scratch_bytes,
                           void* stream) {
    if (bias2 && (bias2_stride < Cout || (bias2_stride & 3))) {
        set_error("flowse_op_conv2d_16_ex: bias2_stride must be a multiple of 4 and at least Cout");
        return ERR_ARG;
    }
    return op_conv2d_16(in1, C1, in2, C2, w, bias, bias2, bias2_stride, res, gn_mean, gn_scale, gn_beta, silu, out,
                        out_f32 != 0, B, H, W, Cout, taps, scale, dt, scratch, scratch_bytes, stream);
}

const char* flowse_op_last_conv_route(void) { return conv_last_route(); }

int flowse_op_conv_route(int in_dt, int out_dt, int B, int H, int W, int C1, int C2, int Cout, int taps, int offer_bits,
                         char* text, int cap) {
    // (fp32 in, 16-bit out: the convs of the 4-channel input in the 16-bit storage modes)
    const bool in4_out16 = in_dt == DT_F32 && C1 == 4 && C2 == 0 && (out_dt == DT_BF16 || out_dt == DT_F16);
    if (!text || cap < 64 || in_dt < DT_F32 || in_dt > DT_F16 || (out_dt != DT_F32 && out_dt != in_dt && !in4_out16) || B < 1 || H < 1 || W < 1) {
        set_error("flowse_op_conv_route: bad argument");
        return ERR_ARG;
    }
    const ConvShape q{in_dt, out_dt, B, H, W, C1, C2, Cout, taps};
    ConvOffer o;
    o.wino = offer_bits & FLOWSE_OFFER_WINO; o.wino2 = offer_bits & FLOWSE_OFFER_WINO2; o.wsm = offer_bits & FLOWSE_OFFER_WSM;
    o.wfrag = offer_bits & FLOWSE_OFFER_WFRAG; o.wq = offer_bits & FLOWSE_OFFER_WQ;
    o.terms = !o.wq ? 0 : (offer_bits & FLOWSE_OFFER_WQ_SPLIT3) ? 3 : 1;
    o.wq_f16 = offer_bits & FLOWSE_OFFER_WQ_F16;
    o.slab = offer_bits & FLOWSE_OFFER_SLAB; o.gn = offer_bits & FLOWSE_OFFER_GN; o.bias2 = offer_bits & FLOWSE_OFFER_BIAS2;
    o.stats = offer_bits & FLOWSE_OFFER_STATS; o.fold = offer_bits & FLOWSE_OFFER_FOLD;
    int err = conv_shape_check(q);
    ConvRoute r;
    if (err == OK) {
        r = conv_route(q, o);
        if ((err = r.err) != OK) set_error("%s", r.err_text);
    }
    if (err != OK) {
        snprintf(text, cap, "error %d", err);
        return OK;
    }
    const char* issued = r.issued == 0.5 ? "1/2" : r.issued == 3.0 ? "3" : r.issued == 1.0 ? "1" : "1/3";
    std::string reads;                                   // "wq+wfrag", "wino", ... in ConvWeight order, wq first; "-": none
    for (int k : {(int)CW_WQ, (int)CW_WINO, (int)CW_WINO2, (int)CW_WSM, (int)CW_WSM16, (int)CW_WFRAG})
        if (r.reads_weight(k)) reads += (reads.empty() ? "" : "+") + std::string(k == CW_WQ ? "wq" : conv_copy(k).name);
    snprintf(text, cap, "%s ks=%d reduce=%d stats=%d gn=%d issued=%s reads=%s", conv_kernel_name(r.kernel), r.ksplit,
             r.reduce ? 1 : 0, r.stats_nblk, r.gn_on_load ? 1 : 0, issued, reads.empty() ? "-" : reads.c_str());
    return OK;
}

// Tail of ResnetBlockBigGANpp in 16-bit storage as ONE launch of the producer / consumer kernel:
//   out = (conv3x3(act(GroupNorm(h)); w1) + b1 + conv1x1(cat[x1, x2]; w2) + b2) * scale       (layerspp.py:265-274)
// with the shortcut as extra K steps (ConvArgs::sc1).  fp32 tensors at the boundary as in flowse_op_conv2d_16.
int flowse_op_resblock_tail_16(const float* h, int C, const float* gn_mean, const float* gn_scale, const float* gn_beta,
                               int silu, const float* w1, const float* b1, const float* x1, int XC1, const float* x2,
                               int XC2, const float* w2, const float* b2, float* out, int B, int H, int W, int Cout,
                               float scale, int dt, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!h || !w1 || !x1 || !w2 || !out || !scratch || (dt != DT_BF16 && dt != DT_F16)) {
        set_error("flowse_op_resblock_tail_16: bad argument");
        return ERR_ARG;
    }
    if (!x2) XC2 = 0;
    if (!conv16_uses_pc(B, H, W, C, 0, Cout, 9)) {
        set_error("flowse_op_resblock_tail_16: only shapes conv3x3_pc16_kernel takes (H, W multiples of 16, C %% 32 == 0, "
                  "Cout %% 128 == 0, >= 64 tile x channel-block items)");
        return ERR_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t M = (int64_t)B * H * W, XC = (int64_t)XC1 + XC2;
    const int64_t nw1 = ((int64_t)Cout * 9 * C + 3) & ~(int64_t)3, nw2 = ((int64_t)Cout * XC + 3) & ~(int64_t)3;
    const auto up = Carver::up;
    const int64_t need = up(2 * M * C) + up(2 * M * XC1) + up(2 * M * XC2) + 2 * up(2 * nw1) + 2 * up(2 * nw2) + up(2 * M * Cout);
    if (scratch_bytes < need) {
        set_error("flowse_op_resblock_tail_16: scratch needs %lld bytes", (long long)need);
        return ERR_ARG;
    }
    Carver cv{static_cast<char*>(scratch)};
    void* h16 = cv.take(2 * M * C);
    void* a1 = cv.take(2 * M * XC1);
    void* a2 = XC2 ? cv.take(2 * M * XC2) : nullptr;
    void* wq1 = cv.take(2 * nw1);
    void* wf1 = cv.take(2 * nw1);
    void* wq2 = cv.take(2 * nw2);
    void* wf2 = cv.take(2 * nw2);
    void* o16 = cv.take(2 * M * Cout);
    int rc = launch_convert(h, DT_F32, h16, dt, M * C, s);
    if (rc == OK) rc = launch_convert(x1, DT_F32, a1, dt, M * XC1, s);
    if (rc == OK && XC2) rc = launch_convert(x2, DT_F32, a2, dt, M * XC2, s);
    if (rc == OK) rc = launch_convert(w1, DT_F32, wq1, dt, nw1, s);
    if (rc == OK) rc = launch_convert(w2, DT_F32, wq2, dt, nw2, s);
    if (rc == OK) rc = launch_pc16_weights(wq1, Cout, C, wf1, s, 9);
    if (rc == OK) rc = launch_pc16_weights(wq2, Cout, (int)XC, wf2, s, 1);
    if (rc != OK) return rc;
    ConvArgs c = conv_args(static_cast<const float*>(h16), C, nullptr, 0, w1, b1, nullptr, 0, nullptr,
                           static_cast<float*>(o16), B, H, W, Cout, 9, scale);
    c.bias_x = b2;
    c.wq = wq1; c.terms = 1; c.wq_f16 = dt == DT_F16 ? 1 : 0;
    c.wfrag = wf1;
    c.sc1 = a1; c.SC1 = XC1; c.sc2 = a2; c.SC2 = XC2; c.wfrag_sc = wf2;
    c.in_dt = dt; c.out_dt = dt;
    if (gn_mean) {
        c.gn = GnParams{gn_mean, gn_scale, gn_beta};
        c.gn_silu = silu;
    }
    rc = op_sink_stats(c, "flowse_op_resblock_tail_16");
    if (rc == OK) rc = launch_conv(c, s);
    if (rc != OK) return rc;
    return launch_convert(o16, dt, out, DT_F32, M * Cout, s);
}

int flowse_op_stats_sink(float* buf, int64_t floats) {
    if ((buf == nullptr) != (floats <= 0)) {
        set_error("flowse_op_stats_sink: a buffer and its size in floats, or (null, 0) to disarm");
        return ERR_ARG;
    }
    g_sink = {buf, buf ? floats : 0, 0};
    return OK;
}
int flowse_op_stats_sink_blocks(void) { return g_sink.blocks; }

int flowse_op_gn_stats(const float* in1, int C1, const float* in2, int C2, int B, int HW, int dt, void* scratch,
                       int64_t scratch_bytes, float* partial, int nblk, void* stream) {
    if (!in1 || !partial || nblk < 1 || B < 1 || HW < 1 || dt < DT_F32 || dt > DT_F16 || (dt != DT_F32 && !scratch)) {
        set_error("flowse_op_gn_stats: bad argument");
        return ERR_ARG;
    }
    if (!in2) C2 = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == DT_F32) return launch_gn_stats(in1, C1, in2, C2, B, HW, partial, nblk, s);
    const int64_t M = (int64_t)B * HW;
    if ((C1 & 3) || (C2 & 3) || scratch_bytes < Carver::up(2 * M * C1) + Carver::up(2 * M * C2)) {
        set_error("flowse_op_gn_stats: channel counts must be multiples of 4 and scratch hold both inputs in 16 bits");
        return ERR_ARG;
    }
    Carver cv{static_cast<char*>(scratch)};
    void* a1 = cv.take(2 * M * C1);
    void* a2 = C2 ? cv.take(2 * M * C2) : nullptr;
    int rc = launch_convert(in1, DT_F32, a1, dt, M * C1, s);
    if (rc == OK && C2) rc = launch_convert(in2, DT_F32, a2, dt, M * C2, s);
    if (rc != OK) return rc;
    return launch_gn_stats(a1, C1, a2, C2, B, HW, partial, nblk, s, dt);
}

int flowse_op_gn_finalize(const float* p1, int nblk1, int C1, const float* p2, int nblk2, int C2, int B, int HW, int G,
                          const float* gamma, float eps, float* mean, float* scale, const float* in1, const float* in2,
                          const float* beta, int silu, float* out, void* stream) {
    if (!p1 || !gamma || nblk1 < 1 || B < 1 || HW < 1 || G < 1 || (out ? !in1 || !beta : !mean || !scale)) {
        set_error("flowse_op_gn_finalize: bad argument");
        return ERR_ARG;
    }
    if (!p2) { C2 = 0; nblk2 = 0; }
    if (C2 > 0 && nblk2 < 1) {
        set_error("flowse_op_gn_finalize: the second set needs its block count");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (out) return launch_gn_finalize_apply(in1, p1, nblk1, C1, in2, p2, nblk2, C2, B, HW, G, gamma, beta, eps, silu, out, s);
    return launch_gn_finalize(p1, nblk1, C1, p2, nblk2, C2, B, HW, G, gamma, eps, mean, scale, s);
}

int flowse_op_pc16_channel_blocks(int mode) {
    pc16_set_channel_blocks(mode);
    return OK;
}

int flowse_op_fir_up(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    GnParams p{nullptr, nullptr, nullptr};
    return launch_fir_up(in, B, H, W, C, p, 0, nullptr, out, static_cast<hipStream_t>(stream));
}
int flowse_op_fir_down(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    GnParams p{nullptr, nullptr, nullptr};
    return launch_fir_down(in, B, H, W, C, p, 0, out, static_cast<hipStream_t>(stream));
}
int flowse_op_attention(const float* qkv, float* out, int B, int L, int C, void* stream) {
    return launch_attention(qkv, B, L, C, out, static_cast<hipStream_t>(stream));
}
// 16-bit attention core: the fp32 tokens rounded to bf16 (dt 1) / half (dt 2) in scratch, attention16_kernel, result widened
int flowse_op_attention_16(const float* qkv, float* out, int B, int L, int C, int dt, void* scratch, int64_t scratch_bytes,
                           void* stream) {
    if (!qkv || !out || !scratch || (dt != DT_BF16 && dt != DT_F16) || B < 1 || L < 1 || C < 1) {
        set_error("flowse_op_attention_16: bad argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * L * C;
    const int64_t need = Carver::up(2 * 3 * n) + Carver::up(2 * n);
    if (scratch_bytes < need) {
        set_error("flowse_op_attention_16: scratch needs %lld bytes", (long long)need);
        return ERR_ARG;
    }
    Carver cv{static_cast<char*>(scratch)};
    void* q16 = cv.take(2 * 3 * n);
    void* o16 = cv.take(2 * n);
    int rc = launch_convert(qkv, DT_F32, q16, dt, 3 * n, s);
    if (rc == OK) rc = launch_attention(q16, B, L, C, o16, s, dt);
    if (rc != OK) return rc;
    return launch_convert(o16, dt, out, DT_F32, n, s);
}
int flowse_op_gfp(const float* t, const float* W, float* out, int B, int E, void* stream) {
    return launch_gfp(t, W, B, E, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
