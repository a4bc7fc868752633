// Dispatch and shape policies of the convolution entry point launch_conv (common.h).
//
//   out[m][n] = ( sum_{tap, ci} A[m][tap, ci] * Wp[n][tap][ci] + bias[n] + bias2[b(m)][n] + res[m][n] ) * scale
//   m = NHWC pixel (b, y, x), n = output channel, K = taps * Cin with the channel axis contiguous in both operands.
//
// Kernel families (one translation unit each):
//   conv_f43.hip      fp32 F(4,3) Winograd 3x3 (production kernel of the fp32 mode)
//   conv_w2d.hip      fp32 F(4,3) x F(2,3) two-dimensional Winograd 3x3 (large images, whole K)
//   conv_halo.hip     direct fp32 LDS-halo 3x3, 4-channel heads; the convs of a 4-channel input (input layer, Combine 1x1):
//                     routed here like every other family, by shape (fp32 input, C1 = 4, C2 = 0), always whole K
//   conv_flat.hip     flat fp32 kernels: 1x1, small 3x3, split-K slices
//   conv_smallm.hip   fp32 convs on <= 2048 pixels: K split inside the block (no slab, no reduction launch)
//   conv_1x1.hip      fp32 1x1 on large images: every wave its own GEMM, operands straight into fragment registers
//   conv_reduce.hip   second pass of split-K launches (+ fused GroupNorm statistics / GroupNorm)
//   conv16.hip        16-bit operand / storage modes
// Replaces (reference): ddpm_conv3x3 / ddpm_conv1x1 (flowmse/backbones/ncsnpp_utils/layers.py:100-124), NIN (:546-555).
#include <cstdio>

#include "conv_smallm.h"

namespace flowse {

// test hooks, read once: FLOWSE_FORCE_GENERIC_CONV=1 routes every shape through the generic gather kernel,
// FLOWSE_NO_HALO_CONV=1 through the flat kernels, FLOWSE_NO_WINOGRAD=1 runs the direct (bitwise fmaf-chain) 3x3 kernel
static const bool g_force_generic = getenv("FLOWSE_FORCE_GENERIC_CONV") != nullptr;
static const bool g_no_halo = getenv("FLOWSE_NO_HALO_CONV") != nullptr;
static const bool g_no_wino = getenv("FLOWSE_NO_WINOGRAD") != nullptr;
static const bool g_no_wino_policy = g_no_wino || g_no_halo || g_force_generic;
// FLOWSE_W2D=0 keeps the 1-D F(4,3) kernel everywhere (A-B hook); default: the 2-D kernel where w2d_wanted says so
static const bool g_w2d = !(getenv("FLOWSE_W2D") && getenv("FLOWSE_W2D")[0] == '0');
static bool conv_w2d_enabled() { return g_w2d && !g_no_wino_policy; }
// FLOWSE_NO_SMALLM=1: small images run the split-K flat / F(4,3) kernels + reduction launches of rounds 1-4 (A-B hook)
static const bool g_no_smallm = getenv("FLOWSE_NO_SMALLM") != nullptr;
static const int g_smallm_max = getenv("FLOWSE_SMALLM_MAX") ? atoi(getenv("FLOWSE_SMALLM_MAX")) : 2048;
bool conv_smallm_ok(int B, int H, int W, int C1, int C2, int Cout, int taps) {
    // (2048 pixels = 16 x 16 at batch 8: 4.96 vs 5.76 ms for the level against the sliced F(4,3) kernel + reduction launches,
    // A-B-A-B on one box; FLOWSE_SMALLM_MAX moves the limit)
    return !g_no_smallm && !g_force_generic && sm_shape_ok(B, H, W, C1, C2, Cout, taps, g_smallm_max, 4);
}
bool conv_force_generic() { return g_force_generic; }

// Images with at most 64 pixels in the whole batch (one utterance at the 8x8 and 4x4 levels): a 128-row tile would spend
// 50-87 % of its MFMAs on padding rows and every K step costs 64 MFMAs per wave whatever M is.  They run 32-row tiles
// (4 waves side by side along N, 16 MFMAs per wave and step) and are sliced along K accordingly.
bool conv_small_m(int64_t M, int Cout) { return M <= 64 && Cout > 64; }

// ------------------------------------------------------------------------------------- the derived weight copies
// One entry per copy (ConvCopy, common.h): which convs get it, how large it is, what makes it.  The model handle uploads
// exactly what the rules name (flowse_model_load_weights), offers it (Builder::offer) and the route below -- which names
// in ConvRoute::reads the copies its kernel reads -- only ever chooses among what was offered.
static int64_t numel_packed(int Cout, int taps, int Cin) { return (int64_t)Cout * taps * Cin; }
static int64_t numel_f43(int Cout, int, int Cin) { return (int64_t)Cout * 18 * Cin; }      // 18 transformed taps per channel pair
static int64_t numel_w2d(int Cout, int, int Cin) { return (int64_t)Cout * 24 * Cin; }      // 24
static bool fits(int64_t numel, int esize) { return numel * esize < (1LL << 31); }         // one 32-bit buffer descriptor
static bool aligned(int Cout, int Cin, int cout_step) { return Cin > 0 && (Cin % KC) == 0 && (Cout % cout_step) == 0; }
static bool gets_wino(int Cout, int taps, int Cin, int act_dt) {
    return act_dt == DT_F32 && taps == 9 && aligned(Cout, Cin, 64) && fits(numel_f43(Cout, 9, Cin), 4);
}
static bool gets_wino2(int Cout, int taps, int Cin, int act_dt) {
    return gets_wino(Cout, taps, Cin, act_dt) && conv_w2d_enabled() && fits(numel_w2d(Cout, 9, Cin), 4);
}
// both fragment orders of the small-image kernels; the attention projections are 1x1 convs and get them too
static bool gets_wsm(int Cout, int taps, int Cin, int act_dt) {
    return act_dt == DT_F32 && !g_no_smallm && !g_force_generic && aligned(Cout, Cin, 32) && fits(numel_packed(Cout, taps, Cin), 4);
}
// 16-bit storage: the 3x3 convs of the producer / consumer kernel, and whatever the 16-bit small-image kernel can take
static bool gets_wfrag(int Cout, int taps, int Cin, int act_dt) {
    return act_dt != DT_F32 && fits(numel_packed(Cout, taps, Cin), 2) &&
           ((taps == 9 && aligned(Cout, Cin, 128)) || (conv16_smallm_enabled() && aligned(Cout, Cin, 32)));
}
const ConvCopy& conv_copy(int k) {
    static const ConvCopy table[CW_COPIES] = {
        {"wino", 4, false, gets_wino, numel_f43,
         [](const float* w, const void*, int Cout, int, int Cin, void* out, hipStream_t s) {
             return launch_f43_weights(w, Cout, Cin, static_cast<float*>(out), s);
         }},
        {"wino2", 4, false, gets_wino2, numel_w2d,
         [](const float* w, const void*, int Cout, int, int Cin, void* out, hipStream_t s) {
             return launch_w2d_weights(w, Cout, Cin, static_cast<float*>(out), s);
         }},
        {"wsm", 4, true, gets_wsm, numel_packed,
         [](const float* w, const void*, int Cout, int taps, int Cin, void* out, hipStream_t s) {
             return launch_smallm_weights(w, Cout, taps, Cin, static_cast<float*>(out), s, false);
         }},
        {"wsm16", 4, true, gets_wsm, numel_packed,
         [](const float* w, const void*, int Cout, int taps, int Cin, void* out, hipStream_t s) {
             return launch_smallm_weights(w, Cout, taps, Cin, static_cast<float*>(out), s, true);
         }},
        {"wfrag", 2, true, gets_wfrag, numel_packed,
         [](const float*, const void* w16, int Cout, int taps, int Cin, void* out, hipStream_t s) {
             return launch_pc16_weights(w16, Cout, Cin, out, s, taps);
         }},
    };
    return table[k];
}

// The two-dimensional Winograd form: whole-K launches on images that give every CU at least two blocks of 16 x 16 pixels x
// 64 channels, or one of 32 channels (below that the 1-D kernel's K slices fill the chip better).
static const int g_w2d_min_blocks = getenv("FLOWSE_W2D_MIN_BLOCKS") ? atoi(getenv("FLOWSE_W2D_MIN_BLOCKS")) : 128;
bool conv_w2d_shape_ok(int B, int H, int W, int C1, int C2, int Cout, int taps) {
    if (g_no_wino_policy || taps != 9 || (H & 15) || (W & 15) || (C1 % KC) || (C2 % KC) || (Cout % 64) || B < 1) return false;
    const int64_t cmax = C1 > C2 ? C1 : C2;
    return fits(numel_w2d(Cout, 9, C1 + C2), 4) && ((int64_t)H * W + 2 * W + 2) * cmax * 4 < (1LL << 31);
}

// ------------------------------------------------------------------------------------------- the policy, fp32 storage
// Everything below answers "what will run" and is asked by conv_route alone; "can this kernel run this shape" lives
// with the kernels (conv_supports_head4, conv_cin4_kernel_of, conv_smallm_ok, conv1x1_stream_ok, conv_w2d_shape_ok,
// conv16_uses_halo / _pc, conv16_smallm_ok).
struct Fp32Policy {
    int ksplit;       // K slices a slab would be cut into (1 = whole K)
    int f43;          // 0: not an F(4,3) shape (or too small even when sliced), 1: whole K, >= 2: that many slices of chunks
    bool halo;        // a whole-K launch runs one of the LDS-halo 3x3 kernels (the ones that can normalise on load)
    bool wino;        // ... the F(4,3) kernel, given its weights (whole K, or the f43 slices)
    bool w2d;         // ... the 2-D kernel, given its weights
};

// F(4,3) plan of a 3x3 shape.  The Winograd kernels tile N by 64, so 256 (pixel tile, channel block) pairs -- one per CU --
// already beat slicing K; below that, K is cut until ~512 blocks exist while every slice keeps at least two chunks.  Only
// the F(4,3) kernel knows how to run a slice.
static int f43_plan(int B, int H, int W, int Cin, int Cout, int taps) {
    if (g_no_wino_policy || taps != 9 || (H & 7) || (W & 15) || (Cin % KC) || (Cout % 64)) return 0;
    const int64_t blocks = ((int64_t)B * H * W / 128) * (Cout / 64);
    if (blocks >= 256) return 1;                      // (round 4 sweep: 128 / 512 / 1024 all lose at B = 1, 4, 8: profiles/r04_policy_sweep.md)
    const int nchunks = Cin / KC;
    if (blocks < 16 || nchunks < 4) return 0;
    int64_t ks = (512 + blocks - 1) / blocks;
    if (ks > nchunks / 2) ks = nchunks / 2;
    const int per = (int)((nchunks + ks - 1) / ks);
    ks = (nchunks + per - 1) / per;                   // every slice non-empty
    return ks >= 2 ? (int)ks : 0;
}

// at least one block per CU: of 64 channels, or -- 128..255 such blocks -- of 32 channels (conv3x3_w2d_kernel<GN, 1>)
static bool w2d_wanted(int B, int H, int W, int C1, int C2, int Cout, int taps) {
    return conv_w2d_enabled() && conv_w2d_shape_ok(B, H, W, C1, C2, Cout, taps) &&
           ((int64_t)B * H * W / 256) * (Cout / 64) >= g_w2d_min_blocks;
}

// Split-K: images so small that the 128x128 tiling yields < 256 blocks (one per CU) are sliced along K until ~512 blocks
// exist, keeping >= 4 K steps per slice; a deterministic second launch (conv_reduce.hip) sums the slices.
// (The in-launch reduction by the last-arriving slice was built in round 2 and measured slower -- 137.4 vs 122.7 ms per
// step at [8,1,256,256], 44.5 vs 33.4 ms at [1,1,256,256]: the last slice of a tile pulls ks x 64 KB through ONE CU's L1
// after its own K loop, while the two-pass kernel spreads the same bytes over every CU; removed in round 4.)
// The head, small-image and 2-D kernels are judged by the TOTAL channel count here: a concat whose parts are not 32-aligned (not
// in the released net) runs the flat kernel unsplit.
static int fp32_ksplit(const ConvShape& q, int f43) {
    const int B = q.B, H = q.H, W = q.W, Cin = q.C1 + q.C2, Cout = q.Cout, taps = q.taps;
    if (conv_supports_head4(B, H, W, Cin, 0, Cout, taps)) return 1;     // 4-channel heads: dedicated kernel
    if (conv_smallm_ok(B, H, W, Cin, 0, Cout, taps)) return 1;          // K is split inside the block
    if (w2d_wanted(B, H, W, Cin, 0, Cout, taps)) return 1;              // whole K on the 2-D Winograd kernel
    const int64_t M = (int64_t)B * H * W;
    const int bn = Cout <= 32 ? 32 : Cout <= 64 ? 64 : 128;       // N tile the flat launcher picks for this width
    const int bm = conv_small_m(M, Cout) ? 32 : 128;              // M tile (single utterances at the 8x8 / 4x4 levels: 32 rows)
    const int64_t tiles = ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn);
    const int steps = ((Cin + KC - 1) / KC) * taps;
    if (tiles >= 256 || steps < 8) return 1;          // measured: 256 beats 128 and 64 at B = 1..8
    if (f43 >= 1) return f43;
    int64_t want = (512 + tiles - 1) / tiles;
    int64_t maxs = steps / 4;                         // (>= 4 K steps per slice: 2 and 1 lose, same sweep)
    int64_t ks = want < maxs ? want : maxs;
    if (ks < 1) ks = 1;
    const int per = (int)((steps + ks - 1) / ks);     // make every slice non-empty
    return (int)((steps + per - 1) / per);
}

static Fp32Policy fp32_policy(const ConvShape& q, bool head4) {
    const int B = q.B, H = q.H, W = q.W, C1 = q.C1, C2 = q.C2, Cin = C1 + C2, Cout = q.Cout, taps = q.taps;
    const int64_t cmax = C1 > C2 ? C1 : C2;
    Fp32Policy p;
    p.f43 = f43_plan(B, H, W, Cin, Cout, taps);
    p.ksplit = fp32_ksplit(q, p.f43);
    p.halo = head4 || (!g_no_halo && !g_force_generic && !conv_smallm_ok(B, H, W, C1, C2, Cout, taps) &&   // (takes a materialised input)
                       taps == 9 && !(H & 7) && !(W & 15) && !(C1 % KC) && !(C2 % KC) && !(Cout & 3) &&
                       (p.ksplit == 1 || p.ksplit == p.f43) &&                                             // only the Winograd kernel runs split
                       (int64_t)(9 * W + 18) * cmax * 4 < (1LL << 31) && (int64_t)Cout * 9 * Cin * 4 < (1LL << 31));
    p.wino = !g_no_wino && p.halo && p.f43 >= 1 && gets_wino(Cout, taps, Cin, DT_F32) &&
             // the F(4,3) kernel addresses a whole sample through one buffer descriptor per source tensor
             ((int64_t)H * W + 2 * W + 2) * cmax * 4 < (1LL << 31);
    p.w2d = p.halo && w2d_wanted(B, H, W, C1, C2, Cout, taps);
    return p;
}

// 16-bit storage: the flat kernel's own split (no Winograd alternative, two K steps per stage, >= 2 stages per slice, until
// ~512 blocks exist)
static int flat16_ksplit(const ConvShape& q) {
    const int Cin = q.C1 + q.C2;
    if (conv16_smallm_ok(q.B, q.H, q.W, Cin, 0, q.Cout, q.taps)) return 1;        // K is split inside the block (conv16_smallm.hip)
    const int64_t M = (int64_t)q.B * q.H * q.W;
    const int64_t tiles = ((M + 127) / 128) * ((q.Cout + 127) / 128);
    const int stages = ((Cin / KC) * q.taps + 1) / 2;
    if (tiles >= 256 || stages < 4) return 1;
    int64_t ks = (512 + tiles - 1) / tiles;           // (swept in round 4: 128 ... 1024 blocks, 2 / 4 stages per slice: flat,
    if (ks > stages / 2) ks = stages / 2;             //  profiles/r04_policy_sweep.md)
    if (ks < 1) ks = 1;
    const int per = (int)((stages + ks - 1) / ks);
    return (int)((stages + per - 1) / per);
}

static thread_local char g_route[48] = "";
void conv_note_route(const char* a, const char* b, const char* c) { snprintf(g_route, sizeof g_route, "%s%s%s", a, b, c); }
const char* conv_last_route() { return g_route; }


// ---------------------------------------------------------------------------------------------------------- the route
const char* conv_kernel_name(ConvKernel k) {
    static const char* const names[] = {"head4", "head4_16", "smallm", "1x1_stream", "w2d", "f43", "f43_splitk", "halo",
                                        "halo_bf16x3", "halo16", "pc16", "smallm16b", "flat", "flat_splitk", "flat16",
                                        "flat16_splitk", "cin4", "cin4_stats", "cin4_mfma", "none"};
    return names[k];
}

// Statistics blocks per sample of the kernel that runs (of its reduction launch, for the split forms): 0 = none
static int route_stats_blocks(ConvKernel k, const ConvShape& q) {
    const int HW = q.H * q.W;
    if (q.Cout & 3) return 0;
    switch (k) {
        case CK_HEAD4: case CK_HEAD4_16: case CK_CIN4: case CK_NONE: return 0;
        case CK_CIN4_STATS: return conv_cin4_stats_blocks(q.B, q.H, q.W, q.Cout);
        case CK_SMALLM: return conv_smallm_stats_blocks(q.B, q.H, q.W);
        case CK_SMALLM16B: return conv16_smallm_stats_blocks(q.B, q.H, q.W);
        case CK_1X1_STREAM: return conv1x1_stream_stats_blocks(q.B, q.H, q.W);
        case CK_W2D: return HW / 64;                       // 4 x 16 pixel strips
        case CK_F43_SPLITK: case CK_FLAT_SPLITK: case CK_FLAT16_SPLITK: {      // the reduction writes them
            const int PB = sk_pixels_per_block(HW);
            return ((HW % PB) == 0 && q.Cout / 4 <= 256) ? HW / PB : 0;
        }
        default: return (HW % 128) == 0 ? HW / 128 : 0;    // one block per 128-pixel tile
    }
}

static bool route_gn_on_load(ConvKernel k) {
    switch (k) {
        case CK_HEAD4: case CK_HEAD4_16: case CK_W2D: case CK_F43: case CK_F43_SPLITK: case CK_HALO: case CK_HALO_BF16X3:
        case CK_HALO16: case CK_PC16: return true;
        default: return false;
    }
}

// The weight pointers the kernel dereferences next to the packed `w` (ConvRoute::reads)
static unsigned route_reads(ConvKernel k, const ConvShape& q) {
    switch (k) {
        case CK_F43: case CK_F43_SPLITK: return 1u << CW_WINO;
        case CK_W2D: return 1u << CW_WINO2;
        case CK_1X1_STREAM: return 1u << CW_WSM;
        case CK_SMALLM: return 1u << (conv_smallm_tile16(q.B, q.H, q.W) ? CW_WSM16 : CW_WSM);
        case CK_HALO_BF16X3: case CK_HALO16: case CK_FLAT16: case CK_FLAT16_SPLITK: return 1u << CW_WQ;
        case CK_PC16: case CK_SMALLM16B: return 1u << CW_WQ | 1u << CW_WFRAG;
        default: return 0;                               // (head4_16 reads the fp32 `w`)
    }
}

ConvRoute conv_route(const ConvShape& q, const ConvOffer& o) {
    const int B = q.B, H = q.H, W = q.W, C1 = q.C1, C2 = q.C2, Cout = q.Cout, taps = q.taps;
    const bool in16 = q.in_dt != DT_F32;
    // a 4-channel fp32 input (the input layer, the Combine 1x1): its own kernels, whole K whatever is offered
    const bool cin4 = !in16 && C1 == 4 && C2 == 0;
    const bool head4 = conv_supports_head4(B, H, W, C1, C2, Cout, taps);
    // (the LDS-halo kernels store the operands' type only: an fp32-output launch of their shapes runs the flat kernel)
    const bool halo16 = in16 && q.out_dt == q.in_dt && conv16_uses_halo(B, H, W, C1, C2, Cout, taps);
    const Fp32Policy p = in16 || cin4 ? Fp32Policy{1, 0, false, false, false} : fp32_policy(q, head4);
    ConvRoute r;
    if (o.slab && !cin4) r.ksplit = !in16 ? p.ksplit : (head4 || halo16) ? 1 : flat16_ksplit(q);
    const int ks = r.ksplit;
    // the F(4,3) weights count half the nominal FLOPs for every conv that could run on them -- also where the bf16 planes
    // take the launch in the end (the plans have always been counted so)
    const bool wino = o.wino && p.wino;
    auto fail = [&](int err, const char* text) {
        r.kernel = CK_NONE;
        r.reads = 0;
        r.err = err;
        r.err_text = text;
        return r;
    };
    auto run = [&](ConvKernel k) {
        r.kernel = k;
        r.reduce = ks > 1;
        r.stats_nblk = route_stats_blocks(k, q);
        r.gn_on_load = route_gn_on_load(k);
        r.reads = route_reads(k, q);
        r.issued = k == CK_W2D ? 1.0 / 3.0 : wino ? 0.5 : k == CK_HALO_BF16X3 ? 3.0 : 1.0;
        if (o.gn && !r.gn_on_load) return fail(ERR_ARG, "conv: fused GroupNorm input requested for a shape the halo kernel does not cover");
        return r;
    };
    if (o.fold) {                                       // folded 1x1 shortcut: the producer / consumer kernel only
        if (!in16 || ks > 1 || q.out_dt != q.in_dt || !o.wfrag || !conv16_uses_pc(B, H, W, C1, C2, Cout, taps))
            return fail(ERR_ARG, "conv: a folded shortcut needs a launch of conv3x3_pc16_kernel (16-bit storage, 16 x 16-pixel tiles)");
        return run(CK_PC16);
    }
    if (cin4) {                                         // (none of these normalises on load: a gn request is run()'s error)
        const ConvKernel k = conv_cin4_kernel_of(q, o.stats);
        if (k != CK_NONE) return run(k);
        run(CK_FLAT);          // shapes the three refuse: only the flat kernel, whole K and without statistics, has ever run them
        r.stats_nblk = 0;
        return r;
    }
    if (in16) {                                        // activations stored as bf16 / half
        if (ks <= 1 && !o.bias2 && !o.stats && q.out_dt == DT_F32 && head4) return run(conv_head4_widens() ? CK_HEAD4 : CK_HEAD4_16);
        if (ks <= 1 && halo16) return run(o.wfrag && conv16_uses_pc(B, H, W, C1, C2, Cout, taps) ? CK_PC16 : CK_HALO16);
        if (o.wfrag && ks <= 1 && !o.gn && (q.out_dt == q.in_dt || q.out_dt == DT_F32) && conv16_smallm_ok(B, H, W, C1, C2, Cout, taps))
            return run(CK_SMALLM16B);
        return run(ks > 1 ? CK_FLAT16_SPLITK : CK_FLAT16);
    }
    if (ks <= 1 && !o.bias2 && !o.stats && head4) return run(CK_HEAD4);
    if (o.wsm && ks <= 1 && !o.gn && q.out_dt == DT_F32 && conv_smallm_ok(B, H, W, C1, C2, Cout, taps)) return run(CK_SMALLM);
    if (o.wsm && ks <= 1 && !o.gn && q.out_dt == DT_F32 && conv1x1_stream_ok(B, H, W, C1, C2, Cout, taps)) return run(CK_1X1_STREAM);
    if (ks <= 1 && p.halo) {
        if (o.wq && (Cout % 128) == 0) {
            if (o.terms == 3 && !o.wq_f16) return run(CK_HALO_BF16X3);
            if (o.terms == 1) return run(CK_HALO16);
            return fail(ERR_ARG, "conv: 16-bit path needs terms = 1 (bf16 / f16) or 3 (bf16 only)");
        }
        if (o.wino2 && p.w2d) return run(CK_W2D);
        return run(wino ? CK_F43 : CK_HALO);
    }
    if (ks > 1 && wino && ks == p.f43) return run(CK_F43_SPLITK);      // slices of chunks, raw partial tiles
    return run(ks > 1 ? CK_FLAT_SPLITK : CK_FLAT);
}

int launch_conv_routed(const ConvArgs& a, const ConvRoute& r, hipStream_t s, bool with_reduce) {
    if (r.err != OK) {
        set_error("%s", r.err_text);
        return r.err;
    }
    int rc = OK;
    switch (r.kernel) {
        case CK_HEAD4: case CK_HEAD4_16: return launch_head4(a, s);
        case CK_SMALLM: return launch_smallm(a, s);
        case CK_1X1_STREAM: return launch_1x1_stream(a, s);
        case CK_W2D:
            if (a.stats && a.stats_nblk != a.H * a.W / 64) {
                set_error("conv: the 2-D Winograd kernel writes its statistics in blocks of 64 pixels (stats_nblk=%d)", a.stats_nblk);
                return ERR_ARG;
            }
            return launch_w2d(a, s);
        case CK_F43: return launch_f43(a, s);
        case CK_HALO: return launch_halo_fp32(a, s);
        case CK_HALO_BF16X3: return launch_halo_bf16x3(a, s);
        case CK_HALO16: return launch_halo16_any(a, s);
        case CK_PC16: return launch_pc16(a, s);
        case CK_SMALLM16B: return launch_smallm16b(a, s);
        case CK_FLAT: return launch_flat_fp32(a, s);
        case CK_FLAT16: return launch_flat16(a, s);
        case CK_CIN4: case CK_CIN4_STATS: case CK_CIN4_MFMA: return launch_cin4(a, r.kernel, s);
        case CK_F43_SPLITK: rc = launch_f43(a, s); break;
        case CK_FLAT_SPLITK: rc = launch_flat_fp32(a, s); break;
        case CK_FLAT16_SPLITK: rc = launch_flat16(a, s); break;
        case CK_NONE:
            set_error("internal: conv launch without a route");
            return ERR_STATE;
    }
    if (rc != OK || !with_reduce) return rc;
    return launch_splitk_reduce(a, s);
}

// the part of launch_conv's argument checks that the shape alone decides
int conv_shape_check(const ConvShape& q) {
    if ((q.C1 & 3) || (q.C2 & 3) || (q.Cout & 3) || (q.taps != 1 && q.taps != 9) || q.C1 <= 0) {
        set_error("conv: unsupported channel counts C1=%d C2=%d taps=%d", q.C1, q.C2, q.taps);
        return ERR_SHAPE;
    }
    if ((int64_t)q.B * q.H * q.W >= (1LL << 31) / 4) {
        set_error("conv: too many pixels for 32-bit pixel indices");
        return ERR_SHAPE;
    }
    return OK;
}

// What a hand-filled ConvArgs offers -- the pointers it carries -- and the route of that: launch_conv's own derivation, shared
// with a caller that needs the answer before the launch (the statistics sink of the per-op entries)
ConvRoute conv_route_of(const ConvArgs& a) {
    const ConvShape q{a.in_dt, a.out_dt, a.B, a.H, a.W, a.C1, a.C2, a.Cout, a.taps};
    ConvOffer o;
    o.wino = a.wino != nullptr; o.wino2 = a.wino2 != nullptr; o.wsm = a.wsm != nullptr || a.wsm16 != nullptr; o.wfrag = a.wfrag != nullptr;
    o.wq = a.wq != nullptr; o.terms = a.terms; o.wq_f16 = a.wq_f16 != 0;
    o.slab = a.partial != nullptr;
    o.gn = a.gn.mean != nullptr;
    o.bias2 = a.bias2 != nullptr; o.stats = a.stats != nullptr;
    o.fold = a.sc1 || a.sc2 || a.wfrag_sc;
    return conv_route(q, o);
}

int launch_conv(const ConvArgs& a, hipStream_t s, bool with_reduce) {
    const ConvShape q{a.in_dt, a.out_dt, a.B, a.H, a.W, a.C1, a.C2, a.Cout, a.taps};
    if ((a.bias2 && (a.bias2_stride & 3)) || (a.in2 == nullptr && a.C2 != 0)) {
        set_error("conv: unsupported channel counts C1=%d C2=%d taps=%d", a.C1, a.C2, a.taps);
        return ERR_SHAPE;
    }
    if (const int rc = conv_shape_check(q)) return rc;
    if (a.ksplit > 1 && !a.partial) {
        set_error("conv: split-K needs a partial buffer");
        return ERR_ARG;
    }
    const ConvRoute r = conv_route_of(a);
    if (r.err == OK && r.ksplit != (a.ksplit > 1 ? a.ksplit : 1)) {     // the slab was sized for another split
        set_error("conv: ksplit=%d, this shape runs over %d K slices", a.ksplit, r.ksplit);
        return ERR_ARG;
    }
    return launch_conv_routed(a, r, s, with_reduce);
}

}  // namespace flowse
