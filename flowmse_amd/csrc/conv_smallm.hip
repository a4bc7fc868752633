// Replaces (reference): ddpm_conv3x3 / ddpm_conv1x1 (flowmse/backbones/ncsnpp_utils/layers.py:100-124) and NIN (:546-555) on
// the SMALL images of the network (ncsnpp.py:289-330, 335-385 at the 16 x 16 ... 4 x 4 levels; 32 x 32 for a single
// utterance): at most 2048 pixels in the whole batch.  The register ring, the operand window and the output stage are shared
// with the 16-bit twin: conv_smallm.h.
#include "conv_smallm.h"

namespace flowse {

// ---------------------------------------------------------------------------------------------------
// Small-M implicit GEMM with the K split INSIDE the block.
//
// With M = B H W <= 2048 pixels a 128 x 128 tiling has at most 16 tiles, so rounds 1-4 sliced K over extra blocks: every
// slice wrote a raw fp32 partial tile ([ksplit][M][Cout] slab: 33 MB for a 2 MB result at 16 x 16, batch 8) and a second
// launch read the slabs back, summed them and ran the epilogue -- 40 us per convolution against an MFMA floor of 8-15.
// Here a block owns a 32-pixel x (32 or 64)-channel output tile (256 blocks at 2048 pixels x 256 channels: one per CU)
// and its EIGHT waves each take every eighth K step (tap, 32-channel chunk): a wave requests its own operands straight
// into MFMA fragment registers -- A: 16 bytes per lane from the lane's pixel through a window descriptor (conv zero
// padding = an out-of-range offset, hardware returns 0), B: weights kept a second time in fragment order (one contiguous
// 1 KB line per wave-level request) -- through a branch-free register ring (ring_run), ahead of the MFMAs that consume them;
// no LDS, no barrier in the K loop.  The eight partial accumulator tiles meet once in LDS ([wave][32][BN + 4]) and one pass
// (sm_finish) sums them in a fixed order, runs the epilogue and leaves the GroupNorm partial statistics of what it stored
// (per block of min(32, H W) pixels and channel: mean, M2).  No slab, no second launch.
template <int NT2>
__global__ __launch_bounds__(512, 2) void conv_smallm_kernel(ConvArgs a) {
    constexpr int BN = 32 * NT2, CROW = BN + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [8][32][CROW]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const int W = a.W, HW = a.H * W, M = a.B * HW;
    const int C1 = a.C1, C2 = a.C2, Cin = C1 + C2;
    const int taps = a.taps, nchunks = Cin / KC, S_all = nchunks * taps;
    const int n_ntiles = a.Cout / BN;
    const int mt = blockIdx.x / n_ntiles, nt = blockIdx.x - mt * n_ntiles;
    const int m0 = mt * SM_BM, n0 = nt * BN;
    const SmWindow<float, SM_BM> win(a, m0, M, li, kh * 4);
    // weights in fragment order: [Cout/32][tap][chunk][k-block 4][lane 64][4 floats]
    const __amdgpu_buffer_rsrc_t rsrcw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wsm), 0, a.Cout * taps * Cin * 4, 0x00020000);
    const unsigned bvo = (unsigned)lane * 16u;
    // Register ring, D steps deep: a step is only 16 NT2 MFMAs (0.5-0.9 us) while its operands come from L2 -- or, for the
    // weights of a 4 x 4 image that few blocks share, straight from HBM -- so D - 1 steps of requests stay in flight.
    constexpr int D = NT2 == 1 ? 4 : 2;
    u32x4 ra[D][4], rb[D][NT2][4];
    auto gload = [&](int s, auto ring) {
        constexpr int R = decltype(ring)::value;
        const bool live = s < S_all;                          // steps past the end: clamped addresses, A reads as zero
        s = live ? s : S_all - 1;
        const int chunk = s / taps, tap = s - chunk * taps;
        int shift = W + 1;                                    // window origin is pixel m0 - W - 1
        if (taps == 9) shift += (tap / 3 - 1) * W + (tap - (tap / 3) * 3 - 1);
        const int c0 = chunk * KC;
        const bool second = c0 >= C1;
        const unsigned soff_a = (unsigned)(second ? shift * C2 + (c0 - C1) : shift * C1 + c0) * 4u;
        const bool ok = live && ((win.tapmask >> tap) & 1u);
        const unsigned vo = ok ? (second ? win.avo2 : win.avo1) : OOB;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            ra[R][j] = second ? __builtin_amdgcn_raw_buffer_load_b128(win.rsrc2, vo + j * 32, soff_a, 0)
                              : __builtin_amdgcn_raw_buffer_load_b128(win.rsrc1, vo + j * 32, soff_a, 0);
#pragma unroll
        for (int t = 0; t < NT2; ++t) {
            const unsigned soff_b = (unsigned)((((n0 >> 5) + t) * taps + tap) * nchunks + chunk) * 4096u;
#pragma unroll
            for (int j = 0; j < 4; ++j) rb[R][t][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrcw, bvo + j * 1024, soff_b, 0);
        }
    };
    f32x16 acc[NT2];
#pragma unroll
    for (int t = 0; t < NT2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    auto compute = [&](auto ring) {
        constexpr int R = decltype(ring)::value;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NT2; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(ra[R][j].x), __uint_as_float(rb[R][t][j].x), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(ra[R][j].y), __uint_as_float(rb[R][t][j].y), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(ra[R][j].z), __uint_as_float(rb[R][t][j].z), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(ra[R][j].w), __uint_as_float(rb[R][t][j].w), acc[t], 0, 0, 0);
            }
    };
    // wave w walks steps w, w + 8, ... (the last one masked for the waves that have one fewer)
    ring_run<D, 8>((S_all + 7) >> 3, wave, gload, compute);

    // ---- the eight partial tiles meet in LDS: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 kh
    float* Cw = smem + wave * (SM_BM * CROW);
#pragma unroll
    for (int t = 0; t < NT2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Cw[((r & 3) + 8 * (r >> 2) + 4 * kh) * CROW + t * 32 + li] = acc[t][r];
    sm_finish<SM_BM, BN, float>(a, smem, m0, n0, M, HW);
}

// ---------------------------------------------------------------------------------------------------
// The same scheme on 16 x 16 output tiles (v_mfma_f32_16x16x4_f32) for at most 256 pixels: a 32 x 32 tile of a 4 x 4 image
// (batch 8: 128 pixels -> 32 blocks; one utterance: 16 pixels -> 8 blocks, half of every tile padding) leaves 7/8 of the
// chip idle while each block grinds through the whole K on one CU (8 us of MFMA time whatever M is).  16 x 16 tiles give
// four times the blocks at a quarter of the MFMA work each.  Fragment layout of a 32-channel chunk: lane (row or column
// l & 15, k group l >> 4) holds channels 8 (l >> 4) .. + 7 as two float4 (MFMA e of the step uses element e of both
// operands); weights are kept a third time in that order ([Cout/16][tap][chunk][half][lane][4]).
__global__ __launch_bounds__(512, 2) void conv_smallm16_kernel(ConvArgs a) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr int BM = 16, BN = 16, CROW = BN + 4;
    __shared__ __attribute__((aligned(16))) float Cs[8 * BM * CROW];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int W = a.W, HW = a.H * W, M = a.B * HW;
    const int C1 = a.C1, C2 = a.C2, Cin = C1 + C2;
    const int taps = a.taps, nchunks = Cin / KC, S_all = nchunks * taps;
    const int n_ntiles = a.Cout / BN;
    const int mt = blockIdx.x / n_ntiles, nt = blockIdx.x - mt * n_ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const SmWindow<float, BM> win(a, m0, M, li, kq * 8);
    const __amdgpu_buffer_rsrc_t rsrcw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wsm16), 0, a.Cout * taps * Cin * 4, 0x00020000);
    const unsigned bvo = (unsigned)lane * 16u;
    // With 16-256 pixels there are only 16-256 blocks and each conv's weights come from HBM once: a wave keeps SEVEN of
    // its 9-18 steps in flight (16 registers per step) -- two latency rounds instead of five.
    constexpr int D = 8;
    u32x4 ra[D][2], rb[D][2];
    auto gload = [&](int s, auto ring) {
        constexpr int R = decltype(ring)::value;
        const bool live = s < S_all;                          // steps past the end: clamped addresses, A reads as zero
        s = live ? s : S_all - 1;
        const int chunk = s / taps, tap = s - chunk * taps;
        int shift = W + 1;                                    // window origin is pixel m0 - W - 1
        if (taps == 9) shift += (tap / 3 - 1) * W + (tap - (tap / 3) * 3 - 1);
        const int c0 = chunk * KC;
        const bool second = c0 >= C1;
        const unsigned soff_a = (unsigned)(second ? shift * C2 + (c0 - C1) : shift * C1 + c0) * 4u;
        const bool ok = live && ((win.tapmask >> tap) & 1u);
        const unsigned vo = ok ? (second ? win.avo2 : win.avo1) : OOB;
        const unsigned soff_b = (unsigned)(((n0 >> 4) * taps + tap) * nchunks + chunk) * 2048u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ra[R][h] = second ? __builtin_amdgcn_raw_buffer_load_b128(win.rsrc2, vo + h * 16, soff_a, 0)
                              : __builtin_amdgcn_raw_buffer_load_b128(win.rsrc1, vo + h * 16, soff_a, 0);
            rb[R][h] = __builtin_amdgcn_raw_buffer_load_b128(rsrcw, bvo + h * 1024, soff_b, 0);
        }
    };
    // two accumulators in turn (a dependent 16x16x4 MFMA waits 40 cycles, an independent one issues after 32)
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    auto compute = [&](auto ring) {
        constexpr int R = decltype(ring)::value;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][0].x), __uint_as_float(rb[R][0].x), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][1].x), __uint_as_float(rb[R][1].x), acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][0].y), __uint_as_float(rb[R][0].y), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][1].y), __uint_as_float(rb[R][1].y), acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][0].z), __uint_as_float(rb[R][0].z), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][1].z), __uint_as_float(rb[R][1].z), acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][0].w), __uint_as_float(rb[R][0].w), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ra[R][1].w), __uint_as_float(rb[R][1].w), acc1, 0, 0, 0);
    };
    ring_run<D, 8>((S_all + 7) >> 3, wave, gload, compute);

    // C/D layout of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + r
    float* Cw = Cs + wave * (BM * CROW);
#pragma unroll
    for (int r = 0; r < 4; ++r) Cw[(4 * kq + r) * CROW + li] = acc0[r] + acc1[r];
    // statistics block = the tile's 16 pixels (one sample: the launch guarantees H W % 16 == 0)
    sm_finish<BM, BN, float, BM>(a, Cs, m0, n0, M, HW);
}

// [Cout][taps][Cin] -> [Cout/16][tap][Cin/32][half][lane][4]: lane = (n & 15) + 16 (k group), k group = (ci & 31) >> 3
__global__ __launch_bounds__(256) void smallm16_weights_kernel(const float* __restrict__ w, int Cout, int taps, int Cin,
                                                               float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (n, tap, ci)
    if (idx >= (int64_t)Cout * taps * Cin) return;
    const int ci = (int)(idx % Cin);
    const int tap = (int)((idx / Cin) % taps);
    const int64_t n = idx / ((int64_t)taps * Cin);
    const int nchunks = Cin >> 5;
    const int chunk = ci >> 5, kq = (ci >> 3) & 3, h = (ci >> 2) & 1, e = ci & 3;
    const int lane = kq * 16 + (int)(n & 15);
    out[(((((n >> 4) * taps + tap) * nchunks + chunk) * 2 + h) * 64 + lane) * 4 + e] = w[idx];
}

// [Cout][taps][Cin] -> fragment order [Cout/32][tap][Cin/32][k-block j][lane][4]
__global__ __launch_bounds__(256) void smallm_weights_kernel(const float* __restrict__ w, int Cout, int taps, int Cin,
                                                             float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (n, tap, ci)
    if (idx >= (int64_t)Cout * taps * Cin) return;
    const int ci = (int)(idx % Cin);
    const int tap = (int)((idx / Cin) % taps);
    const int64_t n = idx / ((int64_t)taps * Cin);
    const int nchunks = Cin >> 5;
    const int chunk = ci >> 5, j = (ci >> 3) & 3, kh = (ci >> 2) & 1, e = ci & 3;
    const int lane = kh * 32 + (int)(n & 31);
    out[(((((n >> 5) * taps + tap) * nchunks + chunk) * 4 + j) * 64 + lane) * 4 + e] = w[idx];
}

int launch_smallm_weights(const float* w_packed, int Cout, int taps, int Cin, float* out, hipStream_t s, bool tile16) {
    if ((Cout % 32) != 0 || (Cin % 32) != 0) {
        set_error("smallm_weights: Cout=%d Cin=%d must be multiples of 32", Cout, Cin);
        return ERR_SHAPE;
    }
    const int64_t n = (int64_t)Cout * taps * Cin;
    if (tile16)
        hipLaunchKernelGGL(smallm16_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_packed, Cout, taps, Cin, out);
    else
        hipLaunchKernelGGL(smallm_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_packed, Cout, taps, Cin, out);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// at most 256 pixels (and whole 16-pixel blocks per sample): the 16 x 16-tile kernel (at 512 pixels its 512 blocks pull
// 151 MB of operands through L2 for a 0.6 GFLOP product: no faster than the 32 x 32 tiles' 128 blocks)
bool conv_smallm_tile16(int B, int H, int W) { return (int64_t)B * H * W <= 256 && ((H * W) % 16) == 0; }

// statistics blocks per sample of this kernel's fused statistics (0: the tile geometry does not allow them)
int conv_smallm_stats_blocks(int B, int H, int W) { return conv_smallm_tile16(B, H, W) ? H * W / 16 : sm_stats_blocks(H * W); }

int launch_smallm(const ConvArgs& a, hipStream_t s) {
    const SmTiles t = sm_tiles(a.B, a.H, a.W, a.Cout);
    if (a.stats && a.stats_nblk != conv_smallm_stats_blocks(a.B, a.H, a.W)) {
        set_error("conv_smallm: inconsistent fused-stats geometry (stats_nblk=%d)", a.stats_nblk);
        return ERR_ARG;
    }
    if (conv_smallm_tile16(a.B, a.H, a.W)) {
        if (!a.wsm16) {
            set_error("conv_smallm: the 16 x 16-tile form needs ConvArgs::wsm16");
            return ERR_ARG;
        }
        const int64_t M = (int64_t)a.B * a.H * a.W;
        hipLaunchKernelGGL(conv_smallm16_kernel, dim3((unsigned)(((M + 15) / 16) * (a.Cout / 16))), dim3(512), 0, s, a);
        conv_note_route("smallm_tile16");
    } else if (t.wide) {
        const size_t lds = (size_t)8 * SM_BM * (64 + 4) * sizeof(float);
        if (const int rc = allow_lds<&conv_smallm_kernel<2>>(lds)) return rc;
        hipLaunchKernelGGL((conv_smallm_kernel<2>), dim3(t.mtiles * (a.Cout / 64)), dim3(512), lds, s, a);
        conv_note_route("smallm<2>");
    } else {
        const size_t lds = (size_t)8 * SM_BM * (32 + 4) * sizeof(float);
        if (const int rc = allow_lds<&conv_smallm_kernel<1>>(lds)) return rc;
        hipLaunchKernelGGL((conv_smallm_kernel<1>), dim3(t.mtiles * (a.Cout / 32)), dim3(512), lds, s, a);
        conv_note_route("smallm<1>");
    }
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // namespace flowse
