// Replaces (reference): ddpm_conv3x3 / ddpm_conv1x1 (flowmse/backbones/ncsnpp_utils/layers.py:100-124) and NIN (:546-555) on
// the small images of the network in the 16-bit STORAGE modes (BASELINE configs 2 / 4: bf16 / fp16 activations): at most
// 2048 pixels in the whole batch (the 16 x 16 ... 4 x 4 levels at batch 8).
#include "conv_smallm.h"

namespace flowse {

// The 16-bit twin of conv_smallm_kernel (conv_smallm.hip), over the same ring, operand window and output stage
// (conv_smallm.h, where the loop structure is described): a block owns a 32-pixel x (32 or 64)-channel output tile, its
// eight waves each take every eighth K step (tap, 32-channel chunk) and request their operands straight into the fragment
// registers of v_mfma_f32_32x32x16_{bf16,f16} -- A: two 16-byte pieces per lane and step (8 channels each) through a window
// descriptor, B: the fragment-order weights the producer / consumer kernel already keeps ([Cout/32][chunk][tap][half][lane][8],
// launch_pc16_weights; built for the 1x1 convs as well) -- through a branch-free ring six or eight steps deep.  A step is only
// two or four 32-cycle MFMAs: the kernel is a latency / L2-bandwidth exercise, the ring is what matters.  The eight fp32
// partial tiles meet once in LDS, are summed in a fixed order, and the same pass adds bias / per-sample bias / residual,
// rounds ONCE to the storage type, stores, and leaves the GroupNorm partial statistics of the ROUNDED values (what the
// consumer reads).  Rounds 2-4 ran these shapes through conv_flat16_kernel with fp32 slabs + a reduction launch.
// OT: storage type of res / out -- the operands' 16-bit type, or float (the few convs that leave the 16-bit domain)
template <int NT2, bool F16, class OT>
__global__ __launch_bounds__(512, 2) void conv_smallm16b_kernel(ConvArgs a) {
    using T16 = typename std::conditional<F16, f16_t, bf16_t>::type;
    constexpr int BM = SM_BM, BN = 32 * NT2, CROW = BN + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [8][32][CROW]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const int W = a.W, HW = a.H * W, M = a.B * HW;
    const int C1 = a.C1, C2 = a.C2, Cin = C1 + C2;
    const int taps = a.taps, nchunks = Cin / KC, S_all = nchunks * taps;
    const int n_ntiles = a.Cout / BN;
    const int mt = blockIdx.x / n_ntiles, nt = blockIdx.x - mt * n_ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const SmWindow<T16, BM> win(a, m0, M, li, kh * 8);
    const __amdgpu_buffer_rsrc_t rsrcw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wfrag), 0, a.Cout * taps * Cin * 2, 0x00020000);
    const unsigned bvo = (unsigned)lane * 16u;
    constexpr int D = NT2 == 1 ? 8 : 6;
    u32x4 ra[D][2], rb[D][NT2][2];
    auto gload = [&](int s, auto ring) {
        constexpr int R = decltype(ring)::value;
        const bool live = s < S_all;                          // steps past the end: clamped addresses, A reads as zero
        s = live ? s : S_all - 1;
        const int chunk = s / taps, tap = s - chunk * taps;
        int shift = W + 1;                                    // window origin is pixel m0 - W - 1
        if (taps == 9) shift += (tap / 3 - 1) * W + (tap - (tap / 3) * 3 - 1);
        const int c0 = chunk * KC;
        const bool second = c0 >= C1;
        const unsigned soff_a = (unsigned)(second ? shift * C2 + (c0 - C1) : shift * C1 + c0) * 2u;
        const bool ok = live && ((win.tapmask >> tap) & 1u);
        const unsigned vo = ok ? (second ? win.avo2 : win.avo1) : OOB;
#pragma unroll
        for (int mh = 0; mh < 2; ++mh)
            ra[R][mh] = second ? __builtin_amdgcn_raw_buffer_load_b128(win.rsrc2, vo + mh * 32, soff_a, 0)
                               : __builtin_amdgcn_raw_buffer_load_b128(win.rsrc1, vo + mh * 32, soff_a, 0);
#pragma unroll
        for (int t = 0; t < NT2; ++t) {
            const unsigned soff_b = (unsigned)((((n0 >> 5) + t) * nchunks + chunk) * taps + tap) * 2048u;
#pragma unroll
            for (int mh = 0; mh < 2; ++mh) rb[R][t][mh] = __builtin_amdgcn_raw_buffer_load_b128(rsrcw, bvo + mh * 1024, soff_b, 0);
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
        for (int mh = 0; mh < 2; ++mh)
#pragma unroll
            for (int t = 0; t < NT2; ++t) {
                if (F16)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ra[R][mh]),
                                                                    __builtin_bit_cast(f16x8, rb[R][t][mh]), acc[t], 0, 0, 0);
                else
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ra[R][mh]),
                                                                     __builtin_bit_cast(bf16x8, rb[R][t][mh]), acc[t], 0, 0, 0);
            }
    };
    ring_run<D, 8>((S_all + 7) >> 3, wave, gload, compute);

    float* Cw = smem + wave * (BM * CROW);
#pragma unroll
    for (int t = 0; t < NT2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Cw[((r & 3) + 8 * (r >> 2) + 4 * kh) * CROW + t * 32 + li] = acc[t][r];
    sm_finish<BM, BN, OT>(a, smem, m0, n0, M, HW);
}

// shapes the kernel takes in the 16-bit storage modes: at most 2048 pixels, 32-aligned channel counts, whole statistics
// blocks, and not one of the launches the LDS-halo kernels cover anyway (those need >= 128 blocks of 128 pixels)
static const bool g_no_smallm16 = getenv("FLOWSE_NO_SMALLM") != nullptr || getenv("FLOWSE_FORCE_GENERIC_CONV") != nullptr;
bool conv16_smallm_enabled() { return !g_no_smallm16; }
bool conv16_smallm_ok(int B, int H, int W, int C1, int C2, int Cout, int taps) {
    if (g_no_smallm16 || !sm_shape_ok(B, H, W, C1, C2, Cout, taps, 2048, 2) || sm_stats_blocks(H * W) == 0) return false;
    return !conv16_uses_halo(B, H, W, C1, C2, Cout, taps);
}

// statistics blocks per sample of the 16-bit kernel's fused statistics: blocks of min(32, H W) pixels
int conv16_smallm_stats_blocks(int B, int H, int W) { (void)B; return sm_stats_blocks(H * W); }

int launch_smallm16b(const ConvArgs& a, hipStream_t s) {
    if (!a.wfrag || a.in_dt == DT_F32 || (a.out_dt != a.in_dt && a.out_dt != DT_F32) || (a.wq_f16 ? DT_F16 : DT_BF16) != a.in_dt || a.gn.mean ||
        !conv16_smallm_ok(a.B, a.H, a.W, a.C1, a.C2, a.Cout, a.taps)) {
        set_error("conv_smallm16b: unsupported configuration (C1=%d C2=%d in_dt=%d out_dt=%d)", a.C1, a.C2, a.in_dt, a.out_dt);
        return ERR_ARG;
    }
    if (a.stats && a.stats_nblk != conv16_smallm_stats_blocks(a.B, a.H, a.W)) {
        set_error("conv_smallm16b: inconsistent fused-stats geometry (stats_nblk=%d)", a.stats_nblk);
        return ERR_ARG;
    }
    const SmTiles tl = sm_tiles(a.B, a.H, a.W, a.Cout);
#define FLOWSE_LSM16(NT2, F16, OT)                                                                            \
    {                                                                                                        \
        const size_t lds = (size_t)8 * 32 * (32 * NT2 + 4) * sizeof(float);                                  \
        if (const int rc = allow_lds<&conv_smallm16b_kernel<NT2, F16, OT>>(lds)) return rc;                  \
        hipLaunchKernelGGL((conv_smallm16b_kernel<NT2, F16, OT>), dim3(tl.mtiles * (a.Cout / (32 * NT2))), dim3(512), lds, s, a); \
        conv_note_route("smallm16b<" #NT2 ", ", F16 ? "f16, " : "bf16, ", sizeof(OT) == 4 ? "out32>" : "out16>"); \
    }
    const bool of32 = a.out_dt == DT_F32;
    if (a.wq_f16) {
        if (tl.wide) { if (of32) FLOWSE_LSM16(2, true, float) else FLOWSE_LSM16(2, true, f16_t) }
        else { if (of32) FLOWSE_LSM16(1, true, float) else FLOWSE_LSM16(1, true, f16_t) }
    } else {
        if (tl.wide) { if (of32) FLOWSE_LSM16(2, false, float) else FLOWSE_LSM16(2, false, bf16_t) }
        else { if (of32) FLOWSE_LSM16(1, false, float) else FLOWSE_LSM16(1, false, bf16_t) }
    }
#undef FLOWSE_LSM16
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // namespace flowse
