// Shared pieces of the kernels that split K INSIDE the block and request their operands straight into MFMA fragment
// registers: conv_smallm_kernel / conv_smallm16_kernel (conv_smallm.hip) and conv_smallm16b_kernel (conv16_smallm.hip);
// conv1x1_stream_kernel (conv_1x1.hip) runs the same ring with its loop written out.  Internal to those translation units
// (+ conv_dispatch.hip for the host-side shape rules).  The kernels keep what is their own: fragment layouts, weight index
// formulas, MFMA sequences and the per-step address arithmetic (profiles/smallm_shared_asm.md says why).
#pragma once
#include "conv_common.h"

namespace flowse {

constexpr int SM_BM = 32;       // pixels per tile of the 32 x 32-MFMA kernels (the 16 x 16-tile kernel: 16)

// ---- the register ring ------------------------------------------------------------------------------------------------
// f(integral_constant<int, 0>) ... f(integral_constant<int, D - 1>): register-ring slots are compile-time indices
template <class F, int... I>
__device__ __forceinline__ void ring_unroll(F& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

// A wave walks steps first, first + STRIDE, ...: nsteps of them, ring slot of its i-th step = i % D.  gload(s, slot) requests
// the operands of step s into slot `slot`, compute(slot) issues the MFMAs of the step held there.  No request sits under a
// runtime branch (hipcc drains vmcnt at every join: a conditional request serialised the whole ring -- 1 us per step): a
// prologue of D - 1 requests, a uniform loop of D-step groups with requests D - 1 steps ahead -- gload clamps the steps past
// the end to harmless addresses -- and a tail of at most D - 1 steps whose operands are already in flight.  (STRIDE is a
// compile-time value: as an argument it costs conv_smallm_kernel<2> a scalar add inside the loop.)
template <int D, int STRIDE, class G, class C>
__device__ __forceinline__ void ring_run(int nsteps, int first, G& gload, C& compute) {
    auto pro = [&](auto dc) {
        constexpr int d = decltype(dc)::value;
        if constexpr (d < D - 1) gload(first + STRIDE * d, dc);
    };
    ring_unroll(pro, std::make_integer_sequence<int, D>{});
    int i = 0;
    for (; i + D <= nsteps; i += D) {
        auto step = [&](auto dc) {
            constexpr int d = decltype(dc)::value;
            gload(first + STRIDE * (i + d + D - 1), std::integral_constant<int, (d + D - 1) % D>{});
            __builtin_amdgcn_sched_barrier(0);            // (hipcc otherwise sinks the requests down to their first use)
            compute(dc);
            __builtin_amdgcn_sched_barrier(0);
        };
        ring_unroll(step, std::make_integer_sequence<int, D>{});
    }
    const int rem = nsteps - i;
    auto tail = [&](auto dc) {
        constexpr int d = decltype(dc)::value;
        if constexpr (d < D - 1) {
            if (d < rem) compute(dc);
        }
    };
    ring_unroll(tail, std::make_integer_sequence<int, D>{});
}

// ---- the small-image operand window -----------------------------------------------------------------------------------
// which taps of pixel m fall inside its image (bit t); 0 for the rows past M
__device__ __forceinline__ unsigned sm_tapmask(int m, int M, int H, int W, int HW, int taps) {
    unsigned tapmask = 0;
    if (m < M) {
        const int rem = m % HW;
        const int y = rem / W, x = rem - y * W;
        if (taps == 9) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
                if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) tapmask |= 1u << t;
            }
        } else {
            tapmask = 1u;
        }
    }
    return tapmask;
}

// A tile's view of the two NHWC sources (the channel concat = two K ranges) of element type T: one wave-uniform descriptor
// per source over pixels m0 - W - 1 ... + BM + 2 W + 2 (every tap of every pixel of the tile), this lane's byte offset
// inside each and its tap mask.  Conv zero padding and the steps past the end = the offset OOB, for which the hardware returns
// 0.  li: the lane's pixel of the tile, kofs: its first channel inside a 32-channel chunk.
// (The per-step arithmetic on these stays written out in each kernel's gload: moved into a function of any form it costs the
// fp32 kernels two scalar registers, profiles/smallm_shared_asm.md.)
template <class T, int BM>
struct SmWindow {
    __amdgpu_buffer_rsrc_t rsrc1, rsrc2;
    unsigned avo1, avo2, tapmask;
    __device__ __forceinline__ SmWindow(const ConvArgs& a, int m0, int M, int li, int kofs) {
        const int W = a.W, C1 = a.C1, C2 = a.C2;
        tapmask = sm_tapmask(m0 + li, M, a.H, W, a.H * W, a.taps);
        avo1 = (unsigned)(li * C1 + kofs) * (unsigned)sizeof(T);
        avo2 = (unsigned)(li * C2 + kofs) * (unsigned)sizeof(T);
        const int64_t wbase = (int64_t)m0 - W - 1;
        const int wpix = BM + 2 * W + 2;
        const T* in1 = reinterpret_cast<const T*>(a.in1);
        const T* in2 = reinterpret_cast<const T*>(a.in2);
        rsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(in1 + wbase * C1), 0, wpix * C1 * (int)sizeof(T), 0x00020000);
        rsrc2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(C2 ? in2 + wbase * C2 : in1), 0,
                                                  C2 ? wpix * C2 * (int)sizeof(T) : 0, 0x00020000);
    }
};

// ---- the output stage -------------------------------------------------------------------------------------------------
// The eight waves' partial tiles sit in LDS, Cs[wave][BM][BN + 4].  They are summed in a fixed order (bit-reproducible) and
// the same pass adds bias / per-sample bias / residual, scales, rounds ONCE to the storage type OT of res / out and stores
// 16-byte (fp32) or 8-byte quads: thread = (tile row, channel quad).  With a.stats it then leaves the GroupNorm partial
// statistics of what it stored, as the consumer will read it: blocks of PB = min(BM, H W) consecutive pixels of one sample
// (launch guarantees: BM % PB == 0, H W % PB == 0, M % PB == 0; PBC: PB where the launch fixes it).  The finished tile goes
// back to LDS slice 0 and one thread per (block, channel) takes mean and M2 in two passes over its PB values (exact, order
// fixed).  All 512 threads must call, right after writing their slice.
template <int BM, int BN, class OT, int PBC = 0>
__device__ __forceinline__ void sm_finish(const ConvArgs& a, float* Cs, int m0, int n0, int M, int HW) {
    constexpr int CROW = BN + 4, C4 = BN / 4;
    const int tid = threadIdx.x;
    __syncthreads();
    const int row = tid / C4, cq = tid - row * C4;       // BN / 4 quads x BM rows = 64 (16 x 16), 256 or 512 (32 x 64) items
    const bool act = row < BM;
    const int mo = m0 + row;
    const int n = n0 + cq * 4;
    OT* outp = reinterpret_cast<OT*>(a.out);
    const OT* resp = reinterpret_cast<const OT*>(a.res);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (act) {
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const float4 t = *reinterpret_cast<const float4*>(Cs + (w * BM + row) * CROW + cq * 4);
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        if (a.bias) {
            const float4 t = *reinterpret_cast<const float4*>(a.bias + n);
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        if (mo < M) {
            if (a.bias2) {
                const float4 t = *reinterpret_cast<const float4*>(a.bias2 + (int64_t)(mo / HW) * a.bias2_stride + n);
                v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
            }
            if (a.res) {
                const float4 t = St<OT>::ld4(resp + (int64_t)mo * a.Cout + n);
                v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
            }
            v.x *= a.scale; v.y *= a.scale; v.z *= a.scale; v.w *= a.scale;
            St<OT>::st4(outp + (int64_t)mo * a.Cout + n, v);
            v = St<OT>::rnd4(v);                              // statistics of what the consumer will read
        }
    }
    if (!a.stats) return;
    __syncthreads();                                     // everyone has read the eight slices
    if (act) *reinterpret_cast<float4*>(Cs + row * CROW + cq * 4) = v;
    __syncthreads();
    const int PB = PBC ? PBC : HW < BM ? HW : BM;
    const int groups = BM / PB;
    for (int idx = tid; idx < groups * BN; idx += 512) {      // (H W < 4: more (block, channel) pairs than threads)
        const int g = idx / BN, c = idx - g * BN;
        const int mg = m0 + g * PB;
        if (mg < M) {
            float sum = 0.f;
            for (int r = 0; r < PB; ++r) sum += Cs[(g * PB + r) * CROW + c];
            const float mean = sum / (float)PB;
            float m2 = 0.f;
            for (int r = 0; r < PB; ++r) {
                const float d = Cs[(g * PB + r) * CROW + c] - mean;
                m2 = fmaf(d, d, m2);
            }
            const int bs = mg / HW, blk = (mg - bs * HW) / PB;
            float* dst = a.stats + (((int64_t)bs * a.stats_nblk + blk) * a.Cout + n0 + c) * 2;
            dst[0] = mean;
            dst[1] = m2;
        }
    }
}

// ---- host side: the shape rules the launchers and the predicates share -------------------------------------------------
// 32-pixel tiles of a launch: 64-channel tiles when that still gives every CU a block, else 32-channel tiles (twice the blocks)
struct SmTiles { int mtiles; bool wide; };
inline SmTiles sm_tiles(int B, int H, int W, int Cout) {
    const int mtiles = (int)(((int64_t)B * H * W + SM_BM - 1) / SM_BM);
    return {mtiles, (Cout % 64) == 0 && (int64_t)mtiles * (Cout / 64) >= 256};
}

// statistics blocks per sample, blocks of PB = min(32, H W) pixels (0: the tile geometry does not allow them)
inline int sm_stats_blocks(int HW) {
    const int PB = HW < SM_BM ? HW : SM_BM;
    return (PB > 0 && (SM_BM % PB) == 0 && (HW % PB) == 0) ? HW / PB : 0;
}

// what both predicates ask of a shape: 1x1 or 3x3, 32-aligned channel counts, 1 ... max_pixels pixels in the batch, window
// and weight descriptors below 2 GB at `esize` bytes per element
inline bool sm_shape_ok(int B, int H, int W, int C1, int C2, int Cout, int taps, int64_t max_pixels, int esize) {
    if ((taps != 1 && taps != 9) || (C1 % KC) || (C2 % KC) || (Cout % 32) || C1 <= 0) return false;
    const int64_t M = (int64_t)B * H * W;
    if (M > max_pixels || M < 1) return false;
    const int64_t cmax = C1 > C2 ? C1 : C2;
    return (int64_t)(SM_BM + 2 * W + 2) * cmax * esize < (1LL << 31) && (int64_t)Cout * taps * (C1 + C2) * esize < (1LL << 31);
}

}  // namespace flowse
