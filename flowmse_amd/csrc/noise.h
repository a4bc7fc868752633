// Device functions of the keyed noise stream (noise.hip has the contract): the Philox4x32-10 block and the map from two of
// its words to one complex standard normal.  A header so that every kernel that generates the stream in registers
// (keyed_noise_kernel, the flow-matching kernels of fmloss.hip) compiles the same text.
#pragma once
#include "common.h"

namespace flowse {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ float2 complex_normal(uint32_t wa, uint32_t wb) {
    const float u1 = ((float)(wa >> 9) + 0.5f) * 0x1p-23f;       // 23-bit integer + 0.5: exact
    const float u2x2 = (float)(wb >> 8) * 0x1p-23f;              // 2 * u2, exact
    const float r = sqrtf(-logf(u1));
    return make_float2(r * cospif(u2x2), r * sinpif(u2x2));
}

// The two values of one Philox call: frames (2 t2, 2 t2 + 1) of bin f of the row of `key`, as (re, im, re, im).
__device__ __forceinline__ float4 keyed_noise_pair(uint32_t t2, uint32_t f, uint64_t key, uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t w[4];
    philox4x32_10(t2, f, (uint32_t)key, (uint32_t)(key >> 32), seed_lo, seed_hi, w);
    const float2 za = complex_normal(w[0], w[1]), zb = complex_normal(w[2], w[3]);
    return make_float4(za.x, za.y, zb.x, zb.y);
}

}  // namespace flowse
