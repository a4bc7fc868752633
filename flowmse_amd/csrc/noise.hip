// Keyed prior noise: x_T = y + sigma * z with z ~ CN(0, 1) generated in registers from a counter-based stream, so the
// noise of an utterance depends on (seed, utterance key, bin, frame) only -- not on the batch it rides in, its row, the
// padded length, or the order of calls.  Replaces (reference): the torch.randn_like of FLOWMATCHING.prior_sampling
// (flowmse/odes.py:93-100).  The stream is a public contract ("Keyed noise stream"):
//
//   Philox4x32-10 (Salmon et al., SC'11; Random123 known answers in tests/test_keyed_noise_host.py)
//   counter = (t >> 1, f, lo32(key_b), hi32(key_b)),  Philox key = (lo32(seed), hi32(seed))
//   t is the ABSOLUTE frame of the utterance: frame0_b + the frame's index in the row (frame0_b = 0 without offsets)
//   words (0, 1) -> the value at the even frame t, words (2, 3) -> the value at t + 1
//   u1 = ((w_a >> 9) + 0.5) * 2^-23 in (0, 1),  u2 = (w_b >> 8) * 2^-24 in [0, 1)      (both exact in fp32)
//   z  = sqrtf(-logf(u1)) * (cospif(2 u2) + i sinpif(2 u2))                                (E|z|^2 = 1)
//
// The four keyed entries of the C ABI (flowse_prior_sample_keyed[_at], flowse_op_keyed_noise[_at]) are at the end.
#include <vector>

#include "../../include/flowse_hip.h"
#include "noise.h"

namespace flowse {

// One thread per Philox call: frames (2 t2, 2 t2 + 1) of one bin of one row = one 16-byte load and store.  The float4
// index of a thread IS its linear index (rows are [F][T] complex, T even).  ADD: out = y + sigma * z, else out = z.
// AT: row b starts at the even absolute frame frame0[b] of its utterance (a chunk of a recording).
template <bool ADD, bool AT>
__global__ __launch_bounds__(256) void keyed_noise_kernel(const float4* __restrict__ y, const uint64_t* __restrict__ keys,
                                                          const int32_t* __restrict__ frame0, uint32_t seed_lo,
                                                          uint32_t seed_hi, float sigma, int F, int Th, int64_t n,
                                                          float4* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        uint32_t t2 = (uint32_t)(i % Th);
        const int64_t row = i / Th;
        const uint32_t f = (uint32_t)(row % F);
        const uint64_t key = keys[row / F];
        if (AT) t2 += (uint32_t)frame0[row / F] >> 1;
        uint32_t w[4];
        philox4x32_10(t2, f, (uint32_t)key, (uint32_t)(key >> 32), seed_lo, seed_hi, w);
        const float2 za = complex_normal(w[0], w[1]), zb = complex_normal(w[2], w[3]);
        if (ADD) {
            const float4 v = y[i];
            out[i] = make_float4(v.x + __fmul_rn(za.x, sigma), v.y + __fmul_rn(za.y, sigma),
                                 v.z + __fmul_rn(zb.x, sigma), v.w + __fmul_rn(zb.y, sigma));
        } else {
            out[i] = make_float4(za.x, za.y, zb.x, zb.y);
        }
    }
}

template <bool ADD, bool AT>
static void launch_one(unsigned blocks, hipStream_t s, const float* y, const uint64_t* keys, const int32_t* frame0,
                       uint32_t lo, uint32_t hi, float sigma, int F, int Th, int64_t n, float* out) {
    hipLaunchKernelGGL((keyed_noise_kernel<ADD, AT>), dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(y),
                       keys, frame0, lo, hi, sigma, F, Th, n, reinterpret_cast<float4*>(out));
}

// out = y + sigma * z (y != null) or out = z (y == null), z = the keyed Philox noise of noise.hip; [B,1,F,T] complex64,
// T even, 16-byte aligned pointers, keys: B device words; frame0 (may be null): B device words, the even absolute frame
// each row starts at
static int launch_keyed_noise(const float* y, const uint64_t* keys, const int32_t* frame0, uint64_t seed, float sigma,
                              float* out, int B, int F, int T, hipStream_t s) {
    const int Th = T / 2;
    const int64_t n = (int64_t)B * F * Th;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    const unsigned g = (unsigned)blocks;
    if (y && frame0) launch_one<true, true>(g, s, y, keys, frame0, lo, hi, sigma, F, Th, n, out);
    else if (y) launch_one<true, false>(g, s, y, keys, nullptr, lo, hi, sigma, F, Th, n, out);
    else if (frame0) launch_one<false, true>(g, s, nullptr, keys, frame0, lo, hi, 0.f, F, Th, n, out);
    else launch_one<false, false>(g, s, nullptr, keys, nullptr, lo, hi, 0.f, F, Th, n, out);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // namespace flowse

using namespace flowse;

extern "C" {

static int keyed_args_ok(const char* who, const void* y, bool need_y, const uint64_t* keys, const void* out, int B, int F,
                         int T) {
    if ((need_y && !y) || !keys || !out || B <= 0 || F <= 0 || T <= 0 || (T & 1)) {
        set_error("%s: bad argument (null pointer, B / F / T <= 0 or odd T; got B=%d F=%d T=%d)", who, B, F, T);
        return ERR_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 15) {
        set_error("%s: y and the output must be 16-byte aligned", who);
        return ERR_ARG;
    }
    return OK;
}

int flowse_prior_sample_keyed(const void* y, const uint64_t* keys_dev, uint64_t seed, float sigma, void* x_out, int B, int F,
                              int T, void* stream) {
    if (const int rc = keyed_args_ok("flowse_prior_sample_keyed", y, true, keys_dev, x_out, B, F, T)) return rc;
    return launch_keyed_noise(static_cast<const float*>(y), keys_dev, nullptr, seed, sigma, static_cast<float*>(x_out), B,
                              F, T, static_cast<hipStream_t>(stream));
}

int flowse_op_keyed_noise(const uint64_t* keys_dev, uint64_t seed, void* z_out_c64, int B, int F, int T, void* stream) {
    if (const int rc = keyed_args_ok("flowse_op_keyed_noise", nullptr, false, keys_dev, z_out_c64, B, F, T)) return rc;
    return launch_keyed_noise(nullptr, keys_dev, nullptr, seed, 0.f, static_cast<float*>(z_out_c64), B, F, T,
                              static_cast<hipStream_t>(stream));
}

// The frame offsets of the *_at calls are read back and checked here, on the host side of the call (one stream
// synchronisation): an odd offset would pair the Philox words of a frame differently than the offset-free stream does.
static int frame0_ok(const char* who, const int32_t* frame0_dev, int B, int T, hipStream_t s) {
    if (!frame0_dev) {
        set_error("%s: null frame0_dev", who);
        return ERR_ARG;
    }
    std::vector<int32_t> h((size_t)B);
    FLOWSE_HIP(hipMemcpyAsync(h.data(), frame0_dev, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FLOWSE_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b)
        if (h[b] < 0 || (h[b] & 1) || h[b] > INT32_MAX - T) {
            set_error("%s: frame0[%d] = %d must be even, >= 0 and <= INT32_MAX - T", who, b, (int)h[b]);
            return ERR_ARG;
        }
    return OK;
}

int flowse_prior_sample_keyed_at(const void* y, const uint64_t* keys_dev, const int32_t* frame0_dev, uint64_t seed,
                                 float sigma, void* x_out, int B, int F, int T, void* stream) {
    if (const int rc = keyed_args_ok("flowse_prior_sample_keyed_at", y, true, keys_dev, x_out, B, F, T)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = frame0_ok("flowse_prior_sample_keyed_at", frame0_dev, B, T, s)) return rc;
    return launch_keyed_noise(static_cast<const float*>(y), keys_dev, frame0_dev, seed, sigma, static_cast<float*>(x_out),
                              B, F, T, s);
}

int flowse_op_keyed_noise_at(const uint64_t* keys_dev, const int32_t* frame0_dev, uint64_t seed, void* z_out_c64, int B,
                             int F, int T, void* stream) {
    if (const int rc = keyed_args_ok("flowse_op_keyed_noise_at", nullptr, false, keys_dev, z_out_c64, B, F, T)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = frame0_ok("flowse_op_keyed_noise_at", frame0_dev, B, T, s)) return rc;
    return launch_keyed_noise(nullptr, keys_dev, frame0_dev, seed, 0.f, static_cast<float*>(z_out_c64), B, F, T, s);
}

}  // extern "C"
