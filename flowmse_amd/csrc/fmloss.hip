// Flow-matching objective on the device: the number a checkpoint is trained on (reference VFModel._step, flowmse/model.py:130-143).
// For a row with clean spectrogram x0, noisy y, time t and noise z (complex64 [B,1,F,T], t float32 [B]):
//
//   sigma(t) = (1 - t) sigma_min + t sigma_max                            odes.py:86-88
//   x_t      = (1 - t) x0 + t y + sigma(t) z                              odes.py:83-84, model.py:134-137
//   u        = (sigma_max - sigma_min) z + (y - x0)                       odes.py:102-107, model.py:138-140
//   v        = VFModel.forward(x_t, t, y) = -dnn(cat[x_t, y], t)          model.py:141, 164-170
//   loss_b   = 0.5 * sum_{f,frame} |v - u|^2      ('mse')                 model.py:118-128
//            = 0.5 * sum_{f,frame} |v - u|        ('mae')
//   loss     = mean_b loss_b
//
// Three HBM-bound streams around the network.  fm_pair_kernel forms x_t (and, on request, u) in fp32 with the reference's
// operation order; fm_loss_partial_kernel re-forms u in float64 from the fp32 inputs -- the target never exists as a tensor
// on the loss path -- and sums |v - u|^2 or |v - u| in float64; fm_loss_finish_kernel merges the block partials in index
// order.  z is either a tensor or generated in registers from the keyed stream of noise.h.  No atomics: the same input
// gives the same bits, and a row's value depends on nothing but that row.
#include <algorithm>

#include "model.h"
#include "noise.h"

namespace flowse {

constexpr int FM_THREADS = 256;
constexpr int FM_PAIR_MAX_BLOCKS = 512;     // two blocks per compute unit; larger tensors loop
constexpr int FM_ROW_MAX_BLOCKS = 64;       // loss partials per row

// One thread per Philox call: frames (2 t2, 2 t2 + 1) of one bin of one row = one 16-byte load and store per tensor, the
// thread geometry of keyed_noise_kernel.  Per real part, in this order (every operation rounds once, nothing is fused):
//   a = 1 - t;  sig = a sigma_min + t sigma_max;  x_t = (a x0 + t y) + sig z;  u = (sigma_max - sigma_min) z + (y - x0)
template <bool KEYED, bool TARGET>
__global__ __launch_bounds__(FM_THREADS) void fm_pair_kernel(const float4* __restrict__ x0, const float4* __restrict__ y,
                                                             const float* __restrict__ t, const float4* __restrict__ z,
                                                             const uint64_t* __restrict__ keys, uint32_t seed_lo,
                                                             uint32_t seed_hi, float sigma_min, float sigma_max, int F, int Th,
                                                             int64_t n, float4* __restrict__ xt, float4* __restrict__ u) {
    const float ds = __fsub_rn(sigma_max, sigma_min);
    for (int64_t i = (int64_t)blockIdx.x * FM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FM_THREADS) {
        const int64_t row = i / Th;
        const int64_t b = row / F;
        const float tb = t[b];
        const float a = __fsub_rn(1.f, tb);
        const float sig = __fadd_rn(__fmul_rn(a, sigma_min), __fmul_rn(tb, sigma_max));
        float4 zz;
        if (KEYED) zz = keyed_noise_pair((uint32_t)(i % Th), (uint32_t)(row % F), keys[b], seed_lo, seed_hi);
        else zz = z[i];
        const float4 c = x0[i], d = y[i];
        auto path = [&](float cv, float dv, float zv) {
            return __fadd_rn(__fadd_rn(__fmul_rn(a, cv), __fmul_rn(tb, dv)), __fmul_rn(sig, zv));
        };
        xt[i] = make_float4(path(c.x, d.x, zz.x), path(c.y, d.y, zz.y), path(c.z, d.z, zz.z), path(c.w, d.w, zz.w));
        if (TARGET) {
            auto field = [&](float cv, float dv, float zv) { return __fadd_rn(__fmul_rn(ds, zv), __fsub_rn(dv, cv)); };
            u[i] = make_float4(field(c.x, d.x, zz.x), field(c.y, d.y, zz.y), field(c.z, d.z, zz.z), field(c.w, d.w, zz.w));
        }
    }
}

// blocks a row of F x T values is summed in: a function of (F, T) only, so a row's partition -- and with it every bit of
// its loss -- does not depend on the batch it rides in or on its position
static int fm_row_blocks(int F, int T) {
    const int64_t n4 = (int64_t)F * (T / 2);
    const int64_t nblk = (n4 + 2 * FM_THREADS - 1) / (2 * FM_THREADS);
    return (int)std::min<int64_t>(std::max<int64_t>(nblk, 1), FM_ROW_MAX_BLOCKS);
}

// Block blk of row b owns the row's float4 j = blk 256 + thread (mod nblk 256): a per-thread strided sum in float64, then
// the fixed-order tree.  d = v - u with u = ds z + (y - x0), every operation in float64 on the fp32 inputs.
template <bool KEYED, bool MAE>
__global__ __launch_bounds__(FM_THREADS) void fm_loss_partial_kernel(const float4* __restrict__ v, const float4* __restrict__ x0,
                                                                     const float4* __restrict__ y, const float4* __restrict__ z,
                                                                     const uint64_t* __restrict__ keys, uint32_t seed_lo,
                                                                     uint32_t seed_hi, double ds, int Th, int64_t n4, int nblk,
                                                                     double* __restrict__ partial) {
    __shared__ double red[FM_THREADS];
    const int64_t b = blockIdx.x / nblk;
    const int blk = blockIdx.x % nblk;
    const int64_t base = b * n4;
    double acc = 0.0;
    for (int64_t j = (int64_t)blk * FM_THREADS + threadIdx.x; j < n4; j += (int64_t)nblk * FM_THREADS) {
        float4 zz;
        if (KEYED) zz = keyed_noise_pair((uint32_t)(j % Th), (uint32_t)(j / Th), keys[b], seed_lo, seed_hi);
        else zz = z[base + j];
        const float4 vv = v[base + j], c = x0[base + j], d = y[base + j];
        auto diff = [&](float vf, float cv, float dv, float zv) {
            return (double)vf - (ds * (double)zv + ((double)dv - (double)cv));
        };
        const double ar = diff(vv.x, c.x, d.x, zz.x), ai = diff(vv.y, c.y, d.y, zz.y);
        const double br = diff(vv.z, c.z, d.z, zz.z), bi = diff(vv.w, c.w, d.w, zz.w);
        const double qa = ar * ar + ai * ai, qb = br * br + bi * bi;
        acc += MAE ? sqrt(qa) : qa;
        acc += MAE ? sqrt(qb) : qb;
    }
    red[threadIdx.x] = acc;
    tree_sum(red, FM_THREADS);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// out[b] = 0.5 * (the row's partials in index order); out[B] = (out[0] + out[1] + ...) / B in row order
__global__ __launch_bounds__(FM_THREADS) void fm_loss_finish_kernel(const double* __restrict__ partial, int nblk, int B,
                                                                    double* __restrict__ out) {
    for (int b = threadIdx.x; b < B; b += FM_THREADS) {
        double s = 0.0;
        for (int k = 0; k < nblk; ++k) s += partial[(int64_t)b * nblk + k];
        out[b] = 0.5 * s;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += out[b];
        out[B] = s / (double)B;
    }
}

static int launch_fm_pair(const float* x0, const float* y, const float* t, const float* z, const uint64_t* keys, uint64_t seed,
                          float sigma_min, float sigma_max, float* xt, float* u, int B, int F, int T, hipStream_t s) {
    const int Th = T / 2;
    const int64_t n = (int64_t)B * F * Th;
    const unsigned g = (unsigned)std::min<int64_t>((n + FM_THREADS - 1) / FM_THREADS, FM_PAIR_MAX_BLOCKS);
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(g), dim3(FM_THREADS), 0, s, reinterpret_cast<const float4*>(x0),
                           reinterpret_cast<const float4*>(y), t, reinterpret_cast<const float4*>(z), keys, lo, hi, sigma_min,
                           sigma_max, F, Th, n, reinterpret_cast<float4*>(xt), reinterpret_cast<float4*>(u));
    };
    if (keys && u) go(fm_pair_kernel<true, true>);
    else if (keys) go(fm_pair_kernel<true, false>);
    else if (u) go(fm_pair_kernel<false, true>);
    else go(fm_pair_kernel<false, false>);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

static int64_t fm_workspace_bytes(int B, int F, int T) {
    return ((int64_t)B * fm_row_blocks(F, T) * (int64_t)sizeof(double) + 255) & ~(int64_t)255;
}

static int launch_fm_loss_rows(const float* v, const float* x0, const float* y, const float* z, const uint64_t* keys,
                               uint64_t seed, float sigma_min, float sigma_max, int mae, double* out, double* partial, int B,
                               int F, int T, hipStream_t s) {
    const int Th = T / 2, nblk = fm_row_blocks(F, T);
    const int64_t n4 = (int64_t)F * Th;
    const double ds = (double)sigma_max - (double)sigma_min;
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((int64_t)B * nblk)), dim3(FM_THREADS), 0, s,
                           reinterpret_cast<const float4*>(v), reinterpret_cast<const float4*>(x0),
                           reinterpret_cast<const float4*>(y), reinterpret_cast<const float4*>(z), keys, lo, hi, ds, Th, n4, nblk,
                           partial);
    };
    if (keys && mae) go(fm_loss_partial_kernel<true, true>);
    else if (keys) go(fm_loss_partial_kernel<true, false>);
    else if (mae) go(fm_loss_partial_kernel<false, true>);
    else go(fm_loss_partial_kernel<false, false>);
    hipLaunchKernelGGL(fm_loss_finish_kernel, dim3(1), dim3(FM_THREADS), 0, s, partial, nblk, B, out);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// the checks the three entries share: shape, the noise source, alignment
static int fm_args_ok(const char* who, bool null_ptr, const void* z, const void* keys, int B, int F, int T,
                      std::initializer_list<const void*> aligned) {
    if (null_ptr || B <= 0 || F <= 0 || T <= 0 || (T & 1) || (int64_t)B * fm_row_blocks(F, T) > INT32_MAX) {
        set_error("%s: bad argument (null pointer, B / F / T <= 0 or odd T; got B=%d F=%d T=%d)", who, B, F, T);
        return ERR_ARG;
    }
    if ((z != nullptr) == (keys != nullptr)) {
        set_error("%s: exactly one of z and keys_dev must be given (got %s)", who, z ? "both" : "neither");
        return ERR_ARG;
    }
    uintptr_t bits = reinterpret_cast<uintptr_t>(z);
    for (const void* p : aligned) bits |= reinterpret_cast<uintptr_t>(p);
    if (bits & 15) {
        set_error("%s: the complex64 tensors must be 16-byte aligned", who);
        return ERR_ARG;
    }
    return OK;
}

static int fm_loss_type_ok(const char* who, int loss_type) {
    if (loss_type == FLOWSE_LOSS_MSE || loss_type == FLOWSE_LOSS_MAE) return OK;
    set_error("%s: loss_type must be FLOWSE_LOSS_MSE (0) or FLOWSE_LOSS_MAE (1), got %d", who, loss_type);
    return ERR_ARG;
}

}  // namespace flowse

extern "C" {

int flowse_fm_pair(const void* x0, const void* y, const float* t_dev, const void* z, const uint64_t* keys_dev, uint64_t seed,
                   float sigma_min, float sigma_max, void* xt_out, void* target_out, int B, int F, int T, void* stream) {
    if (const int rc = fm_args_ok("flowse_fm_pair", !x0 || !y || !t_dev || !xt_out, z, keys_dev, B, F, T,
                                  {x0, y, xt_out, target_out}))
        return rc;
    return launch_fm_pair(static_cast<const float*>(x0), static_cast<const float*>(y), t_dev, static_cast<const float*>(z),
                          keys_dev, seed, sigma_min, sigma_max, static_cast<float*>(xt_out), static_cast<float*>(target_out), B,
                          F, T, static_cast<hipStream_t>(stream));
}

int64_t flowse_fm_loss_workspace_bytes(int B, int F, int T) {
    if (B <= 0 || F <= 0 || T <= 0 || (T & 1)) {
        set_error("flowse_fm_loss_workspace_bytes: B, F, T must be positive and T even (got B=%d F=%d T=%d)", B, F, T);
        return -(int64_t)ERR_ARG;
    }
    return fm_workspace_bytes(B, F, T);
}

int flowse_fm_loss_rows(const void* vf, const void* x0, const void* y, const void* z, const uint64_t* keys_dev, uint64_t seed,
                        float sigma_min, float sigma_max, int loss_type, double* out, void* workspace, int64_t workspace_bytes,
                        int B, int F, int T, void* stream) {
    const char* who = "flowse_fm_loss_rows";
    if (const int rc = fm_args_ok(who, !vf || !x0 || !y || !out || !workspace, z, keys_dev, B, F, T, {vf, x0, y})) return rc;
    if (const int rc = fm_loss_type_ok(who, loss_type)) return rc;
    if (workspace_bytes < fm_workspace_bytes(B, F, T) || (reinterpret_cast<uintptr_t>(workspace) & 7)) {
        set_error("%s: the workspace needs %lld bytes (8-byte aligned), got %lld", who, (long long)fm_workspace_bytes(B, F, T),
                  (long long)workspace_bytes);
        return ERR_ARG;
    }
    return launch_fm_loss_rows(static_cast<const float*>(vf), static_cast<const float*>(x0), static_cast<const float*>(y),
                               static_cast<const float*>(z), keys_dev, seed, sigma_min, sigma_max, loss_type == FLOWSE_LOSS_MAE,
                               out, static_cast<double*>(workspace), B, F, T, static_cast<hipStream_t>(stream));
}

// pair -> the shape's launch list in mode 1 (flowse_vf_forward's path, per-row t) -> loss; x_t, v and the partials live in
// the handle's d_fm, reserved on first use
int flowse_fm_loss(flowse_model* m, const void* x0, const void* y, const float* t_dev, const void* z, const uint64_t* keys_dev,
                   uint64_t seed, float sigma_min, float sigma_max, int loss_type, double* out, int B, int F, int T,
                   void* stream) {
    const char* who = "flowse_fm_loss";
    if (const int rc = fm_args_ok(who, !m || !x0 || !y || !t_dev || !out, z, keys_dev, B, F, T, {x0, y})) return rc;
    if (const int rc = fm_loss_type_ok(who, loss_type)) return rc;
    if (m->block_kind >= 0) {
        set_error("%s: a single-module handle has no vector field", who);
        return ERR_ARG;
    }
    Plan* p = nullptr;
    int rc = get_plan(m, B, F, T, &p);
    if (rc != OK) return rc;
    const size_t state = (((size_t)B * F * T * 2 * sizeof(float)) + 255) & ~(size_t)255;     // one complex64 [B,1,F,T]
    rc = m->d_fm.reserve(2 * state + (size_t)fm_workspace_bytes(B, F, T), true);
    if (rc != OK) return rc;
    float* xt = reinterpret_cast<float*>(m->d_fm.p);
    float* v = reinterpret_cast<float*>(m->d_fm.p + state);
    double* partial = reinterpret_cast<double*>(m->d_fm.p + 2 * state);
    const float* x0f = static_cast<const float*>(x0);
    const float* yf = static_cast<const float*>(y);
    const float* zf = static_cast<const float*>(z);
    return on_handle_stream(m, stream, [&](hipStream_t s) {
        rc = launch_fm_pair(x0f, yf, t_dev, zf, keys_dev, seed, sigma_min, sigma_max, xt, nullptr, B, F, T, s);
        if (rc == OK) rc = launch_set_call(m->d_call, CallBlock{xt, yf, t_dev, v, 1, 0.f}, s);
        if (rc == OK) rc = exec_plan(m, p, s);
        if (rc == OK)
            rc = launch_fm_loss_rows(v, x0f, yf, zf, keys_dev, seed, sigma_min, sigma_max, loss_type == FLOWSE_LOSS_MAE,
                                     out, partial, B, F, T, s);
        return rc;
    });
}

}  // extern "C"
