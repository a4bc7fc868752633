// Adaptive Dormand-Prince 5(4) sampler (flowse_rk45_sample, include/flowse_hip.h): the reference's black-box sampler
// (flowmse/sampling/__init__.py:64-114, scipy.integrate.solve_ivp(method="RK45")) with the state on the device.
//
// The controller below is a line-by-line port of scipy 1.15's RungeKutta._step_impl, rk_step, select_initial_step and
// OdeSolver.step (scipy/integrate/_ivp/{rk,common,base}.py); every scalar is a double, as in scipy.  The device holds
// what scipy holds: y, y_new in complex128 (scipy promotes the complex64 start state), the slopes K1..K7 in complex64
// (each one is a network output: the complex128 copy scipy keeps is exact), and the complex64 stage input the reference
// hands the network (`.type(torch.complex64)` in ode_func).  The elementwise arithmetic repeats numpy's:
//   - np.dot(K[:s].T, a) is an OpenBLAS zgemv over columns in blocks of 4, 2, 1: each block is a fused multiply-add
//     chain started by a plain product, blocks are added in order (dot_blas below; measured bit for bit against
//     numpy 2 / OpenBLAS 0.3.29 for every row of the tableau).  A product with the zero imaginary part of a real
//     coefficient is an exact zero, so the real and imaginary parts are two independent real dot products;
//   - everything else is one IEEE operation per numpy operation, in numpy's order, with contraction off;
//   - the RMS norm (np.linalg.norm(x) / sqrt(x.size), = sqrt(sum re^2 + sum im^2) / sqrt(n)) sums in a fixed
//     partition and order (no atomics): two identical solves take bitwise identical step sequences.  Its summation
//     order is the one difference to numpy (~1e-16 relative).
#include "model.h"

#pragma clang fp contract(off)

namespace flowse {
namespace {

constexpr int NORM_THREADS = 256;
constexpr int NORM_BLOCKS = 1024;          // fixed partition of every norm: min(NORM_BLOCKS, ceil(n / 256)) partial sums

// scipy.integrate._ivp.rk.RK45 (the literals evaluate to the same correctly rounded doubles as Python's true division)
constexpr double RK_C[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
constexpr double RK_A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
constexpr double RK_B[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
constexpr double RK_E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;
constexpr double ERROR_EXPONENT = -1.0 / 5;   // -1 / (error_estimator_order + 1)

struct Slopes { const float2* k[7]; };
struct Coefs { double c[7]; };

// np.dot of S columns with real coefficients (see the file comment)
template <int S>
__device__ __forceinline__ double dot_blas(const double* k, const double* a) {
    double y = 0.0;
    int j = 0;
#pragma unroll
    for (; j + 4 <= S; j += 4) {
        double t = k[j] * a[j];
        t = fma(k[j + 1], a[j + 1], t);
        t = fma(k[j + 2], a[j + 2], t);
        t = fma(k[j + 3], a[j + 3], t);
        y = j == 0 ? t : y + t;
    }
    if (S - j >= 2) {
        const double t = fma(k[j + 1], a[j + 1], k[j] * a[j]);
        y = j == 0 ? t : y + t;
        j += 2;
    }
    if (S - j == 1) {
        const double t = k[j] * a[j];
        y = j == 0 ? t : y + t;
    }
    return y;
}

template <int S>
__device__ __forceinline__ void load_slopes(const Slopes& K, int64_t i, double* kr, double* ki) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const float2 v = K.k[j][i];
        kr[j] = v.x;
        ki[j] = v.y;
    }
}

__device__ __forceinline__ float2 to_c64(double re, double im) { return make_float2((float)re, (float)im); }

// np.abs of a complex128 (npy_hypot)
__device__ __forceinline__ double cabs(double2 v) { return hypot(v.x, v.y); }

// np.maximum: a NaN operand propagates
__device__ __forceinline__ double np_maximum(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    return a >= b ? a : b;
}

// y <- complex128(x)                                       (OdeSolver.__init__: y0.astype(complex))
__global__ __launch_bounds__(256) void dp_init_kernel(const float2* __restrict__ x, double2* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float2 v = x[i];
        y[i] = make_double2(v.x, v.y);
    }
}

// x <- complex64(y)                   (torch.tensor(solution.y[:, -1]).type(torch.complex64))
__global__ __launch_bounds__(256) void dp_output_kernel(const double2* __restrict__ y, float2* __restrict__ x, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double2 v = y[i];
        x[i] = to_c64(v.x, v.y);
    }
}

// Stage input of rk_step: xs = complex64(y + np.dot(K[:S].T, a) * h).  With S = 1 and a = {1} it is also the probe
// of select_initial_step, y1 = y0 + (h0 * direction) * f0.  y_new != null: the solution
// y_new = y + h * np.dot(K[:6].T, B) (same value: one product each way), kept in complex128 and also cast for f_new.
template <int S>
__global__ __launch_bounds__(256) void dp_combine_kernel(const double2* __restrict__ y, Slopes K, Coefs a, double h,
                                                         double2* __restrict__ y_new, float2* __restrict__ xs, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double kr[S], ki[S];
        load_slopes<S>(K, i, kr, ki);
        const double dr = dot_blas<S>(kr, a.c) * h;
        const double di = dot_blas<S>(ki, a.c) * h;
        const double2 yy = y[i];
        const double zr = yy.x + dr, zi = yy.y + di;
        if (y_new) y_new[i] = make_double2(zr, zi);
        xs[i] = to_c64(zr, zi);
    }
}

// Per-block partial sums (sum (re/scale)^2, sum (im/scale)^2) of the vector whose RMS norm scipy takes:
//   NRM_Y0:  y0 / scale,              scale = atol + |y0| * rtol           (select_initial_step: d0)
//   NRM_F0:  f0 / scale                                                   (d1)
//   NRM_DF:  (f1 - f0) / scale                                            (d2 * h0)
//   NRM_ERR: (np.dot(K.T, E) * h) / scale,  scale = atol + np.maximum(|y|, |y_new|) * rtol   (_estimate_error_norm)
// Dividing a complex128 by a real scale divides both parts (numpy's Smith division with a zero imaginary divisor).
enum { NRM_Y0 = 0, NRM_F0 = 1, NRM_DF = 2, NRM_ERR = 3 };

__device__ __forceinline__ void block_sum2(double& sr, double& si, double2* __restrict__ out) {
    __shared__ double lr[NORM_THREADS], li[NORM_THREADS];
    lr[threadIdx.x] = sr;
    li[threadIdx.x] = si;
    __syncthreads();
#pragma unroll
    for (int w = NORM_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            lr[threadIdx.x] = lr[threadIdx.x] + lr[threadIdx.x + w];
            li[threadIdx.x] = li[threadIdx.x] + li[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = make_double2(lr[0], li[0]);
}

template <int MODE>
__global__ __launch_bounds__(NORM_THREADS) void dp_norm_partials_kernel(const double2* __restrict__ y,
                                                                        const double2* __restrict__ y_new, Slopes K,
                                                                        Coefs e, double h, double rtol, double atol,
                                                                        int64_t n, double2* __restrict__ part) {
    double sr = 0.0, si = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * NORM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NORM_THREADS) {
        const double2 yy = y[i];
        double scale, vr, vi;
        if (MODE == NRM_ERR) {
            scale = atol + np_maximum(cabs(yy), cabs(y_new[i])) * rtol;
            double kr[7], ki[7];
            load_slopes<7>(K, i, kr, ki);
            vr = dot_blas<7>(kr, e.c) * h;
            vi = dot_blas<7>(ki, e.c) * h;
        } else {
            scale = atol + cabs(yy) * rtol;
            if (MODE == NRM_Y0) {
                vr = yy.x;
                vi = yy.y;
            } else if (MODE == NRM_F0) {
                const float2 f0 = K.k[0][i];
                vr = f0.x;
                vi = f0.y;
            } else {
                const float2 f0 = K.k[0][i], f1 = K.k[1][i];
                vr = (double)f1.x - (double)f0.x;
                vi = (double)f1.y - (double)f0.y;
            }
        }
        const double qr = vr / scale, qi = vi / scale;
        sr = sr + qr * qr;
        si = si + qi * qi;
    }
    block_sum2(sr, si, part + blockIdx.x);
}

// out[0] = sqrt(sum re^2 + sum im^2) / sqrt(n) over the partials, in a fixed order
__global__ __launch_bounds__(NORM_THREADS) void dp_norm_final_kernel(const double2* __restrict__ part, int nparts,
                                                                     double sqrt_n, double* __restrict__ out) {
    double sr = 0.0, si = 0.0;
    for (int i = threadIdx.x; i < nparts; i += NORM_THREADS) {
        const double2 v = part[i];
        sr = sr + v.x;
        si = si + v.y;
    }
    __shared__ double2 tot;
    block_sum2(sr, si, &tot);
    __syncthreads();
    if (threadIdx.x == 0) out[0] = sqrt(tot.x + tot.y) / sqrt_n;
}

int grid_of(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (int)(g < 4096 ? (g > 0 ? g : 1) : 4096);
}

// Python's min(a, b) / max(a, b): the first argument unless the second compares smaller / larger (so NaN never wins
// as the second argument: max(0.2, nan) == 0.2)
double py_min(double a, double b) { return b < a ? b : a; }
double py_max(double a, double b) { return b > a ? b : a; }

// Device state of one solve, carved out of the handle's d_rk45 buffer.
struct Rk45State {
    double2 *y, *y_new;
    float2* k[7];          // slot j holds K_j of the current step (FSAL: slot pointers rotate, nothing is copied)
    float2* xs;            // network input of the next evaluation
    double2* part;
    double* norm;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t rk45_bytes(int64_t n) {
    return 2 * align256(16 * (size_t)n) + 8 * align256(8 * (size_t)n) + align256(16 * NORM_BLOCKS) + 256;
}

Rk45State carve(char* base, int64_t n) {
    Rk45State st;
    size_t off = 0;
    auto take = [&](size_t b) { char* p = base + off; off += align256(b); return p; };
    st.y = reinterpret_cast<double2*>(take(16 * (size_t)n));
    st.y_new = reinterpret_cast<double2*>(take(16 * (size_t)n));
    for (int j = 0; j < 7; ++j) st.k[j] = reinterpret_cast<float2*>(take(8 * (size_t)n));
    st.xs = reinterpret_cast<float2*>(take(8 * (size_t)n));
    st.part = reinterpret_cast<double2*>(take(16 * NORM_BLOCKS));
    st.norm = reinterpret_cast<double*>(take(8));
    return st;
}

template <int S>
int launch_combine(const Rk45State& st, const double* a, double h, bool solution, int64_t n, hipStream_t s) {
    Slopes K{};
    Coefs c{};
    for (int j = 0; j < S; ++j) {
        K.k[j] = st.k[j];
        c.c[j] = a[j];
    }
    hipLaunchKernelGGL(dp_combine_kernel<S>, dim3(grid_of(n)), dim3(256), 0, s, st.y, K, c, h,
                       solution ? st.y_new : nullptr, st.xs, n);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // namespace
}  // namespace flowse

extern "C" int flowse_rk45_sample(flowse_model* m, void* x_inout, const void* y, double t0, double t_bound, double rtol,
                                  double atol, double first_step, double max_step, int64_t max_nfev, int B, int F,
                                  int T, int64_t* nfev_out, int* status_out, double* t_accepted, int t_cap,
                                  int* n_accepted, void* stream) {
    using namespace flowse;
    const double interval_length = std::fabs(t_bound - t0);
    if (!m || !x_inout || !y || !nfev_out || !status_out || !n_accepted || (t_cap > 0 && !t_accepted) || t_cap < 0 ||
        !std::isfinite(t0) || !std::isfinite(t_bound) || !(rtol > 0) || !(atol >= 0) || !(max_step > 0) ||
        first_step > interval_length || max_nfev < 1) {
        set_error("flowse_rk45_sample: bad argument (null pointer, t0 / t_bound not finite, rtol <= 0, atol < 0, "
                  "max_step <= 0, first_step beyond the interval, or max_nfev < 1)");
        return ERR_ARG;
    }
    Plan* p = nullptr;
    int rc = get_plan(m, B, F, T, &p);
    if (rc != OK) return rc;
    const int64_t n = (int64_t)B * F * T;                        // complex elements of the state
    rc = m->d_ts.reserve((size_t)B, true);
    if (rc == OK) rc = m->d_rk45.reserve(rk45_bytes(n), true);
    if (rc != OK) return rc;
    Rk45State st = carve(m->d_rk45, n);
    hipStream_t s = nullptr;                                     // the stream scope at the end sets it, then runs solve()

    const float* const yy = static_cast<const float*>(y);
    float2* const x = static_cast<float2*>(x_inout);
    const double sqrt_n = std::sqrt((double)n);
    const int nparts = (int)std::min<int64_t>(NORM_BLOCKS, (n + NORM_THREADS - 1) / NORM_THREADS);
    int64_t nfev = 0;
    int nacc = 0, status = 0;

    // fun(t, y): ones(B) * t rounds the double time to float (the times reach the device by value); VF = -dnn
    auto fun = [&](double t, const float2* in, float2* out) -> int {
        const float tf = (float)t;
        int r = launch_fill_times(m->d_ts, &tf, 1, B, s);
        CallBlock cb{reinterpret_cast<const float*>(in), yy, m->d_ts, reinterpret_cast<float*>(out), 1, 0.f};
        if (r == OK) r = launch_set_call(m->d_call, cb, s);
        if (r == OK) r = exec_plan(m, p, s);
        ++nfev;
        return r;
    };
    // norm(...) of common.py; the one host synchronisation: an 8-byte read per norm
    auto norm = [&](int mode, double h, double* out) -> int {
        Slopes K{};
        Coefs e{};
        for (int j = 0; j < 7; ++j) {
            K.k[j] = st.k[j];
            e.c[j] = RK_E[j];
        }
        switch (mode) {
            case NRM_Y0: hipLaunchKernelGGL(dp_norm_partials_kernel<NRM_Y0>, dim3(nparts), dim3(NORM_THREADS), 0, s,
                                            st.y, st.y_new, K, e, h, rtol, atol, n, st.part); break;
            case NRM_F0: hipLaunchKernelGGL(dp_norm_partials_kernel<NRM_F0>, dim3(nparts), dim3(NORM_THREADS), 0, s,
                                            st.y, st.y_new, K, e, h, rtol, atol, n, st.part); break;
            case NRM_DF: hipLaunchKernelGGL(dp_norm_partials_kernel<NRM_DF>, dim3(nparts), dim3(NORM_THREADS), 0, s,
                                            st.y, st.y_new, K, e, h, rtol, atol, n, st.part); break;
            default: hipLaunchKernelGGL(dp_norm_partials_kernel<NRM_ERR>, dim3(nparts), dim3(NORM_THREADS), 0, s,
                                        st.y, st.y_new, K, e, h, rtol, atol, n, st.part); break;
        }
        FLOWSE_LAUNCH_CHECK();
        hipLaunchKernelGGL(dp_norm_final_kernel, dim3(1), dim3(NORM_THREADS), 0, s, st.part, nparts, sqrt_n, st.norm);
        FLOWSE_LAUNCH_CHECK();
        FLOWSE_HIP(hipMemcpyAsync(out, st.norm, sizeof(double), hipMemcpyDeviceToHost, s));
        FLOWSE_HIP(hipStreamSynchronize(s));
        return OK;
    };

    auto solve = [&]() -> int {
        // OdeSolver.__init__ / RungeKutta.__init__
        const double direction = t_bound != t0 ? (t_bound - t0 > 0 ? 1.0 : -1.0) : 1.0;
        hipLaunchKernelGGL(dp_init_kernel, dim3(grid_of(n)), dim3(256), 0, s, x, st.y, n);
        FLOWSE_LAUNCH_CHECK();
        int r = fun(t0, x, st.k[0]);                              // self.f (complex64(y0) == x)
        if (r != OK) return r;
        double h_abs_state;
        if (first_step > 0) {
            h_abs_state = first_step;                            // validate_first_step
        } else if (interval_length == 0.0) {                     // select_initial_step
            h_abs_state = 0.0;
        } else {
            double d0, d1, d2;
            if ((r = norm(NRM_Y0, 0.0, &d0)) != OK) return r;
            if ((r = norm(NRM_F0, 0.0, &d1)) != OK) return r;
            double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
            h0 = py_min(h0, interval_length);
            const double one = 1.0;
            if ((r = launch_combine<1>(st, &one, h0 * direction, false, n, s)) != OK) return r;
            if ((r = fun(t0 + h0 * direction, st.xs, st.k[1])) != OK) return r;
            if ((r = norm(NRM_DF, 0.0, &d2)) != OK) return r;
            d2 = d2 / h0;
            double h1;
            if (d1 <= 1e-15 && d2 <= 1e-15) h1 = py_max(1e-6, h0 * 1e-3);
            else h1 = std::pow(0.01 / py_max(d1, d2), 1.0 / 5);
            h_abs_state = py_min(py_min(py_min(100 * h0, h1), interval_length), max_step);
        }

        double t = t0;
        for (;;) {
            // OdeSolver.step
            if (t == t_bound) {
                t = t_bound;
                if (nacc < t_cap) t_accepted[nacc] = t;
                ++nacc;
                status = 0;
                return OK;
            }
            // RungeKutta._step_impl
            const double min_step = 10 * std::fabs(std::nextafter(t, direction * INFINITY) - t);
            double h_abs = h_abs_state > max_step ? max_step : h_abs_state < min_step ? min_step : h_abs_state;
            bool step_accepted = false, step_rejected = false;
            double t_new = t;
            while (!step_accepted) {
                if (h_abs < min_step) {
                    status = -1;                                 // TOO_SMALL_STEP
                    return OK;
                }
                if (nfev + 6 > max_nfev) {
                    status = -2;
                    return OK;
                }
                double h = h_abs * direction;
                t_new = t + h;
                if (direction * (t_new - t_bound) > 0) t_new = t_bound;
                h = t_new - t;
                h_abs = std::fabs(h);
                // rk_step
                if ((r = launch_combine<1>(st, RK_A[1], h, false, n, s)) != OK) return r;
                if ((r = fun(t + RK_C[1] * h, st.xs, st.k[1])) != OK) return r;
                if ((r = launch_combine<2>(st, RK_A[2], h, false, n, s)) != OK) return r;
                if ((r = fun(t + RK_C[2] * h, st.xs, st.k[2])) != OK) return r;
                if ((r = launch_combine<3>(st, RK_A[3], h, false, n, s)) != OK) return r;
                if ((r = fun(t + RK_C[3] * h, st.xs, st.k[3])) != OK) return r;
                if ((r = launch_combine<4>(st, RK_A[4], h, false, n, s)) != OK) return r;
                if ((r = fun(t + RK_C[4] * h, st.xs, st.k[4])) != OK) return r;
                if ((r = launch_combine<5>(st, RK_A[5], h, false, n, s)) != OK) return r;
                if ((r = fun(t + RK_C[5] * h, st.xs, st.k[5])) != OK) return r;
                if ((r = launch_combine<6>(st, RK_B, h, true, n, s)) != OK) return r;
                if ((r = fun(t + h, st.xs, st.k[6])) != OK) return r;
                double error_norm;
                if ((r = norm(NRM_ERR, h, &error_norm)) != OK) return r;
                if (error_norm < 1) {
                    double factor = error_norm == 0 ? MAX_FACTOR
                                                    : py_min(MAX_FACTOR, SAFETY * std::pow(error_norm, ERROR_EXPONENT));
                    if (step_rejected) factor = py_min(1, factor);
                    h_abs *= factor;
                    step_accepted = true;
                } else {
                    // a NaN norm fails `< 1` and max(MIN_FACTOR, nan) == MIN_FACTOR: the step shrinks to TOO_SMALL_STEP
                    h_abs *= py_max(MIN_FACTOR, SAFETY * std::pow(error_norm, ERROR_EXPONENT));
                    step_rejected = true;
                }
            }
            t = t_new;
            std::swap(st.y, st.y_new);
            h_abs_state = h_abs;
            std::swap(st.k[0], st.k[6]);                         // self.f = f_new (FSAL)
            if (nacc < t_cap) t_accepted[nacc] = t;
            ++nacc;
            if (direction * (t - t_bound) >= 0) {
                status = 0;
                return OK;
            }
        }
    };

    return on_handle_stream(m, stream, [&](hipStream_t work) {
        s = work;
        rc = solve();
        if (rc == OK) {
            hipLaunchKernelGGL(dp_output_kernel, dim3(grid_of(n)), dim3(256), 0, s, st.y, x, n);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) rc = hip_fail(e, "kernel launch", __FILE__, __LINE__);
        }
        *nfev_out = nfev;
        *status_out = status;
        *n_accepted = nacc;
        return rc;
    });
}
