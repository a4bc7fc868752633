// Rational-ratio polyphase FIR resampler, zero phase: what scipy.signal.resample_poly(x, up, down) computes with its
// defaults (window ("kaiser", 5.0), padtype "constant").  The reference has no resampler -- it reads 16 kHz files only
// (flowmse/data_module.py) -- so the definition is scipy's, restated here (include/flowse_hip.h):
//
//   g = gcd(up, down), up /= g, down /= g, R = max(up, down), half = 10 R
//   h[k] = up * firwin(2 half + 1, 1 / R, window = ("kaiser", 5.0))[k],  k = 0 .. 2 half
//   L_out = ceil(L up / down),  out[n] = sum_m x[m] h[half + n down - m up]  over  |n down - m up| <= half, 0 <= m < L
//
// Polyphase form: P = ceil((2 half + 1) / up) taps per output, table H[p][j] = h[p + j up] (zero past 2 half); with
// c = half + n down, p = c mod up, q = c div up:  out[n] = sum_{j < P} H[p][j] x[q - j], x zero outside [0, L).
// c passes 2^31 after 4.87 M outputs at down = 441 (five minutes of 44.1 kHz audio): c, q and every sample index are
// 64-bit, on the device and on the host.
#include <cmath>
#include <cstdio>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/flowse_hip.h"
#include "common.h"

namespace flowse {

static const int RESAMPLE_MAX_RATE = 1024;
static const int RESAMPLE_THREADS = 256;
static const int RESAMPLE_RUN = 1024;              // consecutive outputs of one row per block
static const int RESAMPLE_SPAN_LDS = 5120;         // floats: the largest input span a block stages (20 KiB)
static const int RESAMPLE_TABLE_LDS = 10240;       // floats: the largest polyphase table a block copies (40 KiB)

struct Ratio {
    int up, down, half, P;
};

static int gcd_int(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// reduce and check a ratio; the message names the caller
static int make_ratio(const char* who, int up, int down, Ratio* r) {
    if (up < 1 || down < 1) {
        set_error("%s: up and down must be positive, got %d / %d", who, up, down);
        return ERR_ARG;
    }
    const int g = gcd_int(up, down);
    up /= g;
    down /= g;
    const int R = up > down ? up : down;
    if (R > RESAMPLE_MAX_RATE) {
        set_error("%s: the reduced ratio %d / %d needs max(up, down) <= %d", who, up, down, RESAMPLE_MAX_RATE);
        return ERR_SHAPE;
    }
    r->up = up;
    r->down = down;
    r->half = 10 * R;
    r->P = (2 * r->half + up) / up;                // ceil((2 half + 1) / up)
    return OK;
}

// modified Bessel function I0 by its power series sum_k ((x / 2)^k / k!)^2 (x = 5 here, 5.65 in metrics.hip: 25 to 30 terms
// reach 1e-17); declared in common.h
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// up * firwin(2 half + 1, 1 / R, window = ("kaiser", 5.0)): the windowed sinc, scaled to unit gain at DC, times up
static void design_taps(const Ratio& r, double* h) {
    const int n = 2 * r.half + 1;
    const double cutoff = 1.0 / (double)(r.up > r.down ? r.up : r.down), beta = 5.0, i0b = bessel_i0(beta);
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double m = (double)(k - r.half);
        const double y = M_PI * (m == 0.0 ? 1e-20 : cutoff * m);   // numpy.sinc's guard at 0
        const double t = m / (double)r.half;
        h[k] = cutoff * (sin(y) / y) * (bessel_i0(beta * sqrt(fmax(0.0, 1.0 - t * t))) / i0b);
        sum += h[k];
    }
    for (int k = 0; k < n; ++k) h[k] = h[k] / sum * (double)r.up;
}

// One output: the fmaf chain over j = 0 .. P - 1 of h[j] x[q - j], from +0.f -- the one tap loop of both kernels below, so
// that a window's output is the whole signal's bit for bit.  X_LDS: `xq` points at x[q] in a staged span that holds
// x[q - (P - 1) .. q], zeros already written where the signal has no sample.  Otherwise `x` holds the samples [lo, hi) of
// the row (x[0] is sample lo) and every other sample is zero.
template <bool X_LDS>
__device__ __forceinline__ float resample_output(const float* h, int P, const float* xq, const float* __restrict__ x,
                                                 int64_t q, int64_t lo, int64_t hi) {
    float acc = 0.f;
    if (X_LDS) {
        for (int j = 0; j < P; ++j) acc = fmaf(h[j], xq[-j], acc);
    } else {
        for (int j = 0; j < P; ++j) {
            const int64_t m = q - j;
            acc = fmaf(h[j], m >= lo && m < hi ? x[m - lo] : 0.f, acc);
        }
    }
    return acc;
}

// A block owns `run` consecutive outputs of row blockIdx.y.  X_LDS: the input span they touch is staged once, zeros
// written for samples outside [0, L) -- otherwise (ratios whose span does not fit) each tap reads global memory behind the
// same bounds test.  H_LDS: the whole table is copied next to it -- otherwise rows of it are read through L2.
template <bool X_LDS, bool H_LDS>
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_poly_kernel(const float* __restrict__ sig,
                                                                         const float* __restrict__ H,
                                                                         float* __restrict__ out, int L, int L_out, int up,
                                                                         int down, int half, int P, int run, int span) {
    extern __shared__ float lds[];
    float* xs = lds;                               // [span] when X_LDS
    float* hs = lds + (X_LDS ? span : 0);          // [up][P] when H_LDS
    const float* x = sig + (int64_t)blockIdx.y * L;
    float* o = out + (int64_t)blockIdx.y * L_out;
    const int64_t n0 = (int64_t)blockIdx.x * run;
    const int64_t n1 = n0 + run < L_out ? n0 + run : (int64_t)L_out;
    const int64_t q_lo = ((int64_t)half + n0 * down) / up - (P - 1);      // the first sample the run touches
    if (X_LDS) {
        for (int i = threadIdx.x; i < span; i += RESAMPLE_THREADS) {
            const int64_t m = q_lo + i;
            xs[i] = m >= 0 && m < L ? x[m] : 0.f;
        }
    }
    if (H_LDS) {
        for (int i = threadIdx.x; i < up * P; i += RESAMPLE_THREADS) hs[i] = H[i];
    }
    if (X_LDS || H_LDS) __syncthreads();
    for (int64_t n = n0 + threadIdx.x; n < n1; n += RESAMPLE_THREADS) {
        const int64_t c = (int64_t)half + n * down;
        const int64_t q = c / up;
        const float* h = (H_LDS ? hs : H) + (int)(c - q * up) * P;
        const float* xq = xs + (int)(q - q_lo);                           // in [P - 1, span) when X_LDS
        o[n] = resample_output<X_LDS>(h, P, xq, x, q, 0, L);
    }
}

// The same outputs from a window of ONE row: `win` holds the samples [m0, m0 + n_win) of the signal, block `block` owns the
// `run` consecutive outputs from n0 + block * run on (below n0 + n_out), and out[0] is output n0.  The host has checked
// that every sample of the signal an output needs lies in the window, so a sample outside the window is a zero of the
// definition (below 0, or at or past the end of a closed signal).  Every index is 64-bit: m0, n0, c and q are absolute.
// The one body of both window kernels below: a row of the table entry is the single entry's row by construction.
template <bool X_LDS, bool H_LDS>
__device__ __forceinline__ void resample_window_block(const float* __restrict__ win, int64_t m0, int64_t n_win,
                                                      const float* __restrict__ H, float* __restrict__ out, int64_t n0,
                                                      int64_t n_out, int up, int down, int half, int P, int run, int span,
                                                      int64_t block) {
    extern __shared__ float lds[];
    float* xs = lds;                               // [span] when X_LDS
    float* hs = lds + (X_LDS ? span : 0);          // [up][P] when H_LDS
    const int64_t m1 = m0 + n_win;
    const int64_t na = n0 + block * run;
    const int64_t nb = na + run < n0 + n_out ? na + run : n0 + n_out;
    const int64_t q_lo = ((int64_t)half + na * down) / up - (P - 1);      // the first sample the run touches
    if (X_LDS) {
        for (int i = threadIdx.x; i < span; i += RESAMPLE_THREADS) {
            const int64_t m = q_lo + i;
            xs[i] = m >= m0 && m < m1 ? win[m - m0] : 0.f;
        }
    }
    if (H_LDS) {
        for (int i = threadIdx.x; i < up * P; i += RESAMPLE_THREADS) hs[i] = H[i];
    }
    if (X_LDS || H_LDS) __syncthreads();
    for (int64_t n = na + threadIdx.x; n < nb; n += RESAMPLE_THREADS) {
        const int64_t c = (int64_t)half + n * down;
        const int64_t q = c / up;
        const float* h = (H_LDS ? hs : H) + (int)(c - q * up) * P;
        const float* xq = xs + (int)(q - q_lo);                           // in [P - 1, span) when X_LDS
        out[n - n0] = resample_output<X_LDS>(h, P, xq, win, q, m0, m1);
    }
}

// grid (ceil(n_out / run)): the outputs [n0, n0 + n_out) of one row
template <bool X_LDS, bool H_LDS>
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_poly_window_kernel(const float* __restrict__ win, int64_t m0,
                                                                                int64_t n_win, const float* __restrict__ H,
                                                                                float* __restrict__ out, int64_t n0,
                                                                                int64_t n_out, int up, int down, int half,
                                                                                int P, int run, int span) {
    resample_window_block<X_LDS, H_LDS>(win, m0, n_win, H, out, n0, n_out, up, down, half, P, run, span, blockIdx.x);
}

// The windows of SEVERAL rows at one ratio (flowmse_amd.resample.flush): the descriptors travel by value in the argument
// block, as the window tables of spec.hip do, already checked on the host.
struct ResampleRow {
    const float* win;
    int64_t m0, n_win;
    float* out;
    int64_t n0, n_out;
};
struct ResampleRowTable {
    ResampleRow row[FLOWSE_MAX_RESAMPLE_ROWS];
};
static_assert(sizeof(flowse_resample_row) == 56 && sizeof(ResampleRow) == 48 && sizeof(ResampleRowTable) <= 2048,
              "the table must fit the argument block");

// grid (ceil(largest n_out of any row / run), R): a block past its row's outputs (every block of a row with n_out == 0)
// returns before it touches LDS; the test is uniform over the block, so no thread waits at the barrier for one that left
template <bool X_LDS, bool H_LDS>
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_poly_window_rows_kernel(const ResampleRowTable rows,
                                                                                     const float* __restrict__ H, int up,
                                                                                     int down, int half, int P, int run,
                                                                                     int span) {
    const ResampleRow& w = rows.row[blockIdx.y];
    if ((int64_t)blockIdx.x * run >= w.n_out) return;
    resample_window_block<X_LDS, H_LDS>(w.win, w.m0, w.n_win, H, w.out, w.n0, w.n_out, up, down, half, P, run, span,
                                        blockIdx.x);
}

// the fp32 polyphase table of a reduced ratio on one device: built once per process and device, uploaded on the stream of
// the call that needs it first; `ready` orders calls on other streams behind that upload.  That first call designs the
// taps on the host and copies from pageable memory, which the runtime stages and may wait for, and it records `ready`:
// it must not be made while its stream is being captured.  Every later call for the ratio only enqueues.
struct ResampleTable {
    std::vector<float> host;                       // kept: the source of an asynchronous copy
    float* dev = nullptr;
    hipEvent_t ready = nullptr;
};
static std::mutex g_tables_mutex;
static std::map<std::pair<int, std::pair<int, int>>, ResampleTable> g_tables;

static int get_table(const Ratio& r, hipStream_t s, const float** dev) {
    int device = 0;
    FLOWSE_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_tables_mutex);
    ResampleTable& t = g_tables[std::make_pair(device, std::make_pair(r.up, r.down))];
    if (!t.dev) {
        std::vector<double> h(2 * r.half + 1);
        design_taps(r, h.data());
        t.host.assign((size_t)r.up * r.P, 0.f);
        for (int k = 0; k <= 2 * r.half; ++k) t.host[(size_t)(k % r.up) * r.P + k / r.up] = (float)h[k];
        float* d = nullptr;
        FLOWSE_HIP(hipMalloc(reinterpret_cast<void**>(&d), t.host.size() * sizeof(float)));
        hipError_t e = hipEventCreateWithFlags(&t.ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemcpyAsync(d, t.host.data(), t.host.size() * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(t.ready, s);
        if (e != hipSuccess) {
            if (t.ready) (void)hipEventDestroy(t.ready);
            t.ready = nullptr;
            (void)hipFree(d);
            return hip_fail(e, "resample table upload", __FILE__, __LINE__);
        }
        t.dev = d;
    }
    FLOWSE_HIP(hipStreamWaitEvent(s, t.ready, 0));
    *dev = t.dev;
    return OK;
}

template <bool X_LDS, bool H_LDS>
static void launch_one(dim3 grid, size_t lds_bytes, hipStream_t s, const float* sig, const float* H, float* out, int L,
                       int L_out, const Ratio& r, int run, int span) {
    hipLaunchKernelGGL((resample_poly_kernel<X_LDS, H_LDS>), grid, dim3(RESAMPLE_THREADS), lds_bytes, s, sig, H, out, L, L_out,
                       r.up, r.down, r.half, r.P, run, span);
}

template <bool X_LDS, bool H_LDS>
static void launch_window(dim3 grid, size_t lds_bytes, hipStream_t s, const float* win, int64_t m0, int64_t n_win,
                          const float* H, float* out, int64_t n0, int64_t n_out, const Ratio& r, int run, int span) {
    hipLaunchKernelGGL((resample_poly_window_kernel<X_LDS, H_LDS>), grid, dim3(RESAMPLE_THREADS), lds_bytes, s, win, m0, n_win,
                       H, out, n0, n_out, r.up, r.down, r.half, r.P, run, span);
}

template <bool X_LDS, bool H_LDS>
static void launch_window_rows(dim3 grid, size_t lds_bytes, hipStream_t s, const ResampleRowTable& t, const float* H,
                               const Ratio& r, int run, int span) {
    hipLaunchKernelGGL((resample_poly_window_rows_kernel<X_LDS, H_LDS>), grid, dim3(RESAMPLE_THREADS), lds_bytes, s, t, H, r.up,
                       r.down, r.half, r.P, run, span);
}

// The form of a launch, one test for all entries: the outputs per block, and what of the input span and the table a
// block holds in LDS.
struct LaunchForm {
    int run, span;
    bool x_lds, h_lds;
    size_t lds_bytes;
};

static LaunchForm launch_form(const Ratio& r) {
    // the span of a run: q moves by at most ceil((run - 1) down / up) over it, and every output reaches P - 1 back
    auto span_of = [&](int run) { return ((int64_t)(run - 1) * r.down + r.up - 1) / r.up + r.P; };
    LaunchForm f;
    f.run = RESAMPLE_RUN;
    if (span_of(f.run) > RESAMPLE_SPAN_LDS) f.run = RESAMPLE_THREADS;
    f.x_lds = span_of(f.run) <= RESAMPLE_SPAN_LDS;
    f.h_lds = r.up * r.P <= RESAMPLE_TABLE_LDS;
    f.span = f.x_lds ? (int)span_of(f.run) : 0;
    f.lds_bytes = ((size_t)f.span + (f.h_lds ? (size_t)r.up * r.P : 0)) * sizeof(float);
    return f;
}

// The checks of one window, for the single entry and for every row of the table entry (`who` names the entry, and the
// row): nothing is enqueued before they pass.  The reduced ratio comes back in *ratio.
static int check_window(const char* who, const float* win, int64_t m0, int64_t n_win, int64_t L_total, int up, int down,
                        const float* out, int64_t n0, int64_t n_out, Ratio* ratio) {
    if (!win || !out || m0 < 0 || n_win < 0 || n0 < 0 || n_out < 0 || L_total < -1) {
        set_error("%s: null pointer or a negative count (m0 %lld, n_win %lld, L_total %lld, n0 %lld, n_out %lld)", who,
                  (long long)m0, (long long)n_win, (long long)L_total, (long long)n0, (long long)n_out);
        return ERR_ARG;
    }
    if (const int rc = make_ratio(who, up, down, ratio)) return rc;
    const Ratio& r = *ratio;
    const int64_t reach = (int64_t)1 << 50;        // every product below stays inside 64 bits (up, down <= 2^10)
    if (m0 > reach || n_win > reach || n0 > reach || L_total > reach || n_out > 0x7fffffff) {
        set_error("%s: m0 %lld, n_win %lld, n0 %lld and L_total %lld may reach 2^50, n_out %lld 2^31 - 1", who, (long long)m0,
                  (long long)n_win, (long long)n0, (long long)L_total, (long long)n_out);
        return ERR_SHAPE;
    }
    const int64_t m1 = m0 + n_win, n1 = n0 + n_out;
    if (L_total >= 0) {
        const int64_t L_out = (L_total * r.up + r.down - 1) / r.down;
        if (m1 > L_total || n1 > L_out) {
            set_error("%s: a signal of %lld samples has %lld outputs at %d / %d; the window [%lld, %lld) or the outputs "
                      "[%lld, %lld) pass its end", who, (long long)L_total, (long long)L_out, r.up, r.down, (long long)m0,
                      (long long)m1, (long long)n0, (long long)n1);
            return ERR_SHAPE;
        }
    }
    if (n_out == 0) return OK;
    if (r.up == r.down) {                          // out[n] = x[n]: the slice [n0, n1) of the window
        if (n0 < m0 || n1 > m1) {
            set_error("%s: at %d / %d the outputs [%lld, %lld) are those samples; the window holds [%lld, %lld)", who, r.up,
                      r.down, (long long)n0, (long long)n1, (long long)m0, (long long)m1);
            return ERR_SHAPE;
        }
        return OK;
    }
    // what the outputs read: x[q(n0) - (P - 1) .. q(n1 - 1)], all P taps of each (a table entry past 2 half is a zero
    // that still multiplies its sample), clamped to the signal
    const int64_t q_first = ((int64_t)r.half + n0 * r.down) / r.up, q_last = ((int64_t)r.half + (n1 - 1) * r.down) / r.up;
    if (L_total < 0 && q_last >= m1) {
        set_error("%s: output %lld of an open signal reads sample %lld, the window [%lld, %lld) ends before it (has it "
                  "arrived?)", who, (long long)(n1 - 1), (long long)q_last, (long long)m0, (long long)m1);
        return ERR_SHAPE;
    }
    const int64_t need_lo = q_first - (r.P - 1) > 0 ? q_first - (r.P - 1) : 0;
    const int64_t need_hi = L_total >= 0 && q_last > L_total - 1 ? L_total - 1 : q_last;       // inclusive
    if (need_lo < m0 || need_hi >= m1) {
        set_error("%s: the outputs [%lld, %lld) at %d / %d read the samples [%lld, %lld], the window holds [%lld, %lld)", who,
                  (long long)n0, (long long)n1, r.up, r.down, (long long)need_lo, (long long)need_hi, (long long)m0,
                  (long long)m1);
        return ERR_SHAPE;
    }
    return OK;
}

}  // namespace flowse

using namespace flowse;

extern "C" {

int flowse_resample_num_taps(int up, int down) {
    Ratio r;
    const int rc = make_ratio("flowse_resample_num_taps", up, down, &r);
    return rc != OK ? -rc : 2 * r.half + 1;
}

int flowse_resample_taps(int up, int down, double* taps, int cap) {
    Ratio r;
    if (const int rc = make_ratio("flowse_resample_taps", up, down, &r)) return rc;
    if (!taps || cap < 2 * r.half + 1) {
        set_error("flowse_resample_taps: %d / %d has %d taps, the buffer holds %d", r.up, r.down, 2 * r.half + 1,
                  taps ? cap : 0);
        return ERR_ARG;
    }
    design_taps(r, taps);
    return OK;
}

int flowse_resample_poly(const float* sig, int B, int L, int up, int down, float* out, int L_out, void* stream) {
    if (!sig || !out || B < 1 || L < 1) {
        set_error("flowse_resample_poly: null pointer or B / L < 1 (B %d, L %d)", B, L);
        return ERR_ARG;
    }
    Ratio r;
    if (const int rc = make_ratio("flowse_resample_poly", up, down, &r)) return rc;
    const int64_t want = ((int64_t)L * r.up + r.down - 1) / r.down;
    if (L_out != want) {
        set_error("flowse_resample_poly: %d samples at %d / %d give %lld per row, got L_out %d", L, r.up, r.down,
                  (long long)want, L_out);
        return ERR_SHAPE;
    }
    if (B > 65535) {
        set_error("flowse_resample_poly: at most 65535 rows in one call (a row is a grid row), got B %d", B);
        return ERR_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (r.up == r.down) {
        FLOWSE_HIP(hipMemcpyAsync(out, sig, (size_t)B * L * sizeof(float), hipMemcpyDeviceToDevice, s));
        return OK;
    }
    const float* H = nullptr;
    if (const int rc = get_table(r, s, &H)) return rc;
    const LaunchForm f = launch_form(r);
    const dim3 grid((unsigned)(((int64_t)L_out + f.run - 1) / f.run), (unsigned)B);
    if (f.x_lds && f.h_lds) launch_one<true, true>(grid, f.lds_bytes, s, sig, H, out, L, L_out, r, f.run, f.span);
    else if (f.x_lds) launch_one<true, false>(grid, f.lds_bytes, s, sig, H, out, L, L_out, r, f.run, f.span);
    else if (f.h_lds) launch_one<false, true>(grid, f.lds_bytes, s, sig, H, out, L, L_out, r, f.run, f.span);
    else launch_one<false, false>(grid, f.lds_bytes, s, sig, H, out, L, L_out, r, f.run, f.span);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_resample_poly_window(const float* win, int64_t m0, int64_t n_win, int64_t L_total, int up, int down, float* out,
                                int64_t n0, int64_t n_out, void* stream) {
    const char* who = "flowse_resample_poly_window";
    Ratio r;
    if (const int rc = check_window(who, win, m0, n_win, L_total, up, down, out, n0, n_out, &r)) return rc;
    if (n_out == 0) return OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (r.up == r.down) {                          // out[n] = x[n]: the slice [n0, n0 + n_out) of the window
        FLOWSE_HIP(hipMemcpyAsync(out, win + (n0 - m0), (size_t)n_out * sizeof(float), hipMemcpyDeviceToDevice, s));
        return OK;
    }
    const float* H = nullptr;
    if (const int rc = get_table(r, s, &H)) return rc;
    const LaunchForm f = launch_form(r);
    const dim3 grid((unsigned)((n_out + f.run - 1) / f.run));
    if (f.x_lds && f.h_lds) launch_window<true, true>(grid, f.lds_bytes, s, win, m0, n_win, H, out, n0, n_out, r, f.run, f.span);
    else if (f.x_lds) launch_window<true, false>(grid, f.lds_bytes, s, win, m0, n_win, H, out, n0, n_out, r, f.run, f.span);
    else if (f.h_lds) launch_window<false, true>(grid, f.lds_bytes, s, win, m0, n_win, H, out, n0, n_out, r, f.run, f.span);
    else launch_window<false, false>(grid, f.lds_bytes, s, win, m0, n_win, H, out, n0, n_out, r, f.run, f.span);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_resample_poly_window_rows(const flowse_resample_row* rows, int R, int up, int down, void* stream) {
    if (!rows) {
        set_error("flowse_resample_poly_window_rows: null table");
        return ERR_ARG;
    }
    if (R < 1 || R > FLOWSE_MAX_RESAMPLE_ROWS) {
        set_error("flowse_resample_poly_window_rows: need 1 <= R <= %d (got R=%d)", FLOWSE_MAX_RESAMPLE_ROWS, R);
        return ERR_SHAPE;
    }
    // every row passes the single entry's checks before anything is enqueued
    Ratio r;
    ResampleRowTable t;
    char who[64];
    int64_t longest = 0;
    for (int i = 0; i < R; ++i) {
        const flowse_resample_row& w = rows[i];
        snprintf(who, sizeof(who), "flowse_resample_poly_window_rows: row %d", i);
        if (const int rc = check_window(who, w.win, w.m0, w.n_win, w.L_total, up, down, w.out, w.n0, w.n_out, &r)) return rc;
        t.row[i] = ResampleRow{w.win, w.m0, w.n_win, w.out, w.n0, w.n_out};
        if (w.n_out > longest) longest = w.n_out;
    }
    for (int i = R; i < FLOWSE_MAX_RESAMPLE_ROWS; ++i) t.row[i] = t.row[0];    // never read: the grid has R rows
    if (longest == 0) return OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (r.up == r.down) {                          // per row the single entry's copy
        for (int i = 0; i < R; ++i) {
            const ResampleRow& w = t.row[i];
            if (w.n_out == 0) continue;
            FLOWSE_HIP(hipMemcpyAsync(w.out, w.win + (w.n0 - w.m0), (size_t)w.n_out * sizeof(float), hipMemcpyDeviceToDevice,
                                      s));
        }
        return OK;
    }
    const float* H = nullptr;
    if (const int rc = get_table(r, s, &H)) return rc;
    const LaunchForm f = launch_form(r);
    const dim3 grid((unsigned)((longest + f.run - 1) / f.run), (unsigned)R);
    if (f.x_lds && f.h_lds) launch_window_rows<true, true>(grid, f.lds_bytes, s, t, H, r, f.run, f.span);
    else if (f.x_lds) launch_window_rows<true, false>(grid, f.lds_bytes, s, t, H, r, f.run, f.span);
    else if (f.h_lds) launch_window_rows<false, true>(grid, f.lds_bytes, s, t, H, r, f.run, f.span);
    else launch_window_rows<false, false>(grid, f.lds_bytes, s, t, H, r, f.run, f.span);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
