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
        float acc = 0.f;
        if (X_LDS) {
            const float* xq = xs + (int)(q - q_lo);                       // in [P - 1, span)
            for (int j = 0; j < P; ++j) acc = fmaf(h[j], xq[-j], acc);
        } else {
            for (int j = 0; j < P; ++j) {
                const int64_t m = q - j;
                acc = fmaf(h[j], m >= 0 && m < L ? x[m] : 0.f, acc);
            }
        }
        o[n] = acc;
    }
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
    // the span of a run: q moves by at most ceil((run - 1) down / up) over it, and every output reaches P - 1 back
    auto span_of = [&](int run) { return ((int64_t)(run - 1) * r.down + r.up - 1) / r.up + r.P; };
    int run = RESAMPLE_RUN;
    if (span_of(run) > RESAMPLE_SPAN_LDS) run = RESAMPLE_THREADS;
    const bool x_lds = span_of(run) <= RESAMPLE_SPAN_LDS, h_lds = r.up * r.P <= RESAMPLE_TABLE_LDS;
    const int span = x_lds ? (int)span_of(run) : 0;
    const size_t lds_bytes = ((size_t)span + (h_lds ? (size_t)r.up * r.P : 0)) * sizeof(float);
    const dim3 grid((unsigned)(((int64_t)L_out + run - 1) / run), (unsigned)B);
    if (x_lds && h_lds) launch_one<true, true>(grid, lds_bytes, s, sig, H, out, L, L_out, r, run, span);
    else if (x_lds) launch_one<true, false>(grid, lds_bytes, s, sig, H, out, L, L_out, r, run, span);
    else if (h_lds) launch_one<false, true>(grid, lds_bytes, s, sig, H, out, L, L_out, r, run, span);
    else launch_one<false, false>(grid, lds_bytes, s, sig, H, out, L, L_out, r, run, span);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
