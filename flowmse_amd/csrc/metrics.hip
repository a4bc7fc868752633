// Evaluation metrics on the device: ESTOI and the SI-SDR / SI-SIR / SI-SAR energy ratios, float64 throughout.
//
// ESTOI is defined in include/flowse_hip.h, step by step after pystoi.stoi(x, y, 16000, extended=True) of
// pystoi 0.3 / 0.4.  pystoi is not available where this library is built and tested: equality with it has NOT been
// checked; the kernels are held to the float64 restatement flowmse_amd.metrics.estoi_reference.  The chain of one call:
//
//   resample     clean, proc fp32 @ 16 kHz -> x10, y10 fp64 @ 10 kHz (5 / 8 polyphase, 581 taps, five phases of <= 117)
//   energy       e[i] of the f0 first-pass frames of x10 (one block per frame, fixed-order tree sum)
//   select       one block: max(e), the keep mask, an exclusive scan over any f0, the kept frame list and the count K
//   spectra      one block per rebuilt frame j < K - 1: the 256 overlap-added samples from kept frames j - 1, j, j + 1,
//                windowed, direct DFT over bins 7 .. 218 with a 512-entry twiddle table, 15 band sums -> X_tob, Y_tob
//   segment      one block per segment s < K - 30: row / column normalisation of the 15 x 30 slices, 450-term product
//   finish       one block: fixed-order sum of the segments / (K - 30), or 1e-5 for K - 1 < 30 or L10 <= 256
//
// K is data dependent and lives in device memory: grids are sized for f0 frames, blocks past K read it and leave.  A measurement,
// not a hot loop (a few hundred MFLOP per utterance): plain C++, no atomics, every sum in a fixed order.
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/flowse_hip.h"
#include "common.h"

namespace flowse {

static const int MET_MAX_L = 1 << 24;
static const int MET_UP = 5, MET_DOWN = 8, MET_HALF = 290, MET_TAPS = 2 * MET_HALF + 1, MET_P = 117;   // ceil(581 / 5)
static const int MET_FRAME = 256, MET_HOP = 128, MET_NFFT = 512, MET_BANDS = 15, MET_SEG = 30;
static const int MET_BIN0 = 7, MET_NBIN = 212;                     // DFT bins 7 .. 218 cover the 15 bands
static const int MET_SPAN = 528;                                   // input samples 256 consecutive outputs touch (525)
static const int MET_SCAN = 1024;                                  // threads of the select block
static const int MET_ER_BLOCKS = 128, MET_ER_THREADS = 256;
// the device table: [5][117] polyphase taps (5 h), [256] window, [512] cos(2 pi k / 512)
static const int TAB_H = 0, TAB_W = MET_UP * MET_P, TAB_C = TAB_W + MET_FRAME, TAB_SIZE = TAB_C + MET_NFFT;
#define MET_EPS 2.220446049250313e-16                              // 2^-52

__constant__ int MET_BAND_EDGE[MET_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// h of step 1: kaiser(581, 0.1102 (60 - 8.7)) * 2 * 5 * fc * sinc(2 fc t), fc = 1 / 16, normalised to sum 1
static void design_estoi_taps(double* h) {
    const double fc = 1.0 / 16.0, beta = 0.1102 * (60.0 - 8.7), i0b = bessel_i0(beta);
    double sum = 0.0;
    for (int k = 0; k < MET_TAPS; ++k) {
        const double t = (double)(k - MET_HALF);
        const double y = M_PI * 2.0 * fc * t;
        const double r = t / (double)MET_HALF;
        const double sinc = k == MET_HALF ? 1.0 : sin(y) / y;
        h[k] = bessel_i0(beta * sqrt(fmax(0.0, 1.0 - r * r))) / i0b * (2.0 * (double)MET_UP * fc * sinc);
        sum += h[k];
    }
    for (int k = 0; k < MET_TAPS; ++k) h[k] /= sum;
}

// grid (ceil(L10 / 256), 2): row 0 the clean signal, row 1 the processed one.  c = 290 + 8 n, p = c mod 5, q = c div 5,
// out[n] = sum_{j < 117} H[p][j] x[q - j], x zero outside [0, L); 64-bit sample indices as in resample.hip.
__global__ __launch_bounds__(256) void met_resample_kernel(const float* __restrict__ clean, const float* __restrict__ proc,
                                                           const double* __restrict__ tab, double* __restrict__ x10,
                                                           double* __restrict__ y10, int L, int L10) {
    __shared__ double hs[MET_UP * MET_P];
    __shared__ double xs[MET_SPAN];
    const float* x = blockIdx.y ? proc : clean;
    double* o = blockIdx.y ? y10 : x10;
    const int64_t n0 = (int64_t)blockIdx.x * 256;
    const int64_t q_lo = ((int64_t)MET_HALF + n0 * MET_DOWN) / MET_UP - (MET_P - 1);
    for (int i = threadIdx.x; i < MET_UP * MET_P; i += 256) hs[i] = tab[TAB_H + i];
    for (int i = threadIdx.x; i < MET_SPAN; i += 256) {
        const int64_t m = q_lo + i;
        xs[i] = m >= 0 && m < L ? (double)x[m] : 0.0;
    }
    __syncthreads();
    const int64_t n = n0 + threadIdx.x;
    if (n >= L10) return;
    const int64_t c = (int64_t)MET_HALF + n * MET_DOWN;
    const int64_t q = c / MET_UP;
    const double* h = hs + (int)(c - q * MET_UP) * MET_P;
    const double* xq = xs + (int)(q - q_lo);                       // in [116, 525]
    double acc = 0.0;
    for (int j = 0; j < MET_P; ++j) acc = fma(h[j], xq[-j], acc);
    o[n] = acc;
}

// grid f0: e[i] = 20 log10(|w x10[128 i : 128 i + 256]| + EPS); the last frame ends before L10 (128 (f0 - 1) < L10 - 256)
__global__ __launch_bounds__(256) void met_energy_kernel(const double* __restrict__ x10, const double* __restrict__ tab,
                                                         double* __restrict__ e) {
    __shared__ double red[MET_FRAME];
    const double v = tab[TAB_W + threadIdx.x] * x10[(int64_t)blockIdx.x * MET_HOP + threadIdx.x];
    red[threadIdx.x] = v * v;
    tree_sum(red, MET_FRAME);
    if (threadIdx.x == 0) e[blockIdx.x] = 20.0 * log10(sqrt(red[0]) + MET_EPS);
}

// one block of 1024 threads, any f0 >= 0: thread t owns the frames [t chunk, (t + 1) chunk), chunk = ceil(f0 / 1024);
// counts are scanned across the block, every thread then writes its kept frames in order.  hdr[0] = K.
__global__ __launch_bounds__(MET_SCAN) void met_select_kernel(const double* __restrict__ e, int f0, int* __restrict__ kept,
                                                              int* __restrict__ hdr) {
    __shared__ double mx[MET_SCAN];
    __shared__ int cnt[MET_SCAN];
    const int t = threadIdx.x;
    double m = -INFINITY;
    for (int i = t; i < f0; i += MET_SCAN) m = fmax(m, e[i]);
    mx[t] = m;
    for (int s = MET_SCAN >> 1; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) mx[t] = fmax(mx[t], mx[t + s]);
    }
    __syncthreads();
    const double thr = mx[0] - 40.0;
    const int chunk = (f0 + MET_SCAN - 1) / MET_SCAN;
    const int lo = t * chunk, hi = lo + chunk < f0 ? lo + chunk : f0;
    int c = 0;
    for (int i = lo; i < hi; ++i) c += thr - e[i] < 0.0 ? 1 : 0;
    cnt[t] = c;
    for (int off = 1; off < MET_SCAN; off <<= 1) {                 // inclusive scan
        __syncthreads();
        const int v = t >= off ? cnt[t - off] : 0;
        __syncthreads();
        cnt[t] += v;
    }
    __syncthreads();
    int pos = cnt[t] - c;
    for (int i = lo; i < hi; ++i)
        if (thr - e[i] < 0.0) kept[pos++] = i;
    if (t == MET_SCAN - 1) hdr[0] = cnt[t];
}

// grid max(f0, 1); block j < K - 1 forms rebuilt frame j.  Sample r of it sits at 128 j + r of the rebuilt signal: kept
// frame j at offset r, plus kept frame j - 1 at r + 128 (r < 128, j > 0) or kept frame j + 1 at r - 128 (r >= 128; j + 1 <= K - 1).
// Thread f < 212 then takes DFT bin 7 + f of both signals; sin(2 pi i / 512) = cos(2 pi (i - 128) / 512) from the same table.
__global__ __launch_bounds__(256) void met_spectra_kernel(const double* __restrict__ x10, const double* __restrict__ y10,
                                                          const double* __restrict__ tab, const int* __restrict__ kept,
                                                          const int* __restrict__ hdr, double* __restrict__ xtob,
                                                          double* __restrict__ ytob, int stride) {
    __shared__ double ct[MET_NFFT];
    __shared__ double v[2][MET_FRAME];
    __shared__ double pw[2][MET_NBIN];
    const int K = hdr[0], j = blockIdx.x, r = threadIdx.x;
    if (j >= K - 1) return;
    const double w = tab[TAB_W + r];
    const int64_t own = (int64_t)kept[j] * MET_HOP + r;
    int64_t other = -1;
    double wo = 0.0;
    if (r < MET_HOP) {
        if (j > 0) other = (int64_t)kept[j - 1] * MET_HOP + r + MET_HOP;
        wo = tab[TAB_W + r + MET_HOP];
    } else {
        other = (int64_t)kept[j + 1] * MET_HOP + r - MET_HOP;
        wo = tab[TAB_W + r - MET_HOP];
    }
    double a = w * x10[own], b = w * y10[own];
    if (other >= 0) {
        a += wo * x10[other];
        b += wo * y10[other];
    }
    v[0][r] = w * a;
    v[1][r] = w * b;
    ct[r] = tab[TAB_C + r];
    ct[r + 256] = tab[TAB_C + r + 256];
    __syncthreads();
    if (r < MET_NBIN) {
        const int k = MET_BIN0 + r;
        double xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0;
        int idx = 0;                                               // (k n) mod 512
        for (int n = 0; n < MET_FRAME; ++n) {
            const double c = ct[idx], s = ct[(idx + 384) & 511];
            xr = fma(v[0][n], c, xr);
            xi = fma(v[0][n], s, xi);
            yr = fma(v[1][n], c, yr);
            yi = fma(v[1][n], s, yi);
            idx = (idx + k) & 511;
        }
        pw[0][r] = xr * xr + xi * xi;
        pw[1][r] = yr * yr + yi * yi;
    }
    __syncthreads();
    if (r < 2 * MET_BANDS) {
        const int z = r / MET_BANDS, band = r % MET_BANDS;
        double sum = 0.0;
        for (int k = MET_BAND_EDGE[band]; k < MET_BAND_EDGE[band + 1]; ++k) sum += pw[z][k - MET_BIN0];
        (z ? ytob : xtob)[(int64_t)band * stride + j] = sqrt(sum);
    }
}

// grid max(f0 - 30, 1), 64 threads; block s < K - 30 takes columns [s, s + 30) of both band matrices
__global__ __launch_bounds__(64) void met_segment_kernel(const double* __restrict__ xtob, const double* __restrict__ ytob,
                                                         const int* __restrict__ hdr, double* __restrict__ seg, int stride) {
    __shared__ double a[2][MET_BANDS][MET_SEG];
    __shared__ double part[MET_SEG];
    const int K = hdr[0], s = blockIdx.x, t = threadIdx.x;
    if (s >= K - MET_SEG) return;
    for (int i = t; i < 2 * MET_BANDS * MET_SEG; i += 64) {
        const int z = i / (MET_BANDS * MET_SEG), band = i % (MET_BANDS * MET_SEG) / MET_SEG, n = i % MET_SEG;
        a[z][band][n] = (z ? ytob : xtob)[(int64_t)band * stride + s + n];
    }
    __syncthreads();
    if (t < 2 * MET_BANDS) {                                       // rows: mean over time, then the norm
        double* row = a[t / MET_BANDS][t % MET_BANDS];
        double mean = 0.0, sq = 0.0;
        for (int n = 0; n < MET_SEG; ++n) mean += row[n];
        mean /= (double)MET_SEG;
        for (int n = 0; n < MET_SEG; ++n) {
            row[n] -= mean;
            sq += row[n] * row[n];
        }
        const double d = sqrt(sq) + MET_EPS;
        for (int n = 0; n < MET_SEG; ++n) row[n] /= d;
    }
    __syncthreads();
    if (t < 2 * MET_SEG) {                                         // columns: mean over bands, then the norm
        const int z = t / MET_SEG, n = t % MET_SEG;
        double mean = 0.0, sq = 0.0;
        for (int band = 0; band < MET_BANDS; ++band) mean += a[z][band][n];
        mean /= (double)MET_BANDS;
        for (int band = 0; band < MET_BANDS; ++band) {
            a[z][band][n] -= mean;
            sq += a[z][band][n] * a[z][band][n];
        }
        const double d = sqrt(sq) + MET_EPS;
        for (int band = 0; band < MET_BANDS; ++band) a[z][band][n] /= d;
    }
    __syncthreads();
    if (t < MET_SEG) {
        double sum = 0.0;
        for (int band = 0; band < MET_BANDS; ++band) sum += a[0][band][t] * a[1][band][t];
        part[t] = sum;
    }
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int n = 0; n < MET_SEG; ++n) sum += part[n];
        seg[s] = sum / (double)MET_SEG;
    }
}

__global__ __launch_bounds__(256) void met_finish_kernel(const double* __restrict__ seg, const int* __restrict__ hdr, int L10,
                                                         double* __restrict__ out) {
    __shared__ double red[256];
    const int nseg = hdr[0] - MET_SEG;                             // K - 1 frames give K - 30 segments
    if (L10 <= MET_FRAME || nseg < 1) {
        if (threadIdx.x == 0) out[0] = 1e-5;
        return;
    }
    double acc = 0.0;
    for (int i = threadIdx.x; i < nseg; i += 256) acc += seg[i];
    red[threadIdx.x] = acc;
    tree_sum(red, 256);
    if (threadIdx.x == 0) out[0] = red[0] / (double)nseg;
}

// ---- energy ratios: every block owns the samples i = block 256 + thread (mod 128 * 256); partial sums per block, merged by
// the next kernel in a fixed order
__global__ __launch_bounds__(MET_ER_THREADS) void met_er_dots_kernel(const float* __restrict__ est, const float* __restrict__ clean,
                                                                     const float* __restrict__ noisy, int L,
                                                                     double* __restrict__ p1) {
    __shared__ double red[MET_ER_THREADS];
    double d[4] = {0.0, 0.0, 0.0, 0.0};                            // <est, s>, <s, s>, <est, n>, <n, n>
    for (int64_t i = (int64_t)blockIdx.x * MET_ER_THREADS + threadIdx.x; i < L; i += (int64_t)MET_ER_BLOCKS * MET_ER_THREADS) {
        const double sh = (double)est[i], s = (double)clean[i], n = (double)noisy[i] - s;
        d[0] += sh * s;
        d[1] += s * s;
        d[2] += sh * n;
        d[3] += n * n;
    }
    for (int q = 0; q < 4; ++q) {
        red[threadIdx.x] = d[q];
        tree_sum(red, MET_ER_THREADS);
        if (threadIdx.x == 0) p1[blockIdx.x * 4 + q] = red[0];
        __syncthreads();
    }
}

// the four dot products from the 128 block partials, the same order in every block that asks
__device__ __forceinline__ void er_merge_dots(const double* __restrict__ p1, double* red, double* dots) {
    for (int q = 0; q < 4; ++q) {
        if (threadIdx.x < MET_ER_BLOCKS) red[threadIdx.x] = p1[threadIdx.x * 4 + q];
        tree_sum(red, MET_ER_BLOCKS);
        dots[q] = red[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(MET_ER_THREADS) void met_er_norms_kernel(const float* __restrict__ est, const float* __restrict__ clean,
                                                                      const float* __restrict__ noisy, int L,
                                                                      const double* __restrict__ p1, double* __restrict__ p2) {
    __shared__ double red[MET_ER_THREADS];
    double dots[4];
    er_merge_dots(p1, red, dots);
    const double a_s = dots[0] / dots[1], a_n = dots[2] / dots[3];
    double d[3] = {0.0, 0.0, 0.0};                                 // |est - a_s s|^2, |a_n n|^2, |est - a_s s - a_n n|^2
    for (int64_t i = (int64_t)blockIdx.x * MET_ER_THREADS + threadIdx.x; i < L; i += (int64_t)MET_ER_BLOCKS * MET_ER_THREADS) {
        const double sh = (double)est[i], s = (double)clean[i], n = (double)noisy[i] - s;
        const double r = sh - a_s * s, en = a_n * n, art = r - en;
        d[0] += r * r;
        d[1] += en * en;
        d[2] += art * art;
    }
    for (int q = 0; q < 3; ++q) {
        red[threadIdx.x] = d[q];
        tree_sum(red, MET_ER_THREADS);
        if (threadIdx.x == 0) p2[blockIdx.x * 3 + q] = red[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(MET_ER_THREADS) void met_er_finish_kernel(const double* __restrict__ p1, const double* __restrict__ p2,
                                                                       double* __restrict__ out3) {
    __shared__ double red[MET_ER_THREADS];
    double dots[4], norms[3];
    er_merge_dots(p1, red, dots);
    for (int q = 0; q < 3; ++q) {
        if (threadIdx.x < MET_ER_BLOCKS) red[threadIdx.x] = p2[threadIdx.x * 3 + q];
        tree_sum(red, MET_ER_BLOCKS);
        norms[q] = red[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a_s = dots[0] / dots[1];
        const double target = a_s * a_s * dots[1];                 // |a_s s|^2
        out3[0] = 10.0 * log10(target / norms[0]);
        out3[1] = 10.0 * log10(target / norms[1]);
        out3[2] = 10.0 * log10(target / norms[2]);
    }
}

// ---- the workspace of one length: every region 256-byte aligned, sized for the worst case K = f0
struct MetLayout {
    int L10, f0;
    int64_t x10, y10, e, xtob, ytob, seg, kept, hdr, p1, p2, total;
};

static MetLayout met_layout(int L) {
    MetLayout w;
    w.L10 = (int)(((int64_t)L * MET_UP + MET_DOWN - 1) / MET_DOWN);
    w.f0 = w.L10 > MET_FRAME ? (w.L10 - MET_FRAME + MET_HOP - 1) / MET_HOP : 0;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        const int64_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const int64_t f = w.f0 > 0 ? w.f0 : 1;
    w.hdr = take(256);
    w.p1 = take((int64_t)MET_ER_BLOCKS * 4 * sizeof(double));
    w.p2 = take((int64_t)MET_ER_BLOCKS * 3 * sizeof(double));
    w.x10 = take((int64_t)w.L10 * sizeof(double));
    w.y10 = take((int64_t)w.L10 * sizeof(double));
    w.e = take(f * sizeof(double));
    w.xtob = take(f * MET_BANDS * sizeof(double));
    w.ytob = take(f * MET_BANDS * sizeof(double));
    w.seg = take(f * sizeof(double));
    w.kept = take(f * sizeof(int));
    w.total = at;
    return w;
}

// The table of one device, cached as resample.hip caches its polyphase tables: built on the host and uploaded on the stream
// of the call that needs it first, `ready` orders calls on other streams behind that upload.  That first call allocates,
// copies from pageable memory (the runtime stages it and may wait) and records an event: it must not be made while its
// stream is being captured.  Every later call only enqueues.
struct MetTable {
    std::vector<double> host;                      // kept: the source of an asynchronous copy
    double* dev = nullptr;
    hipEvent_t ready = nullptr;
};
static std::mutex g_met_mutex;
static std::map<int, MetTable> g_met_tables;

static int get_met_table(hipStream_t s, const double** dev) {
    int device = 0;
    FLOWSE_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_met_mutex);
    MetTable& t = g_met_tables[device];
    if (!t.dev) {
        std::vector<double> h(MET_TAPS);
        design_estoi_taps(h.data());
        t.host.assign(TAB_SIZE, 0.0);
        for (int k = 0; k < MET_TAPS; ++k) t.host[TAB_H + (k % MET_UP) * MET_P + k / MET_UP] = (double)MET_UP * h[k];
        for (int n = 0; n < MET_FRAME; ++n)        // hanning(258)[1:-1]
            t.host[TAB_W + n] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)(n + 1) / (double)(MET_FRAME + 1));
        for (int k = 0; k < MET_NFFT; ++k) t.host[TAB_C + k] = cos(2.0 * M_PI * (double)k / (double)MET_NFFT);
        double* d = nullptr;
        FLOWSE_HIP(hipMalloc(reinterpret_cast<void**>(&d), t.host.size() * sizeof(double)));
        hipError_t e = hipEventCreateWithFlags(&t.ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemcpyAsync(d, t.host.data(), t.host.size() * sizeof(double), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(t.ready, s);
        if (e != hipSuccess) {
            if (t.ready) (void)hipEventDestroy(t.ready);
            t.ready = nullptr;
            (void)hipFree(d);
            return hip_fail(e, "metrics table upload", __FILE__, __LINE__);
        }
        t.dev = d;
    }
    FLOWSE_HIP(hipStreamWaitEvent(s, t.ready, 0));
    *dev = t.dev;
    return OK;
}

// the argument checks both calls share; the message names the caller
static int met_check(const char* who, bool null_ptr, int L, int64_t workspace_bytes, MetLayout* w) {
    if (L < 1 || L > MET_MAX_L) {
        set_error("%s: L must be 1 .. %d samples, got %d", who, MET_MAX_L, L);
        return ERR_ARG;
    }
    if (null_ptr) {
        set_error("%s: null pointer (signals, workspace and out are device memory)", who);
        return ERR_ARG;
    }
    *w = met_layout(L);
    if (workspace_bytes < w->total) {
        set_error("%s: L = %d needs a workspace of %lld bytes (flowse_metrics_workspace_bytes), got %lld", who, L,
                  (long long)w->total, (long long)workspace_bytes);
        return ERR_ARG;
    }
    return OK;
}

}  // namespace flowse

using namespace flowse;

extern "C" {

int flowse_estoi_num_taps(void) { return MET_TAPS; }

int flowse_estoi_taps(double* taps, int cap) {
    if (!taps || cap < MET_TAPS) {
        set_error("flowse_estoi_taps: %d taps, the buffer holds %d", MET_TAPS, taps ? cap : 0);
        return ERR_ARG;
    }
    design_estoi_taps(taps);
    return OK;
}

int64_t flowse_metrics_workspace_bytes(int L) {
    if (L < 1 || L > MET_MAX_L) {
        set_error("flowse_metrics_workspace_bytes: L must be 1 .. %d samples, got %d", MET_MAX_L, L);
        return -(int64_t)ERR_ARG;
    }
    return met_layout(L).total;
}

int flowse_estoi(const float* clean, const float* proc, int L, void* workspace, int64_t workspace_bytes, double* out,
                 void* stream) {
    MetLayout w;
    if (const int rc = met_check("flowse_estoi", !clean || !proc || !workspace || !out, L, workspace_bytes, &w)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double* tab = nullptr;
    if (const int rc = get_met_table(s, &tab)) return rc;
    char* base = static_cast<char*>(workspace);
    double* x10 = reinterpret_cast<double*>(base + w.x10);
    double* y10 = reinterpret_cast<double*>(base + w.y10);
    double* e = reinterpret_cast<double*>(base + w.e);
    double* xtob = reinterpret_cast<double*>(base + w.xtob);
    double* ytob = reinterpret_cast<double*>(base + w.ytob);
    double* seg = reinterpret_cast<double*>(base + w.seg);
    int* kept = reinterpret_cast<int*>(base + w.kept);
    int* hdr = reinterpret_cast<int*>(base + w.hdr);
    const int stride = w.f0 > 0 ? w.f0 : 1;
    hipLaunchKernelGGL(met_resample_kernel, dim3((unsigned)((w.L10 + 255) / 256), 2), dim3(256), 0, s, clean, proc, tab, x10,
                       y10, L, w.L10);
    if (w.f0 > 0) hipLaunchKernelGGL(met_energy_kernel, dim3((unsigned)w.f0), dim3(256), 0, s, x10, tab, e);
    hipLaunchKernelGGL(met_select_kernel, dim3(1), dim3(MET_SCAN), 0, s, e, w.f0, kept, hdr);
    hipLaunchKernelGGL(met_spectra_kernel, dim3((unsigned)stride), dim3(256), 0, s, x10, y10, tab, kept, hdr, xtob, ytob, stride);
    hipLaunchKernelGGL(met_segment_kernel, dim3((unsigned)(w.f0 > MET_SEG ? w.f0 - MET_SEG : 1)), dim3(64), 0, s, xtob, ytob,
                       hdr, seg, stride);
    hipLaunchKernelGGL(met_finish_kernel, dim3(1), dim3(256), 0, s, seg, hdr, w.L10, out);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_energy_ratios(const float* est, const float* clean, const float* noisy, int L, void* workspace,
                         int64_t workspace_bytes, double* out3, void* stream) {
    MetLayout w;
    if (const int rc = met_check("flowse_energy_ratios", !est || !clean || !noisy || !workspace || !out3, L, workspace_bytes, &w))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(workspace);
    double* p1 = reinterpret_cast<double*>(base + w.p1);
    double* p2 = reinterpret_cast<double*>(base + w.p2);
    hipLaunchKernelGGL(met_er_dots_kernel, dim3(MET_ER_BLOCKS), dim3(MET_ER_THREADS), 0, s, est, clean, noisy, L, p1);
    hipLaunchKernelGGL(met_er_norms_kernel, dim3(MET_ER_BLOCKS), dim3(MET_ER_THREADS), 0, s, est, clean, noisy, L, p1, p2);
    hipLaunchKernelGGL(met_er_finish_kernel, dim3(1), dim3(MET_ER_THREADS), 0, s, p1, p2, out3);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
