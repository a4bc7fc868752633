// STFT + magnitude compression, and its inverse, as two fused kernels.
//
// Replaces (reference): SpecsDataModule.stft -> spec_fwd and spec_back -> istft (flowmse/data_module.py:149-175,
// 199-205; model.py:190-203), i.e. torch.stft(n_fft=510, hop=128, periodic hann, center=True [reflect], onesided)
// followed by  c * |z|^e * exp(j arg z)  (e = 0.5, c = 0.15), the zero padding of pad_spec (util/other.py:83-90),
// and the inverse chain ending in torch.istft(..., length).  The steps on either side of the sampler
// (SURVEY.md section 8(f), rank 1).  O(n_fft^2) direct DFTs with an exact 510-entry twiddle table: 0.13 MFLOP per
// frame -- microseconds per utterance, no FFT library, no intermediate tensors.
#include <cmath>
#include <cstdio>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/flowse_hip.h"
#include "common.h"

namespace flowse {

constexpr int NFFT = 510, HOP = 128, NBIN = 256, PADC = NFFT / 2;   // 255 samples of centre padding

// [3][NFFT]: window, cos(2 pi k / NFFT), sin(2 pi k / NFFT) -- one copy per device, created under a lock on the
// first call made with that device current (a pointer of one device must never be handed to another's kernels)
static std::mutex g_tab_mu;
static std::map<int, float*> g_tab_of_device;

static int ensure_tables(float** out) {
    int dev = 0;
    FLOWSE_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tab_mu);
    auto it = g_tab_of_device.find(dev);
    if (it != g_tab_of_device.end()) {
        *out = it->second;
        return OK;
    }
    std::vector<float> h(3 * NFFT);
    for (int k = 0; k < NFFT; ++k) {
        const double a = 2.0 * M_PI * (double)k / (double)NFFT;
        h[k] = (float)(0.5 - 0.5 * cos(a));           // periodic Hann
        h[NFFT + k] = (float)cos(a);
        h[2 * NFFT + k] = (float)sin(a);
    }
    float* d = nullptr;
    FLOWSE_HIP(hipMalloc(reinterpret_cast<void**>(&d), h.size() * sizeof(float)));
    FLOWSE_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    g_tab_of_device[dev] = d;
    *out = d;
    return OK;
}

// One frame by one block of 256 threads = 256 bins: frame t of `sig` (L samples, T = L / 128 + 1 frames) to *dst; frames
// t >= T are the zero padding of pad_spec.  Every STFT kernel below is this function, so a frame's value depends on
// (samples, scale_in, t) only -- not on the kernel, the row or the batch that asked for it.  Sample and frame indices in
// 64 bits.  `sig` points at sample s0 of the signal (0: the whole signal; > 0: a window of it, whose caller has checked
// that every index this frame reads lies inside the window).
__device__ __forceinline__ void stft_frame(const float* __restrict__ sig, int64_t L, float scale_in,
                                           const float* __restrict__ tab, float2* __restrict__ dst, int64_t t, int64_t T,
                                           float factor, float exponent, int64_t s0 = 0) {
    __shared__ float xw[NFFT], ct[NFFT], st[NFFT];
    const int f = threadIdx.x;
    if (t >= T) {
        *dst = make_float2(0.f, 0.f);
        return;
    }
    for (int n = threadIdx.x; n < NFFT; n += 256) {
        int64_t j = t * HOP + n - PADC;                // centre=True, reflect padding
        if (j < 0) j = -j;
        if (j >= L) j = 2 * (L - 1) - j;
        xw[n] = sig[j - s0] * scale_in * tab[n];
        ct[n] = tab[NFFT + n];
        st[n] = tab[2 * NFFT + n];
    }
    __syncthreads();
    float re = 0.f, im = 0.f;
    int idx = 0;                                       // (f * n) mod NFFT
    for (int n = 0; n < NFFT; ++n) {
        re = fmaf(xw[n], ct[idx], re);
        im = fmaf(-xw[n], st[idx], im);
        idx += f;
        if (idx >= NFFT) idx -= NFFT;
    }
    // spec_fwd: factor * |z|^e * exp(j arg z) = z * factor * |z|^(e-1)
    const float mag = sqrtf(re * re + im * im);
    float s = factor;
    if (exponent != 1.f) s = mag > 0.f ? factor * powf(mag, exponent - 1.f) : 0.f;
    *dst = make_float2(re * s, im * s);
}

// grid (Tpad, B), 256 threads = 256 bins.  Row b of the output holds frames row_frame0 * b + [0, Tpad) of signal
// sig + row_sig * b: (row_frame0, row_sig) = (0, L) for a batch of utterances, (hop, 0) for the chunks of one recording.
__global__ __launch_bounds__(256) void stft_compress_kernel(const float* __restrict__ sig, int L, float scale_in,
                                                            const float* __restrict__ tab, float2* __restrict__ out,
                                                            int T, int Tpad, float factor, float exponent,
                                                            int row_frame0, int row_sig) {
    const int b = blockIdx.y;
    stft_frame(sig + (int64_t)b * row_sig, L, scale_in, tab, out + ((int64_t)b * NBIN + threadIdx.x) * Tpad + blockIdx.x,
               b * row_frame0 + blockIdx.x, T, factor, exponent);
}

// The rows of ONE sampler call from up to FLOWSE_MAX_SPEC_ROWS different signals: grid (Tw, R), row r = frames
// [frame0_r, frame0_r + Tw) of signal r under its own scale.  The table travels in the kernel's argument block (by value:
// no allocation, no upload, nothing for the host to keep alive) and is indexed by the block's row only.
struct SpecRowTable {
    flowse_spec_row row[FLOWSE_MAX_SPEC_ROWS];
};
static_assert(sizeof(flowse_spec_row) == 24 && sizeof(SpecRowTable) <= 2048, "the table must fit the argument block");

__global__ __launch_bounds__(256) void stft_compress_rows_kernel(const SpecRowTable rows, const float* __restrict__ tab,
                                                                 float2* __restrict__ out, int Tw, float factor,
                                                                 float exponent) {
    const int r = blockIdx.y;
    const float* sig = rows.row[r].sig;
    const int L = rows.row[r].L, frame0 = rows.row[r].frame0;
    const float scale_in = rows.row[r].scale_in;
    stft_frame(sig, L, scale_in, tab, out + ((int64_t)r * NBIN + threadIdx.x) * Tw + blockIdx.x, frame0 + blockIdx.x,
               L / HOP + 1, factor, exponent);
}

// Frame t of a recording held as K chunks [K][NBIN][Tc] that start `hop` frames apart (To = Tc - hop <= hop frames of
// overlap, so at most two chunks cover a frame): chunk k = min(t / hop, K - 1) at j = t - k hop; in the first To frames
// of every chunk but the first, the linear cross-fade  a + w (b - a),  w = (j + 0.5) / To,  from the previous chunk's
// tail a to this chunk's head b -- on the compressed value, before spec_back.  `rows(k)` is chunk k's [NBIN][Tc]: StackRows
// for a contiguous stack, WindowRows for the chunks a live session still holds.
struct StackRows {
    const float2* base;
    int Tc;
    __device__ __forceinline__ const float2* operator()(int k) const { return base + (int64_t)k * NBIN * Tc; }
};

template <class Rows>
__device__ __forceinline__ float2 seam_frame(const Rows& rows, int f, int t, int K, int Tc, int hop) {
    int k = t / hop;
    if (k > K - 1) k = K - 1;
    const int j = t - k * hop, To = Tc - hop;
    const float2 b = rows(k)[(int64_t)f * Tc + j];
    if (k == 0 || j >= To) return b;
    const float2 a = rows(k - 1)[(int64_t)f * Tc + j + hop];
    const float w = ((float)j + 0.5f) / (float)To;
    return make_float2(a.x + w * (b.x - a.x), a.y + w * (b.y - a.y));
}

// spec_back: (|z| / factor)^(1/e) * exp(j arg z)
__device__ __forceinline__ float2 spec_back_value(float2 z, float factor, float exponent) {
    z.x /= factor;
    z.y /= factor;
    if (exponent != 1.f) {
        const float mag = sqrtf(z.x * z.x + z.y * z.y);
        const float s = mag > 0.f ? powf(mag, 1.f / exponent - 1.f) : 0.f;
        z.x *= s;
        z.y *= s;
    }
    return z;
}

// Where the rows of draw d of stack b lie: row b stack_rows + d draw_rows (+ chunk k), in rows of NBIN * Tc values.
// One draw per stack is {1, 1.f, K, 0}.
struct DrawLayout {
    int D;
    float inv_D;
    int64_t stack_rows, draw_rows;
};

// The linear STFT value of draw d at (f, t): the seam rule on that draw's compressed rows, then spec_back.
template <bool SEAM>
__device__ __forceinline__ float2 draw_value(const float2* __restrict__ spec, int b, int d, int f, int t, int Tpad,
                                             float factor, float exponent, int K, int Tc, int hop, const DrawLayout& lay) {
    const float2 z = SEAM ? seam_frame(StackRows{spec + (b * lay.stack_rows + d * lay.draw_rows) * NBIN * Tc, Tc}, f, t, K, Tc,
                                       hop)
                          : spec[((int64_t)b * NBIN + f) * Tpad + t];
    return spec_back_value(z, factor, exponent);
}

// The mean over the draws, summed in the order d = 0 .. D-1 and multiplied by 1 / D.  D == 1: the draw itself (z * 1.f).
template <bool SEAM>
__device__ __forceinline__ float2 mean_value(const float2* __restrict__ spec, int b, int f, int t, int Tpad, float factor,
                                             float exponent, int K, int Tc, int hop, const DrawLayout& lay) {
    float2 m = draw_value<SEAM>(spec, b, 0, f, t, Tpad, factor, exponent, K, Tc, hop, lay);
    for (int d = 1; d < lay.D; ++d) {
        const float2 z = draw_value<SEAM>(spec, b, d, f, t, Tpad, factor, exponent, K, Tc, hop, lay);
        m.x += z.x;
        m.y += z.y;
    }
    return make_float2(m.x * lay.inv_D, m.y * lay.inv_D);
}

// The HOP output samples [n0, n0 + 128) by one block of 256 threads: sample = tid & 127, the two halves split the bins.
// Every inverse-STFT kernel below is this function, so a sample's value depends on the frames over it only -- not on the
// kernel or the block that asked for it.  frames(t, f): the linear value of frame t at bin f, asked only for t < frames.T
// (the frames >= frames.T take no part in the overlap-add).  Sample n is stored at out[n - n_lo] if n_lo <= n < n_hi.
// Sample and frame indices in 64 bits.
template <class Frames>
__device__ __forceinline__ void istft_gather(const Frames& frames, const float* __restrict__ tab, float* __restrict__ out,
                                             int64_t n0, int64_t n_lo, int64_t n_hi, float scale_out) {
    constexpr int NF = 5;                               // frames that can overlap a block of HOP samples
    __shared__ float2 Xs[NF][NBIN];
    __shared__ float ct[NFFT], st[NFFT], win[NFFT];
    __shared__ float part[256];
    const int tid = threadIdx.x;
    const int64_t T = frames.T;
    // frame t covers output samples [128 t - 255, 128 t + 254]
    int64_t t_lo = (n0 - (NFFT - 1 - PADC) + HOP - 1) / HOP;      // ceil((n0 - 254) / 128), may be negative
    if (n0 - (NFFT - 1 - PADC) < 0) t_lo = 0;
    for (int i = tid; i < NFFT; i += 256) {
        win[i] = tab[i];
        ct[i] = tab[NFFT + i];
        st[i] = tab[2 * NFFT + i];
    }
    for (int i = tid; i < NF * NBIN; i += 256) {
        const int fr = i / NBIN, f = i - fr * NBIN;
        const int64_t t = t_lo + fr;
        float2 z = make_float2(0.f, 0.f);
        if (t < T) z = frames(t, f);
        Xs[fr][f] = z;
    }
    __syncthreads();
    const int64_t n = n0 + (tid & 127);
    const int half = tid >> 7;
    float acc = 0.f, env = 0.f;
    for (int fr = 0; fr < NF; ++fr) {
        const int64_t t = t_lo + fr;
        const int64_t kk = n + PADC - t * HOP;          // position inside frame t
        if (t >= T || kk < 0 || kk >= NFFT) continue;
        const int k = (int)kk;
        const float w = win[k];
        env = fmaf(w, w, env);
        // irfft: 1/N [Re X0 + (-1)^k Re X_{N/2} + 2 sum_{f=1}^{N/2-1} (Re X_f cos - Im X_f sin)(2 pi f k / N)]
        const int f0 = half * 128;
        int idx = (int)(((int64_t)f0 * k) % NFFT);
        float s = 0.f;
        for (int f = f0; f < f0 + 128; ++f) {
            const float2 z = Xs[fr][f];
            const float c = (f == 0 || f == NBIN - 1) ? 1.f : 2.f;
            const float zi = (f == 0 || f == NBIN - 1) ? 0.f : z.y;
            s += c * (z.x * ct[idx] - zi * st[idx]);
            idx += k;
            if (idx >= NFFT) idx -= NFFT;
        }
        acc = fmaf(s * (1.f / NFFT), w, acc);
    }
    part[tid] = acc;
    __syncthreads();
    if (half == 0 && n >= n_lo && n < n_hi) {
        const float v = part[tid] + part[tid + 128];
        out[n - n_lo] = env > 1e-11f ? v / env * scale_out : 0.f;
    }
}

// grid (ceil(Lout / 128), B), 256 threads.
// SEAM: `spec` holds B chunk stacks as above, T == Tpad == Tg frames each, of lay.D draws each (DrawLayout; B == 1 and one
// draw for the chunks of one recording); the frame that is transformed back is the mean of the draws' linear values.
// else [B][NBIN][Tpad], one draw.
template <bool SEAM>
struct SpecFrames {
    const float2* spec;
    int64_t T;
    int b, Tpad, K, Tc, hop;
    float factor, exponent;
    DrawLayout lay;
    __device__ __forceinline__ float2 operator()(int64_t t, int f) const {
        return mean_value<SEAM>(spec, b, f, (int)t, Tpad, factor, exponent, K, Tc, hop, lay);
    }
};

template <bool SEAM>
__global__ __launch_bounds__(256) void istft_decompress_kernel(const float2* __restrict__ spec, int T, int Tpad,
                                                               float factor, float exponent,
                                                               const float* __restrict__ tab, float* __restrict__ out,
                                                               int Lout, float scale_out, int K, int Tc, int hop,
                                                               const DrawLayout lay) {
    const int b = blockIdx.y;
    istft_gather(SpecFrames<SEAM>{spec, T, b, Tpad, K, Tc, hop, factor, exponent, lay}, tab, out + (int64_t)b * Lout,
                 (int64_t)blockIdx.x * HOP, 0, Lout, scale_out);
}

// The chunks a live session holds when chunk k has been sampled: c[i] = chunk m + i of the recording, m = max(k - 2, 0),
// as rows of a stack whose frame 0 is the recording's frame m hop.  Chunk m is read as the head of that stack -- WITHOUT
// the blend into chunk m - 1 -- so the host admits only frames that do not need it: [t_lo, t_hi), checked there against
// the seam rule.  Frames outside that range are read as zero; no sample that is stored lies under one.
struct WindowRows {
    const float2* c[3];
    __device__ __forceinline__ const float2* operator()(int k) const { return k == 0 ? c[0] : (k == 1 ? c[1] : c[2]); }
};

struct WindowFrames {
    WindowRows rows;
    int64_t T;                                          // frames >= T take no part: Tg after the last chunk, else none
    int64_t base, t_lo, t_hi;                           // base = m hop
    int Kw, Tc, hop;                                    // Kw: chunks of the local stack (one more while the recording is open)
    float factor, exponent;
    __device__ __forceinline__ float2 operator()(int64_t t, int f) const {
        if (t < t_lo || t >= t_hi) return make_float2(0.f, 0.f);
        // mean_value of one draw multiplies by 1.f, which is exact
        return spec_back_value(seam_frame(rows, f, (int)(t - base), Kw, Tc, hop), factor, exponent);
    }
};

// grid (blocks of 128 samples that meet [e0, e0 + n_out)), 256 threads: out[i] = sample e0 + i of the recording
__global__ __launch_bounds__(256) void istft_decompress_window_kernel(const WindowFrames frames,
                                                                      const float* __restrict__ tab,
                                                                      float* __restrict__ out, int64_t e0, int64_t n_out,
                                                                      float scale_out) {
    istft_gather(frames, tab, out, (e0 / HOP + blockIdx.x) * HOP, e0, e0 + n_out, scale_out);
}

// grid (Tc), 256 threads = 256 bins: frames [frame0, frame0 + Tc) of a recording of which `buf` holds the samples from s0 on
__global__ __launch_bounds__(256) void stft_compress_window_kernel(const float* __restrict__ buf, int64_t s0, int64_t L,
                                                                   float scale_in, const float* __restrict__ tab,
                                                                   float2* __restrict__ out, int64_t frame0, int64_t T,
                                                                   int Tc, float factor, float exponent) {
    stft_frame(buf, L, scale_in, tab, out + (int64_t)threadIdx.x * Tc + blockIdx.x, frame0 + blockIdx.x, T, factor,
               exponent, s0);
}

// ---- trailing chunks (flowmse_amd.chunked.enhance_trailing): chunk k holds the recording's frames [k H - P, k H + H),
// P = Tc - H lead frames of context, of which only the last H (+ X of cross-fade) are kept.
// grid (Tc, rows), 256 threads = 256 bins: row b = chunk k0 + b, frame0 = k0 H - P (negative for the first chunks: the
// frames before the recording are zero, like those >= T).  Every other frame is stft_frame's.
__global__ __launch_bounds__(256) void stft_compress_trailing_kernel(const float* __restrict__ buf, int64_t s0, int64_t L,
                                                                     float scale_in, const float* __restrict__ tab,
                                                                     float2* __restrict__ out, int64_t frame0, int H,
                                                                     int64_t T, int Tc, float factor, float exponent) {
    const int b = blockIdx.y;
    const int64_t t = frame0 + (int64_t)b * H + blockIdx.x;
    float2* dst = out + ((int64_t)b * NBIN + threadIdx.x) * Tc + blockIdx.x;
    if (t < 0) {                                        // the whole block: no barrier is skipped by part of it
        *dst = make_float2(0.f, 0.f);
        return;
    }
    stft_frame(buf, L, scale_in, tab, dst, t, T, factor, exponent, s0);
}

// Frame t of a recording held as trailing chunks [K][NBIN][Tc] (t counted from chunk `rows(0)`'s frame P): chunk
// k = min((t + X) / H, K - 1) at j = t - k H + P; in the X frames before k H the linear cross-fade  a + w (b - a),
// w = (i + 0.5) / X,  i = t - (k H - X), from chunk k - 1 (a, at j + H) to chunk k (b) -- on the compressed value, before
// spec_back.  H + X <= Tc keeps j >= 0 and j + H < Tc.
template <class Rows>
__device__ __forceinline__ float2 trailing_frame(const Rows& rows, int f, int t, int K, int Tc, int H, int X) {
    int k = (t + X) / H;
    if (k > K - 1) k = K - 1;
    const int j = t - k * H + Tc - H;
    const float2 b = rows(k)[(int64_t)f * Tc + j];
    if (k == 0 || t >= k * H) return b;
    const float2 a = rows(k - 1)[(int64_t)f * Tc + j + H];
    const float w = ((float)(t - (k * H - X)) + 0.5f) / (float)X;
    return make_float2(a.x + w * (b.x - a.x), a.y + w * (b.y - a.y));
}

// Rows: StackRows for the K chunks of a file (base = 0, every frame < T = Tg is served), WindowRows for the chunks a live
// session holds (as WindowFrames: chunk m + i, base = m H, and only the frames [t_lo, t_hi) the host admitted).
template <class Rows>
struct TrailingFrames {
    Rows rows;
    int64_t T, base, t_lo, t_hi;
    int Kw, Tc, H, X;
    float factor, exponent;
    __device__ __forceinline__ float2 operator()(int64_t t, int f) const {
        if (t < t_lo || t >= t_hi) return make_float2(0.f, 0.f);
        return spec_back_value(trailing_frame(rows, f, (int)(t - base), Kw, Tc, H, X), factor, exponent);
    }
};

// grid (blocks of 128 samples that meet [e0, e0 + n_out)), 256 threads: out[i] = sample e0 + i of the recording
template <class Rows>
__global__ __launch_bounds__(256) void istft_decompress_trailing_kernel(const TrailingFrames<Rows> frames,
                                                                        const float* __restrict__ tab,
                                                                        float* __restrict__ out, int64_t e0, int64_t n_out,
                                                                        float scale_out) {
    istft_gather(frames, tab, out, (e0 / HOP + blockIdx.x) * HOP, e0, e0 + n_out, scale_out);
}

// The same two kernels for the rows of SEVERAL live sessions (flowmse_amd.livepool): the descriptors travel by value in the
// argument block, as SpecRowTable does, already checked and reduced on the host to what the device code reads.
struct WindowInRow {
    const float* buf;
    int64_t s0, L, frame0, T;                           // L, T: INT64_MAX / 4 while the recording is open
    float scale_in;
};
struct WindowInTable {
    WindowInRow row[FLOWSE_MAX_WINDOW_ROWS];
};
struct WindowOutRow {
    WindowRows rows;
    int64_t T, base, t_lo, t_hi;                        // WindowFrames' own, per row
    float* out;
    int64_t e0, n_out;
    int Kw;
    float scale_out;
};
struct WindowOutTable {
    WindowOutRow row[FLOWSE_MAX_WINDOW_ROWS];
};
static_assert(sizeof(WindowInRow) == 48 && sizeof(WindowOutRow) == 88 && sizeof(WindowInTable) <= 2048 &&
              sizeof(WindowOutTable) <= 2048, "the tables must fit the argument block");

// grid (Tw, R), 256 threads = 256 bins: row r = frames [frame0_r, frame0_r + Tw) from the window of session r
__global__ __launch_bounds__(256) void stft_compress_window_rows_kernel(const WindowInTable rows,
                                                                        const float* __restrict__ tab,
                                                                        float2* __restrict__ out, int Tw, float factor,
                                                                        float exponent) {
    const WindowInRow& w = rows.row[blockIdx.y];
    stft_frame(w.buf, w.L, w.scale_in, tab, out + ((int64_t)blockIdx.y * NBIN + threadIdx.x) * Tw + blockIdx.x,
               w.frame0 + blockIdx.x, w.T, factor, exponent, w.s0);
}

// grid (largest block count of any row, R), 256 threads: a block past its row's range returns without storing
__global__ __launch_bounds__(256) void istft_decompress_window_rows_kernel(const WindowOutTable rows,
                                                                           const float* __restrict__ tab, int Tc, int hop,
                                                                           float factor, float exponent) {
    const WindowOutRow& w = rows.row[blockIdx.y];
    const int64_t b0 = w.e0 / HOP;
    if ((int64_t)blockIdx.x > (w.e0 + w.n_out - 1) / HOP - b0) return;
    const WindowFrames frames{w.rows, w.T, w.base, w.t_lo, w.t_hi, w.Kw, Tc, hop, factor, exponent};
    istft_gather(frames, tab, w.out, (b0 + blockIdx.x) * HOP, w.e0, w.e0 + w.n_out, w.scale_out);
}

// Per-frame agreement tracks of an ensemble: grid (ceil(Tg / 64), S), 256 threads = 64 frames (lanes along t, the
// contiguous axis of a row) x 4 quarters of the bins.  tracks [S][2][Tg]: dev[t] = sum_f sum_d |Z_d - M|^2 / (D - 1), then
// pow[t] = sum_f |M|^2, with M the mean the iSTFT kernel transforms (the same mean_value).  Two passes over the draws per
// (f, t): the mean first, the deviations from the finished mean second -- never sum |Z_d|^2 - D |M|^2, which finds a small
// term by cancellation.  A thread sums its 64 bins in ascending order, the quarters are added in ascending order by one
// thread: no atomics, the same bits on every call.
__global__ __launch_bounds__(256) void ensemble_tracks_kernel(const float2* __restrict__ spec, int Tg, float factor,
                                                              float exponent, float* __restrict__ tracks, int K, int Tc,
                                                              int hop, const DrawLayout lay) {
    __shared__ float sdev[4][64], spow[4][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    float dev = 0.f, pw = 0.f;
    if (t < Tg) {
        for (int f = q * 64; f < q * 64 + 64; ++f) {
            const float2 m = mean_value<true>(spec, b, f, t, Tg, factor, exponent, K, Tc, hop, lay);
            pw += m.x * m.x + m.y * m.y;
            for (int d = 0; d < lay.D; ++d) {
                const float2 z = draw_value<true>(spec, b, d, f, t, Tg, factor, exponent, K, Tc, hop, lay);
                const float ex = z.x - m.x, ey = z.y - m.y;
                dev += ex * ex + ey * ey;
            }
        }
    }
    sdev[q][lane] = dev;
    spow[q][lane] = pw;
    __syncthreads();
    if (q == 0 && t < Tg) {
        dev = ((sdev[0][lane] + sdev[1][lane]) + sdev[2][lane]) + sdev[3][lane];
        pw = ((spow[0][lane] + spow[1][lane]) + spow[2][lane]) + spow[3][lane];
        float* row = tracks + (int64_t)b * 2 * Tg;
        row[t] = dev / (float)(lay.D - 1);
        row[(int64_t)Tg + t] = pw;
    }
}

}  // namespace flowse

using namespace flowse;

// ================================================================================================ C ABI
// Each entry: the null check (ERR_ARG), the shape checks (ERR_SHAPE), the launch.
extern "C" {

// fused STFT + compression (-> complex64 [B,1,256,Tpad], frames >= T zeroed) and decompression + iSTFT
int flowse_stft_compress(const float* sig, int B, int L, float scale_in, void* out_c64, int T, int Tpad, float factor,
                         float exponent, void* stream) {
    if (!sig || !out_c64) {
        set_error("flowse_stft_compress: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (L <= PADC || T != L / HOP + 1 || Tpad < T || B < 1 || B > 65535) {
        set_error("stft: need L > %d, T == L / %d + 1 (got L=%d T=%d Tpad=%d B=%d)", PADC, HOP, L, T, Tpad, B);
        return ERR_SHAPE;
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_compress_kernel, dim3(Tpad, B), dim3(256), 0, s, sig, L, scale_in, tab,
                       reinterpret_cast<float2*>(out_c64), T, Tpad, factor, exponent, 0, L);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// geometry of a chunk stack: K chunks of Tc frames, `hop` apart, at most two over any frame
static bool chunks_ok(int K, int Tc, int hop) {
    return K >= 1 && K <= 65535 && Tc >= 1 && hop >= 1 && hop <= Tc && 2 * (int64_t)hop >= Tc &&
           (int64_t)(K - 1) * hop + Tc <= (1 << 23);
}

// the same pair for ONE recording held as K chunks [K,1,256,Tc] that start `hop` frames apart: chunk rows are slices of
// the recording's spectrogram (frames past L / 128 + 1 zero); synthesis cross-fades the Tc - hop shared frames
int flowse_stft_compress_chunks(const float* sig, int L, float scale_in, void* out_c64, int K, int Tc, int hop, float factor,
                                float exponent, void* stream) {
    if (!sig || !out_c64) {
        set_error("flowse_stft_compress_chunks: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int T = L / HOP + 1;
    if (L <= PADC || !chunks_ok(K, Tc, hop) || (int64_t)(K - 1) * hop + Tc < T) {
        set_error("stft chunks: need L > %d, 1 <= hop <= Tc <= 2 hop, 1 <= K <= 65535 and (K - 1) hop + Tc >= L / %d + 1 "
                  "(got L=%d K=%d Tc=%d hop=%d)", PADC, HOP, L, K, Tc, hop);
        return ERR_SHAPE;
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_compress_kernel, dim3(Tc, K), dim3(256), 0, s, sig, L, scale_in, tab,
                       reinterpret_cast<float2*>(out_c64), T, Tc, factor, exponent, hop, 0);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_istft_decompress(const void* spec_c64, int B, int T, int Tpad, float factor, float exponent, float* out,
                            int Lout, float scale_out, void* stream) {
    if (!spec_c64 || !out) {
        set_error("flowse_istft_decompress: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (T < 1 || Tpad < T || Lout < 1 || Lout > (T - 1) * HOP + NFFT - PADC || B < 1 || B > 65535 || factor == 0.f) {
        set_error("istft: bad shape T=%d Tpad=%d Lout=%d B=%d", T, Tpad, Lout, B);
        return ERR_SHAPE;
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(istft_decompress_kernel<false>, dim3((Lout + HOP - 1) / HOP, B), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(spec_c64), T, Tpad, factor, exponent, tab, out, Lout,
                       scale_out, 0, 0, 0, DrawLayout{1, 1.f, 0, 0});
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// S chunk stacks of one geometry and D draws each -> [S][Lout] (and the tracks [S][2][Tg] of the ensemble call); chunk k of
// draw d of stack s is row s stack_rows + d draw_rows + k.  `who` names the entry in the error text
static int launch_istft_stacks(const char* who, const float* chunks_c64, int S, int D, int K, int Tc, int hop,
                               int64_t stack_rows, int64_t draw_rows, float factor, float exponent, float* out, int Lout,
                               float scale_out, float* tracks, hipStream_t s) {
    const int64_t Tg = (int64_t)(K - 1) * hop + Tc;
    if (S < 1 || S > 65535 || !chunks_ok(K, Tc, hop) || Lout < 1 || Lout > (Tg - 1) * HOP + NFFT - PADC || factor == 0.f) {
        set_error("istft %s: need 1 <= hop <= Tc <= 2 hop, 1 <= K <= 65535, 1 <= S <= 65535, 1 <= Lout <= 128 (Tg - 1) + 255 "
                  "and factor != 0 (got S=%d K=%d Tc=%d hop=%d Lout=%d)", who, S, K, Tc, hop, Lout);
        return ERR_SHAPE;
    }
    if (D < 1 || D > FLOWSE_MAX_DRAWS || (tracks && D == 1)) {
        set_error("istft %s: need 1 <= D <= %d, and null tracks at D = 1 (got D=%d tracks=%s)", who, FLOWSE_MAX_DRAWS, D,
                  tracks ? "given" : "null");
        return ERR_SHAPE;
    }
    // no two of the S D K rows may coincide: the stacks apart by whole draw sets, or the draws apart by whole stack sets;
    // the bounds keep every element offset far inside 64 bits
    constexpr int64_t STRIDE_MAX = (int64_t)1 << 31;
    const bool in_range = stack_rows >= 0 && draw_rows >= 0 && stack_rows <= STRIDE_MAX && draw_rows <= STRIDE_MAX;
    const bool stack_major = (D == 1 || draw_rows >= K) && (S == 1 || stack_rows >= (D - 1) * draw_rows + K);
    const bool draw_major = (S == 1 || stack_rows >= K) && (D == 1 || draw_rows >= (S - 1) * stack_rows + K);
    if (!in_range || !(stack_major || draw_major) ||
        ((S - 1) * stack_rows + (D - 1) * draw_rows + K) > ((int64_t)1 << 59) / ((int64_t)NBIN * Tc)) {
        set_error("istft %s: rows s * stack_stride + d * draw_stride + k alias or leave the address range (got S=%d D=%d K=%d "
                  "stack_stride=%lld draw_stride=%lld)", who, S, D, K, (long long)stack_rows, (long long)draw_rows);
        return ERR_SHAPE;
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    const DrawLayout lay{D, 1.f / (float)D, stack_rows, draw_rows};
    hipLaunchKernelGGL(istft_decompress_kernel<true>, dim3((Lout + HOP - 1) / HOP, S), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(chunks_c64), (int)Tg, (int)Tg, factor, exponent, tab, out, Lout,
                       scale_out, K, Tc, hop, lay);
    FLOWSE_LAUNCH_CHECK();
    if (tracks) {
        hipLaunchKernelGGL(ensemble_tracks_kernel, dim3((unsigned)((Tg + 63) / 64), S), dim3(256), 0, s,
                           reinterpret_cast<const float2*>(chunks_c64), (int)Tg, factor, exponent, tracks, K, Tc, hop, lay);
        FLOWSE_LAUNCH_CHECK();
    }
    return OK;
}

int flowse_istft_decompress_chunks(const void* chunks_c64, int K, int Tc, int hop, float factor, float exponent, float* out,
                                   int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_chunks: null argument");
        return ERR_ARG;
    }
    return launch_istft_stacks("chunks", static_cast<const float*>(chunks_c64), 1, 1, K, Tc, hop, K, 0, factor, exponent, out,
                               Lout, scale_out, nullptr, static_cast<hipStream_t>(stream));
}

// the chunk synthesis for S stacks of one geometry in one launch: [S][K][256][Tc] -> [S][Lout]
int flowse_istft_decompress_stacks(const void* chunks_c64, int S, int K, int Tc, int hop, float factor, float exponent,
                                   float* out, int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_stacks: null argument");
        return ERR_ARG;
    }
    return launch_istft_stacks("stacks", static_cast<const float*>(chunks_c64), S, 1, K, Tc, hop, K, 0, factor, exponent, out,
                               Lout, scale_out, nullptr, static_cast<hipStream_t>(stream));
}

// the stack synthesis over D draws per stack: the mean of the draws' linear spectra -> [S][Lout], and (tracks != null,
// D >= 2) the per-frame deviation and power tracks [S][2][Tg]; row of (s, d, k) = s stack_stride + d draw_stride + k
int flowse_istft_decompress_ensemble(const void* chunks_c64, int S, int D, int K, int Tc, int hop, int64_t stack_stride,
                                     int64_t draw_stride, float factor, float exponent, float* out, int Lout,
                                     float scale_out, float* tracks, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_ensemble: null argument");
        return ERR_ARG;
    }
    return launch_istft_stacks("ensemble", static_cast<const float*>(chunks_c64), S, D, K, Tc, hop, stack_stride, draw_stride,
                               factor, exponent, out, Lout, scale_out, tracks, static_cast<hipStream_t>(stream));
}

// the R rows [R,1,256,Tw] of one sampler call from up to FLOWSE_MAX_SPEC_ROWS signals; `rows`: HOST table
int flowse_stft_compress_rows(const flowse_spec_row* rows, int R, int Tw, void* out_c64, float factor, float exponent,
                              void* stream) {
    if (!rows || !out_c64) {
        set_error("flowse_stft_compress_rows: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R < 1 || R > FLOWSE_MAX_SPEC_ROWS || Tw < 1 || Tw > (1 << 23)) {
        set_error("stft rows: need 1 <= R <= %d and 1 <= Tw <= 2^23 (got R=%d Tw=%d)", FLOWSE_MAX_SPEC_ROWS, R, Tw);
        return ERR_SHAPE;
    }
    SpecRowTable t;
    for (int r = 0; r < FLOWSE_MAX_SPEC_ROWS; ++r) {
        t.row[r] = rows[r < R ? r : 0];                // the slots past R are never read; keep them defined
        if (r >= R) continue;
        if (!rows[r].sig || rows[r].frame0 < 0) {
            set_error("stft rows: row %d has a null signal or frame0 < 0 (frame0=%d)", r, rows[r].frame0);
            return ERR_ARG;
        }
        if (rows[r].L <= PADC || (int64_t)rows[r].frame0 + Tw > (1 << 23)) {
            set_error("stft rows: need L > %d and frame0 + Tw <= 2^23 (row %d: L=%d frame0=%d Tw=%d)", PADC, r, rows[r].L,
                      rows[r].frame0, Tw);
            return ERR_SHAPE;
        }
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_compress_rows_kernel, dim3(Tw, R), dim3(256), 0, s, t, tab, reinterpret_cast<float2*>(out_c64),
                       Tw, factor, exponent);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// ---- windows of a recording that is still arriving (flowmse_amd.live) -------------------------------------------------
// the same per-frame and per-sample code on a WINDOW of the recording: one row of frames [frame0, frame0 + Tc) from the
// samples [s0, s0 + n); the output samples [e0, e0 + n_out) from chunks k-2, k-1, k
constexpr int64_t WINDOW_MAX = (int64_t)1 << 40;        // frames and chunk indices: every product below stays in 64 bits

// The shape checks of one STFT window, shared by the single entry and the row table (`who` names the entry, and the row, in
// the error text).  On success *T is the frame count the kernel takes: L_total / 128 + 1, or INT64_MAX / 4 while open.
static int check_stft_window(const char* who, int64_t s0, int64_t n, int64_t frame0, int Tc, int64_t L_total, int64_t* T_out) {
    const bool closed = L_total >= 0;
    if (s0 < 0 || n < 1 || s0 > WINDOW_MAX * HOP || n > WINDOW_MAX * HOP || frame0 < 0 || frame0 > WINDOW_MAX || Tc < 1 ||
        Tc > (1 << 23) || L_total < -1 || (closed && (L_total <= PADC || s0 + n > L_total))) {
        set_error("%s: need s0 >= 0, n >= 1, 0 <= frame0 <= 2^40, 1 <= Tc <= 2^23 and L_total = -1 or 255 < "
                  "s0 + n <= L_total (got s0=%lld n=%lld frame0=%lld Tc=%d L_total=%lld)", who, (long long)s0, (long long)n,
                  (long long)frame0, Tc, (long long)L_total);
        return ERR_SHAPE;
    }
    // the frames that read samples: [frame0, t_end); those >= T = L_total / 128 + 1 of a closed recording are zero
    const int64_t T = closed ? L_total / HOP + 1 : INT64_MAX / 4;
    const int64_t t_end = frame0 + Tc < T ? frame0 + Tc : T;
    if (t_end > frame0) {
        const int64_t j_lo = frame0 * HOP - PADC, j_hi = (t_end - 1) * HOP + (NFFT - 1 - PADC);   // before reflection
        if (j_lo < 0 && s0 != 0) {
            set_error("%s: frame %lld reflects about sample 0 and needs samples [0, %lld], the window starts at "
                      "s0=%lld", who, (long long)frame0, (long long)-j_lo, (long long)s0);
            return ERR_SHAPE;
        }
        int64_t need_lo = j_lo < 0 ? 0 : j_lo, need_hi = j_hi;
        if (j_lo < 0 && -j_lo > need_hi) need_hi = -j_lo;
        if (closed && j_hi >= L_total) {                // reflected about the last sample: 2 (L - 1) - j for j in [L, j_hi]
            const int64_t r_lo = 2 * (L_total - 1) - j_hi;
            if (r_lo < need_lo) need_lo = r_lo;
            need_hi = L_total - 1;
        }
        if (need_lo < s0 || need_hi >= s0 + n) {
            set_error("%s: frames [%lld, %lld) need samples [%lld, %lld], the window holds [%lld, %lld) "
                      "(L_total=%lld)", who, (long long)frame0, (long long)t_end, (long long)need_lo, (long long)need_hi,
                      (long long)s0, (long long)(s0 + n), (long long)L_total);
            return ERR_SHAPE;
        }
    }
    *T_out = T;
    return OK;
}

int flowse_stft_compress_window(const float* buf, int64_t s0, int64_t n, float scale_in, int64_t frame0, int Tc,
                                int64_t L_total, void* out_c64, float factor, float exponent, void* stream) {
    if (!buf || !out_c64) {
        set_error("flowse_stft_compress_window: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t T = 0;
    int rc = check_stft_window("stft window", s0, n, frame0, Tc, L_total, &T);
    if (rc != OK) return rc;
    float* tab = nullptr;
    rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_compress_window_kernel, dim3(Tc), dim3(256), 0, s, buf, s0, L_total >= 0 ? L_total : INT64_MAX / 4,
                       scale_in, tab, reinterpret_cast<float2*>(out_c64), frame0, T, Tc, factor, exponent);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// The shape checks of one output range, shared likewise; on success *fr is what the kernel reads for it.
static int check_istft_window(const char* who, const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k,
                              int Tc, int hop, int last, int64_t L, float factor, float exponent, int64_t e0, int64_t n_out,
                              WindowFrames* fr) {
    if (k < 0 || k > WINDOW_MAX || Tc < 1 || Tc > (1 << 23) || hop < 1 || hop > Tc || 2 * (int64_t)hop < Tc || e0 < 0 ||
        n_out < 1 || n_out > ((int64_t)1 << 30) || e0 > WINDOW_MAX * HOP || factor == 0.f) {
        set_error("%s: need 0 <= k <= 2^40, 1 <= hop <= Tc <= 2 hop, Tc <= 2^23, e0 >= 0, 1 <= n_out <= 2^30 and "
                  "factor != 0 (got k=%lld Tc=%d hop=%d e0=%lld n_out=%lld)", who, (long long)k, Tc, hop, (long long)e0,
                  (long long)n_out);
        return ERR_SHAPE;
    }
    const int64_t Tg = k * hop + Tc, To = Tc - hop;
    if (last && (e0 + n_out > L || L > (Tg - 1) * HOP + NFFT - PADC)) {
        set_error("%s: after the last chunk need e0 + n_out <= L <= 128 (Tg - 1) + 255 (got e0=%lld n_out=%lld "
                  "L=%lld Tg=%lld)", who, (long long)e0, (long long)n_out, (long long)L, (long long)Tg);
        return ERR_SHAPE;
    }
    // the frames over the samples [e0, e0 + n_out): the index range of istft_gather for one sample, over all of them
    const int64_t t_first = e0 <= NFFT - 1 - PADC ? 0 : (e0 - (NFFT - 1 - PADC) + HOP - 1) / HOP;
    int64_t t_last = (e0 + n_out - 1 + PADC) / HOP;
    if (last && t_last > Tg - 1) t_last = Tg - 1;
    // the chunks the seam rule reads for them
    const int64_t c_hi = last && t_last / hop > k ? k : t_last / hop;
    int64_t c_lo = last && t_first / hop > k ? k : t_first / hop;
    if (c_lo > 0 && t_first - c_lo * hop < To) c_lo -= 1;
    const int64_t m = k >= 2 ? k - 2 : 0;
    if (c_hi > k || c_lo < m || (c_lo <= k - 1 && !prev_c64) || (c_lo <= k - 2 && !prev2_c64)) {
        set_error("%s: samples [%lld, %lld) lie under frames [%lld, %lld], which the seam rule takes from chunks "
                  "%lld..%lld; given are chunk k=%lld%s%s%s", who, (long long)e0, (long long)(e0 + n_out), (long long)t_first,
                  (long long)t_last, (long long)c_lo, (long long)c_hi, (long long)k,
                  (k >= 1 && prev_c64) ? ", k-1" : "", (k >= 2 && prev2_c64) ? ", k-2" : "",
                  last ? " (the last)" : " (not the last: frames from (k+1) hop on wait for chunk k+1)");
        return ERR_SHAPE;
    }
    const float2* given[3] = {reinterpret_cast<const float2*>(prev2_c64), reinterpret_cast<const float2*>(prev_c64),
                              reinterpret_cast<const float2*>(cur_c64)};
    const int held = (int)(k - m) + 1;                  // chunks m .. k
    for (int i = 0; i < 3; ++i) fr->rows.c[i] = i < held ? given[3 - held + i] : nullptr;
    fr->T = last ? Tg : INT64_MAX / 4;
    fr->base = m * hop;
    fr->t_lo = t_first;
    fr->t_hi = t_last + 1;
    fr->Kw = held + (last ? 0 : 1);
    fr->Tc = Tc;
    fr->hop = hop;
    fr->factor = factor;
    fr->exponent = exponent;
    return OK;
}

int flowse_istft_decompress_window(const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k, int Tc,
                                   int hop, int last, int64_t L, float factor, float exponent, float* out, int64_t e0,
                                   int64_t n_out, float scale_out, void* stream) {
    if (!cur_c64 || !out) {
        set_error("flowse_istft_decompress_window: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    WindowFrames fr;
    int rc = check_istft_window("istft window", prev2_c64, prev_c64, cur_c64, k, Tc, hop, last, L, factor, exponent, e0, n_out,
                                &fr);
    if (rc != OK) return rc;
    float* tab = nullptr;
    rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    const int64_t blocks = (e0 + n_out - 1) / HOP - e0 / HOP + 1;
    hipLaunchKernelGGL(istft_decompress_window_kernel, dim3((unsigned)blocks), dim3(256), 0, s, fr, tab, out, e0, n_out,
                       scale_out);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// ---- trailing chunks: the file pair and the window pair (flowmse_amd.chunked.enhance_trailing, flowmse_amd.live) -----------
// geometry: Tc a positive multiple of 64, H even in 4..Tc, 0 <= X <= H, H + X <= Tc (X < 0: the entry has no fade)
static bool trailing_ok(int Tc, int H, int X) {
    return Tc >= 64 && Tc <= (1 << 23) && Tc % 64 == 0 && H >= 4 && H <= Tc && H % 2 == 0 &&
           (X < 0 || (X <= H && (int64_t)H + X <= Tc));
}
#define TRAILING_GEOMETRY "Tc a multiple of 64 in 64..2^23, H even in 4..Tc"

int flowse_stft_compress_trailing(const float* sig, int L, float scale_in, void* out_c64, int K, int Tc, int H, float factor,
                                  float exponent, void* stream) {
    if (!sig || !out_c64) {
        set_error("flowse_stft_compress_trailing: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int T = L / HOP + 1;
    if (L <= PADC || !trailing_ok(Tc, H, -1) || K < 1 || K > 65535 || (int64_t)K * H < T || (int64_t)K * H + Tc > (1 << 23)) {
        set_error("flowse_stft_compress_trailing: need L > %d, " TRAILING_GEOMETRY ", 1 <= K <= 65535 and L / %d + 1 <= K H <= "
                  "2^23 - Tc (got L=%d K=%d Tc=%d H=%d)", PADC, HOP, L, K, Tc, H);
        return ERR_SHAPE;
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_compress_trailing_kernel, dim3(Tc, K), dim3(256), 0, s, sig, (int64_t)0, (int64_t)L, scale_in, tab,
                       reinterpret_cast<float2*>(out_c64), (int64_t)H - Tc, H, (int64_t)T, Tc, factor, exponent);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_istft_decompress_trailing(const void* chunks_c64, int K, int Tc, int H, int X, float factor, float exponent,
                                     float* out, int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_trailing: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t Tg = (int64_t)K * H;
    if (!trailing_ok(Tc, H, X) || X < 0 || K < 1 || K > 65535 || Tg + Tc > (1 << 23) || Lout < 1 ||
        Lout > (Tg - 1) * HOP + NFFT - PADC || factor == 0.f) {
        set_error("flowse_istft_decompress_trailing: need " TRAILING_GEOMETRY ", 0 <= X <= H, H + X <= Tc, 1 <= K <= 65535, "
                  "K H <= 2^23 - Tc, 1 <= Lout <= 128 (K H - 1) + 255 and factor != 0 (got K=%d Tc=%d H=%d X=%d Lout=%d)", K, Tc,
                  H, X, Lout);
        return ERR_SHAPE;
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    const TrailingFrames<StackRows> fr{StackRows{reinterpret_cast<const float2*>(chunks_c64), Tc}, Tg, 0, 0, Tg, K, Tc, H, X,
                                       factor, exponent};
    hipLaunchKernelGGL(istft_decompress_trailing_kernel<StackRows>, dim3((Lout + HOP - 1) / HOP), dim3(256), 0, s, fr, tab, out,
                       (int64_t)0, (int64_t)Lout, scale_out);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_stft_compress_trailing_window(const float* buf, int64_t s0, int64_t n, float scale_in, int64_t k, int Tc, int H,
                                         int64_t L_total, void* out_c64, float factor, float exponent, void* stream) {
    if (!buf || !out_c64) {
        set_error("flowse_stft_compress_trailing_window: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!trailing_ok(Tc, H, -1) || k < 0 || k > WINDOW_MAX / H - 1) {
        set_error("flowse_stft_compress_trailing_window: need " TRAILING_GEOMETRY " and 0 <= k, (k + 1) H <= 2^40 (got k=%lld "
                  "Tc=%d H=%d)", (long long)k, Tc, H);
        return ERR_SHAPE;
    }
    // the frames that read samples start at max(k H - P, 0): the checks of the plain window over those
    const int64_t frame0 = k * H - (Tc - H), first = frame0 < 0 ? 0 : frame0;
    int64_t T = 0;
    int rc = check_stft_window("flowse_stft_compress_trailing_window", s0, n, first, (int)(frame0 + Tc - first), L_total, &T);
    if (rc != OK) return rc;
    float* tab = nullptr;
    rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_compress_trailing_kernel, dim3(Tc, 1), dim3(256), 0, s, buf, s0,
                       L_total >= 0 ? L_total : INT64_MAX / 4, scale_in, tab, reinterpret_cast<float2*>(out_c64), frame0, H, T, Tc,
                       factor, exponent);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_istft_decompress_trailing_window(const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k, int Tc,
                                            int H, int X, int last, int64_t L, float factor, float exponent, float* out,
                                            int64_t e0, int64_t n_out, float scale_out, void* stream) {
    const char* who = "flowse_istft_decompress_trailing_window";
    if (!cur_c64 || !out) {
        set_error("%s: null argument", who);
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!trailing_ok(Tc, H, X) || X < 0 || k < 0 || k > WINDOW_MAX / H - 1 || e0 < 0 || n_out < 1 ||
        n_out > ((int64_t)1 << 30) || e0 > WINDOW_MAX * HOP || factor == 0.f) {
        set_error("%s: need " TRAILING_GEOMETRY ", 0 <= X <= H, H + X <= Tc, 0 <= k, (k + 1) H <= 2^40, e0 >= 0, 1 <= n_out <= "
                  "2^30 and factor != 0 (got k=%lld Tc=%d H=%d X=%d e0=%lld n_out=%lld)", who, (long long)k, Tc, H, X,
                  (long long)e0, (long long)n_out);
        return ERR_SHAPE;
    }
    const int64_t Tg = (k + 1) * H;
    if (last && (e0 + n_out > L || L > (Tg - 1) * HOP + NFFT - PADC)) {
        set_error("%s: after the last chunk need e0 + n_out <= L <= 128 (Tg - 1) + 255 (got e0=%lld n_out=%lld L=%lld "
                  "Tg=%lld)", who, (long long)e0, (long long)n_out, (long long)L, (long long)Tg);
        return ERR_SHAPE;
    }
    // the frames over the samples [e0, e0 + n_out): the index range of istft_gather for one sample, over all of them
    const int64_t t_first = e0 <= NFFT - 1 - PADC ? 0 : (e0 - (NFFT - 1 - PADC) + HOP - 1) / HOP;
    int64_t t_last = (e0 + n_out - 1 + PADC) / HOP;
    if (last && t_last > Tg - 1) t_last = Tg - 1;
    // the chunks the seam rule reads for them: the owner of a frame, and the chunk before it inside the fade; both grow with t
    int64_t c_hi = (t_last + X) / H, c_lo = (t_first + X) / H;
    if (last && c_hi > k) c_hi = k;
    if (last && c_lo > k) c_lo = k;
    if (c_lo > 0 && t_first < c_lo * H) c_lo -= 1;
    const int64_t m = k >= 2 ? k - 2 : 0;
    if (c_hi > k || c_lo < m || (c_lo <= k - 1 && !prev_c64) || (c_lo <= k - 2 && !prev2_c64)) {
        set_error("%s: samples [%lld, %lld) lie under frames [%lld, %lld], which the seam rule takes from chunks %lld..%lld; "
                  "given are chunk k=%lld%s%s%s", who, (long long)e0, (long long)(e0 + n_out), (long long)t_first,
                  (long long)t_last, (long long)c_lo, (long long)c_hi, (long long)k, (k >= 1 && prev_c64) ? ", k-1" : "",
                  (k >= 2 && prev2_c64) ? ", k-2" : "",
                  last ? " (the last)" : " (not the last: frames from (k+1) H - X on wait for chunk k+1)");
        return ERR_SHAPE;
    }
    const float2* given[3] = {reinterpret_cast<const float2*>(prev2_c64), reinterpret_cast<const float2*>(prev_c64),
                              reinterpret_cast<const float2*>(cur_c64)};
    const int held = (int)(k - m) + 1;                  // chunks m .. k
    TrailingFrames<WindowRows> fr;
    for (int i = 0; i < 3; ++i) fr.rows.c[i] = i < held ? given[3 - held + i] : nullptr;
    fr.T = last ? Tg : INT64_MAX / 4;
    fr.base = m * H;
    fr.t_lo = t_first;
    fr.t_hi = t_last + 1;
    fr.Kw = held + (last ? 0 : 1);
    fr.Tc = Tc;
    fr.H = H;
    fr.X = X;
    fr.factor = factor;
    fr.exponent = exponent;
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    const int64_t blocks = (e0 + n_out - 1) / HOP - e0 / HOP + 1;
    hipLaunchKernelGGL(istft_decompress_trailing_kernel<WindowRows>, dim3((unsigned)blocks), dim3(256), 0, s, fr, tab, out, e0,
                       n_out, scale_out);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

// ---- the windows of several sessions in one launch each (flowmse_amd.livepool); `rows`: HOST tables ---------------------
int flowse_stft_compress_window_rows(const flowse_window_row* rows, int R, int Tw, void* out_c64, float factor,
                                     float exponent, void* stream) {
    if (!rows || !out_c64) {
        set_error("flowse_stft_compress_window_rows: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R < 1 || R > FLOWSE_MAX_WINDOW_ROWS) {
        set_error("stft window rows: need 1 <= R <= %d (got R=%d)", FLOWSE_MAX_WINDOW_ROWS, R);
        return ERR_SHAPE;
    }
    WindowInTable t;
    char who[48];
    for (int r = 0; r < FLOWSE_MAX_WINDOW_ROWS; ++r) {
        if (r >= R) {
            t.row[r] = t.row[0];                        // the slots past R are never read; keep them defined
            continue;
        }
        const flowse_window_row& w = rows[r];
        if (!w.buf) {
            set_error("stft window rows: row %d has a null buf", r);
            return ERR_ARG;
        }
        snprintf(who, sizeof(who), "stft window rows: row %d", r);
        int64_t T = 0;
        const int rc = check_stft_window(who, w.s0, w.n, w.frame0, Tw, w.L_total, &T);
        if (rc != OK) return rc;
        t.row[r] = WindowInRow{w.buf, w.s0, w.L_total >= 0 ? w.L_total : INT64_MAX / 4, w.frame0, T, w.scale_in};
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_compress_window_rows_kernel, dim3(Tw, R), dim3(256), 0, s, t, tab,
                       reinterpret_cast<float2*>(out_c64), Tw, factor, exponent);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_istft_decompress_window_rows(const flowse_window_out* rows, int R, int Tc, int hop, float factor, float exponent,
                                        void* stream) {
    if (!rows) {
        set_error("flowse_istft_decompress_window_rows: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R < 1 || R > FLOWSE_MAX_WINDOW_ROWS) {
        set_error("istft window rows: need 1 <= R <= %d (got R=%d)", FLOWSE_MAX_WINDOW_ROWS, R);
        return ERR_SHAPE;
    }
    WindowOutTable t;
    char who[48];
    int64_t blocks = 0;
    for (int r = 0; r < FLOWSE_MAX_WINDOW_ROWS; ++r) {
        if (r >= R) {
            t.row[r] = t.row[0];                        // never read: the grid has R rows
            continue;
        }
        const flowse_window_out& w = rows[r];
        if (!w.cur_c64 || !w.out) {
            set_error("istft window rows: row %d has a null cur_c64 or out", r);
            return ERR_ARG;
        }
        snprintf(who, sizeof(who), "istft window rows: row %d", r);
        WindowFrames fr;
        const int rc = check_istft_window(who, w.prev2_c64, w.prev_c64, w.cur_c64, w.k, Tc, hop, w.last, w.L, factor, exponent,
                                          w.e0, w.n_out, &fr);
        if (rc != OK) return rc;
        t.row[r] = WindowOutRow{fr.rows, fr.T, fr.base, fr.t_lo, fr.t_hi, w.out, w.e0, w.n_out, fr.Kw, w.scale_out};
        const int64_t b = (w.e0 + w.n_out - 1) / HOP - w.e0 / HOP + 1;
        if (b > blocks) blocks = b;
    }
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(istft_decompress_window_rows_kernel, dim3((unsigned)blocks, R), dim3(256), 0, s, t, tab, Tc, hop, factor,
                       exponent);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
