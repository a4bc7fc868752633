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

// One row of an STFT launch: frames frame0 + [0, Tw) of the signal of L samples and T frames of which `buf` holds the
// samples from s0 on, under its own scale.  frame0 may be negative (the lead of the first trailing chunks); L and T are
// INT64_MAX / 4 while a recording is open.
struct SignalRow {
    const float* buf;
    int64_t s0, L, frame0, T;
    float scale_in;
};

// Where the row descriptor of block row b comes from.  Affine in b: row b = signal buf + b row_sig at frames
// frame0 + b row_frame0 -- (row_sig, row_frame0) = (L, 0) for a batch of utterances, (0, hop) for the chunks of one
// recording, (0, H) with frame0 = -P for its trailing chunks, one row for a window of a live session.
struct AffineRows {
    SignalRow row0;
    int64_t row_sig, row_frame0;
    __device__ __forceinline__ SignalRow operator()(int b) const {
        SignalRow r = row0;
        r.buf += b * row_sig;
        r.frame0 += b * row_frame0;
        return r;
    }
};

// Or a table: the rows of ONE sampler call from up to FLOWSE_MAX_SPEC_ROWS different signals, or from the windows of up to
// FLOWSE_MAX_WINDOW_ROWS live sessions (flowmse_amd.livepool; already checked and reduced on the host to what the device
// code reads).  A table travels in the kernel's argument block (by value: no allocation, no upload, nothing for the host to
// keep alive) and is indexed by the block's row only.  Two descriptor types, because 64 SignalRows would not fit.
struct SpecRowTable {
    flowse_spec_row row[FLOWSE_MAX_SPEC_ROWS];
    __device__ __forceinline__ SignalRow operator()(int r) const {
        return SignalRow{row[r].sig, 0, row[r].L, row[r].frame0, row[r].L / HOP + 1, row[r].scale_in};
    }
};
struct WindowInTable {
    SignalRow row[FLOWSE_MAX_WINDOW_ROWS];
    __device__ __forceinline__ SignalRow operator()(int r) const { return row[r]; }
};
static_assert(sizeof(flowse_spec_row) == 24 && sizeof(SpecRowTable) <= 2048, "the table must fit the argument block");

// grid (Tw, R), 256 threads = 256 bins: row r of out [R][NBIN][Tw] holds the frames of rows(r); frames < 0 or >= T are zero
template <class Rows>
__global__ __launch_bounds__(256) void stft_kernel(const Rows rows, const float* __restrict__ tab, float2* __restrict__ out,
                                                   int Tw, float factor, float exponent) {
    const SignalRow w = rows(blockIdx.y);
    const int64_t t = w.frame0 + blockIdx.x;
    float2* dst = out + ((int64_t)blockIdx.y * NBIN + threadIdx.x) * Tw + blockIdx.x;
    if (t < 0) {                                        // the whole block: no barrier is skipped by part of it
        *dst = make_float2(0.f, 0.f);
        return;
    }
    stft_frame(w.buf, w.L, w.scale_in, tab, dst, t, w.T, factor, exponent, w.s0);
}

// ---- the seam rule.  A recording is held as K chunks [K][NBIN][Tc] whose kept parts start H frames apart: chunk k holds
// the recording's frames [k H - P, k H + H), P = Tc - H frames of lead, counted from chunk 0's frame P.  Frame u belongs to
// chunk k = min((u + X) / H, K - 1) at j = u - k H + P; in the X frames before k H the linear cross-fade  a + w (b - a),
// w = (i + 0.5) / X,  i = u - (k H - X), from chunk k - 1 (a, at j + H) to chunk k (b) -- on the compressed value, before
// spec_back.  H + X <= Tc keeps j >= 0 and j + H < Tc.  The caller counts frames from u = -shift:
//   trailing chunks (flowmse_amd.chunked.enhance_trailing)  {Tc, H, X, 0}: frames before the recording are zero rows;
//   overlap chunks `hop` apart, To = Tc - hop <= hop shared  {Tc, hop, To, To}: the same rule at X = P with the lead of
//   chunk 0 counted in -- k = min(t / hop, K - 1) at j = t - k hop, the fade over j < To with w = (j + 0.5) / To.
// u + X >= 0 in both, so the truncating division is the floor.
struct ChunkGeom {
    int Tc, H, X, shift;
};

// `rows(k)` is chunk k's [NBIN][Tc]: StackRows for a contiguous stack, WindowRows for the chunks a live session still holds.
struct StackRows {
    const float2* base;
    int Tc;
    __device__ __forceinline__ const float2* operator()(int k) const { return base + (int64_t)k * NBIN * Tc; }
};

template <class Rows>
__device__ __forceinline__ float2 chunk_frame(const Rows& rows, int f, int t, int K, const ChunkGeom& g) {
    const int u = t - g.shift;
    int k = (u + g.X) / g.H;
    if (k > K - 1) k = K - 1;
    const int j = u - k * g.H + g.Tc - g.H;
    const float2 b = rows(k)[(int64_t)f * g.Tc + j];
    if (k == 0 || u >= k * g.H) return b;
    const float2 a = rows(k - 1)[(int64_t)f * g.Tc + j + g.H];
    const float w = ((float)(u - (k * g.H - g.X)) + 0.5f) / (float)g.X;
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

// Chunk stacks of one geometry, of lay.D draws each.  [B][NBIN][Tpad] is B stacks of one chunk: K = 1, {Tpad, Tpad, 0, 0}.
struct Stacks {
    const float2* spec;
    int K;
    ChunkGeom g;
    float factor, exponent;
    DrawLayout lay;
};

// The linear STFT value of draw d of stack b at (f, t): the seam rule on that draw's compressed rows, then spec_back.
__device__ __forceinline__ float2 draw_value(const Stacks& s, int b, int d, int f, int t) {
    const StackRows rows{s.spec + (b * s.lay.stack_rows + d * s.lay.draw_rows) * NBIN * s.g.Tc, s.g.Tc};
    return spec_back_value(chunk_frame(rows, f, t, s.K, s.g), s.factor, s.exponent);
}

// The mean over the draws, summed in the order d = 0 .. D-1 and multiplied by 1 / D.  D == 1: the draw itself (z * 1.f).
__device__ __forceinline__ float2 mean_value(const Stacks& s, int b, int f, int t) {
    float2 m = draw_value(s, b, 0, f, t);
    for (int d = 1; d < s.lay.D; ++d) {
        const float2 z = draw_value(s, b, d, f, t);
        m.x += z.x;
        m.y += z.y;
    }
    return make_float2(m.x * s.lay.inv_D, m.y * s.lay.inv_D);
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

// ---- frame sources of istft_gather, and what one row of an iSTFT launch stores: out[i] = sample e0 + i of the signal whose
// frames are `frames`, for 0 <= i < n_out.  A single range is its own one-row source.
template <class Frames>
struct OutputRange {
    Frames frames;
    float* out;
    int64_t e0, n_out;
    float scale_out;
    __device__ __forceinline__ const OutputRange& operator()(int) const { return *this; }
};

// Stack b of `st`, T frames: the frame that is transformed back is the mean of the draws' linear values.
struct StackFrames {
    Stacks st;
    int64_t T;
    int b;
    __device__ __forceinline__ float2 operator()(int64_t t, int f) const { return mean_value(st, b, f, (int)t); }
};
// row b = all Lout samples of stack b -> out [B][Lout]
struct StackOutputs {
    Stacks st;
    int T, Lout;
    float* out;
    float scale_out;
    __device__ __forceinline__ OutputRange<StackFrames> operator()(int b) const {
        return OutputRange<StackFrames>{StackFrames{st, T, b}, out + (int64_t)b * Lout, 0, Lout, scale_out};
    }
};

// The chunks a live session holds when chunk k has been sampled: c[i] = chunk m + i of the recording, m = max(k - 2, 0),
// as rows of a stack whose frame 0 is the recording's frame m H.  Chunk m is read as the head of that stack -- WITHOUT
// the blend into chunk m - 1 -- so the host admits only frames that do not need it: [t_lo, t_hi), checked there against
// the seam rule.  Frames outside that range are read as zero; no sample that is stored lies under one.
struct WindowRows {
    const float2* c[3];
    __device__ __forceinline__ const float2* operator()(int k) const { return k == 0 ? c[0] : (k == 1 ? c[1] : c[2]); }
};

// A window of a recording: Rows = WindowRows as above, or StackRows for the K chunks of a file (base = 0, every frame
// < T = Tg is served).
template <class Rows>
struct ChunkWindow {
    Rows rows;
    int64_t T;                                          // frames >= T take no part: Tg after the last chunk, else none
    int64_t base, t_lo, t_hi;                           // base = m H
    int Kw;                                             // chunks of the local stack (one more while the recording is open)
    ChunkGeom g;
    float factor, exponent;
    __device__ __forceinline__ float2 operator()(int64_t t, int f) const {
        if (t < t_lo || t >= t_hi) return make_float2(0.f, 0.f);
        // mean_value of one draw multiplies by 1.f, which is exact
        return spec_back_value(chunk_frame(rows, f, (int)(t - base), Kw, g), factor, exponent);
    }
};

// The output ranges of SEVERAL live sessions of one geometry (flowmse_amd.livepool), by value like the tables above.
struct WindowOutRow {
    WindowRows rows;
    int64_t T, base, t_lo, t_hi;                        // ChunkWindow's own, per row
    float* out;
    int64_t e0, n_out;
    int Kw;
    float scale_out;
};
struct WindowOutTable {
    WindowOutRow row[FLOWSE_MAX_WINDOW_ROWS];
    ChunkGeom g;
    float factor, exponent;
    __device__ __forceinline__ OutputRange<ChunkWindow<WindowRows>> operator()(int r) const {
        const WindowOutRow& w = row[r];
        return OutputRange<ChunkWindow<WindowRows>>{{w.rows, w.T, w.base, w.t_lo, w.t_hi, w.Kw, g, factor, exponent},
                                                    w.out, w.e0, w.n_out, w.scale_out};
    }
};
static_assert(sizeof(SignalRow) == 48 && sizeof(WindowOutRow) == 88 && sizeof(WindowInTable) <= 2048 &&
              sizeof(WindowOutTable) <= 2048, "the tables must fit the argument block");

// grid (blocks of 128 samples that meet the longest row's [e0, e0 + n_out), R), 256 threads: a block past its row's range
// returns (all of it) without storing
template <class Outputs>
__global__ __launch_bounds__(256) void istft_kernel(const Outputs outputs, const float* __restrict__ tab) {
    const auto r = outputs(blockIdx.y);
    const int64_t b0 = r.e0 / HOP;
    if ((int64_t)blockIdx.x > (r.e0 + r.n_out - 1) / HOP - b0) return;
    istft_gather(r.frames, tab, r.out, (b0 + blockIdx.x) * HOP, r.e0, r.e0 + r.n_out, r.scale_out);
}

// Per-frame agreement tracks of an ensemble: grid (ceil(Tg / 64), S), 256 threads = 64 frames (lanes along t, the
// contiguous axis of a row) x 4 quarters of the bins.  tracks [S][2][Tg]: dev[t] = sum_f sum_d |Z_d - M|^2 / (D - 1), then
// pow[t] = sum_f |M|^2, with M the mean the iSTFT kernel transforms (the same mean_value).  Two passes over the draws per
// (f, t): the mean first, the deviations from the finished mean second -- never sum |Z_d|^2 - D |M|^2, which finds a small
// term by cancellation.  A thread sums its 64 bins in ascending order, the quarters are added in ascending order by one
// thread: no atomics, the same bits on every call.
__global__ __launch_bounds__(256) void ensemble_tracks_kernel(const Stacks st, int Tg, float* __restrict__ tracks) {
    __shared__ float sdev[4][64], spow[4][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    float dev = 0.f, pw = 0.f;
    if (t < Tg) {
        for (int f = q * 64; f < q * 64 + 64; ++f) {
            const float2 m = mean_value(st, b, f, t);
            pw += m.x * m.x + m.y * m.y;
            for (int d = 0; d < st.lay.D; ++d) {
                const float2 z = draw_value(st, b, d, f, t);
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
        row[t] = dev / (float)(st.lay.D - 1);
        row[(int64_t)Tg + t] = pw;
    }
}

}  // namespace flowse

using namespace flowse;

// The tail of every entry: the tables of the current device, the launch, its check.
template <class Rows>
static int launch_stft(const Rows& rows, int Tw, int R, void* out_c64, float factor, float exponent, void* stream) {
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(stft_kernel<Rows>, dim3(Tw, R), dim3(256), 0, static_cast<hipStream_t>(stream), rows, tab,
                       reinterpret_cast<float2*>(out_c64), Tw, factor, exponent);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

template <class Outputs>
static int launch_istft(const Outputs& outputs, int64_t blocks, int R, void* stream) {
    float* tab = nullptr;
    int rc = ensure_tables(&tab);
    if (rc != OK) return rc;
    hipLaunchKernelGGL(istft_kernel<Outputs>, dim3((unsigned)blocks, R), dim3(256), 0, static_cast<hipStream_t>(stream),
                       outputs, tab);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

static ChunkGeom overlap_geom(int Tc, int hop) { return ChunkGeom{Tc, hop, Tc - hop, Tc - hop}; }
static ChunkGeom trailing_geom(int Tc, int H, int X) { return ChunkGeom{Tc, H, X, 0}; }

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
    if (L <= PADC || T != L / HOP + 1 || Tpad < T || B < 1 || B > 65535) {
        set_error("stft: need L > %d, T == L / %d + 1 (got L=%d T=%d Tpad=%d B=%d)", PADC, HOP, L, T, Tpad, B);
        return ERR_SHAPE;
    }
    return launch_stft(AffineRows{{sig, 0, L, 0, T, scale_in}, L, 0}, Tpad, B, out_c64, factor, exponent, stream);
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
    const int T = L / HOP + 1;
    if (L <= PADC || !chunks_ok(K, Tc, hop) || (int64_t)(K - 1) * hop + Tc < T) {
        set_error("stft chunks: need L > %d, 1 <= hop <= Tc <= 2 hop, 1 <= K <= 65535 and (K - 1) hop + Tc >= L / %d + 1 "
                  "(got L=%d K=%d Tc=%d hop=%d)", PADC, HOP, L, K, Tc, hop);
        return ERR_SHAPE;
    }
    return launch_stft(AffineRows{{sig, 0, L, 0, T, scale_in}, 0, hop}, Tc, K, out_c64, factor, exponent, stream);
}

int flowse_istft_decompress(const void* spec_c64, int B, int T, int Tpad, float factor, float exponent, float* out,
                            int Lout, float scale_out, void* stream) {
    if (!spec_c64 || !out) {
        set_error("flowse_istft_decompress: null argument");
        return ERR_ARG;
    }
    if (T < 1 || Tpad < T || Lout < 1 || Lout > (T - 1) * HOP + NFFT - PADC || B < 1 || B > 65535 || factor == 0.f) {
        set_error("istft: bad shape T=%d Tpad=%d Lout=%d B=%d", T, Tpad, Lout, B);
        return ERR_SHAPE;
    }
    const Stacks st{reinterpret_cast<const float2*>(spec_c64), 1, ChunkGeom{Tpad, Tpad, 0, 0}, factor, exponent,
                    DrawLayout{1, 1.f, 1, 0}};
    return launch_istft(StackOutputs{st, T, Lout, out, scale_out}, (Lout + HOP - 1) / HOP, B, stream);
}

// S chunk stacks of one geometry and D draws each -> [S][Lout] (and the tracks [S][2][Tg] of the ensemble call); chunk k of
// draw d of stack s is row s stack_rows + d draw_rows + k.  `who` names the entry in the error text
static int launch_istft_stacks(const char* who, const float* chunks_c64, int S, int D, int K, int Tc, int hop,
                               int64_t stack_rows, int64_t draw_rows, float factor, float exponent, float* out, int Lout,
                               float scale_out, float* tracks, void* stream) {
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
    const Stacks st{reinterpret_cast<const float2*>(chunks_c64), K, overlap_geom(Tc, hop), factor, exponent,
                    DrawLayout{D, 1.f / (float)D, stack_rows, draw_rows}};
    const int rc = launch_istft(StackOutputs{st, (int)Tg, Lout, out, scale_out}, (Lout + HOP - 1) / HOP, S, stream);
    if (rc != OK || !tracks) return rc;
    hipLaunchKernelGGL(ensemble_tracks_kernel, dim3((unsigned)((Tg + 63) / 64), S), dim3(256), 0,
                       static_cast<hipStream_t>(stream), st, (int)Tg, tracks);
    FLOWSE_LAUNCH_CHECK();
    return OK;
}

int flowse_istft_decompress_chunks(const void* chunks_c64, int K, int Tc, int hop, float factor, float exponent, float* out,
                                   int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_chunks: null argument");
        return ERR_ARG;
    }
    return launch_istft_stacks("chunks", static_cast<const float*>(chunks_c64), 1, 1, K, Tc, hop, K, 0, factor, exponent, out,
                               Lout, scale_out, nullptr, stream);
}

// the chunk synthesis for S stacks of one geometry in one launch: [S][K][256][Tc] -> [S][Lout]
int flowse_istft_decompress_stacks(const void* chunks_c64, int S, int K, int Tc, int hop, float factor, float exponent,
                                   float* out, int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_stacks: null argument");
        return ERR_ARG;
    }
    return launch_istft_stacks("stacks", static_cast<const float*>(chunks_c64), S, 1, K, Tc, hop, K, 0, factor, exponent, out,
                               Lout, scale_out, nullptr, stream);
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
                               factor, exponent, out, Lout, scale_out, tracks, stream);
}

// the R rows [R,1,256,Tw] of one sampler call from up to FLOWSE_MAX_SPEC_ROWS signals; `rows`: HOST table
int flowse_stft_compress_rows(const flowse_spec_row* rows, int R, int Tw, void* out_c64, float factor, float exponent,
                              void* stream) {
    if (!rows || !out_c64) {
        set_error("flowse_stft_compress_rows: null argument");
        return ERR_ARG;
    }
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
    return launch_stft(t, Tw, R, out_c64, factor, exponent, stream);
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
    int64_t T = 0;
    const int rc = check_stft_window("stft window", s0, n, frame0, Tc, L_total, &T);
    if (rc != OK) return rc;
    return launch_stft(AffineRows{{buf, s0, L_total >= 0 ? L_total : INT64_MAX / 4, frame0, T, scale_in}, 0, 0}, Tc, 1, out_c64,
                       factor, exponent, stream);
}

// The shape checks of one output range [e0, e0 + n_out) after chunk k, past the entry's own argument checks, for either
// geometry; on success *fr is what the kernel reads for it.  `who` names the entry (and the row); `open_note` ends the error text
// while the recording is open: the first frame that waits for chunk k + 1, in the entry's own symbols.
static int check_istft_window(const char* who, const char* open_note, const void* prev2_c64, const void* prev_c64,
                              const void* cur_c64, int64_t k, const ChunkGeom& g, int last, int64_t L, float factor,
                              float exponent, int64_t e0, int64_t n_out, ChunkWindow<WindowRows>* fr) {
    const int64_t Tg = (k + 1) * g.H + g.shift;         // frames of a recording that ends with chunk k
    if (last && (e0 + n_out > L || L > (Tg - 1) * HOP + NFFT - PADC)) {
        set_error("%s: after the last chunk need e0 + n_out <= L <= 128 (Tg - 1) + 255 (got e0=%lld n_out=%lld "
                  "L=%lld Tg=%lld)", who, (long long)e0, (long long)n_out, (long long)L, (long long)Tg);
        return ERR_SHAPE;
    }
    // the frames over the samples [e0, e0 + n_out): the index range of istft_gather for one sample, over all of them
    const int64_t t_first = e0 <= NFFT - 1 - PADC ? 0 : (e0 - (NFFT - 1 - PADC) + HOP - 1) / HOP;
    int64_t t_last = (e0 + n_out - 1 + PADC) / HOP;
    if (last && t_last > Tg - 1) t_last = Tg - 1;
    // the chunks the seam rule reads for them: the owner of a frame, and the chunk before it inside the fade; both grow with t
    int64_t c_hi = (t_last - g.shift + g.X) / g.H, c_lo = (t_first - g.shift + g.X) / g.H;
    if (last && c_hi > k) c_hi = k;
    if (last && c_lo > k) c_lo = k;
    if (c_lo > 0 && t_first - g.shift < c_lo * g.H) c_lo -= 1;
    const int64_t m = k >= 2 ? k - 2 : 0;
    if (c_hi > k || c_lo < m || (c_lo <= k - 1 && !prev_c64) || (c_lo <= k - 2 && !prev2_c64)) {
        set_error("%s: samples [%lld, %lld) lie under frames [%lld, %lld], which the seam rule takes from chunks "
                  "%lld..%lld; given are chunk k=%lld%s%s%s", who, (long long)e0, (long long)(e0 + n_out),
                  (long long)t_first, (long long)t_last, (long long)c_lo, (long long)c_hi, (long long)k,
                  (k >= 1 && prev_c64) ? ", k-1" : "", (k >= 2 && prev2_c64) ? ", k-2" : "",
                  last ? " (the last)" : open_note);
        return ERR_SHAPE;
    }
    const float2* given[3] = {reinterpret_cast<const float2*>(prev2_c64), reinterpret_cast<const float2*>(prev_c64),
                              reinterpret_cast<const float2*>(cur_c64)};
    const int held = (int)(k - m) + 1;                  // chunks m .. k
    for (int i = 0; i < 3; ++i) fr->rows.c[i] = i < held ? given[3 - held + i] : nullptr;
    fr->T = last ? Tg : INT64_MAX / 4;
    fr->base = m * g.H;
    fr->t_lo = t_first;
    fr->t_hi = t_last + 1;
    fr->Kw = held + (last ? 0 : 1);
    fr->g = g;
    fr->factor = factor;
    fr->exponent = exponent;
    return OK;
}

// the overlap entries' own argument checks, then the above
static int check_overlap_window(const char* who, const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k,
                                int Tc, int hop, int last, int64_t L, float factor, float exponent, int64_t e0, int64_t n_out,
                                ChunkWindow<WindowRows>* fr) {
    if (k < 0 || k > WINDOW_MAX || Tc < 1 || Tc > (1 << 23) || hop < 1 || hop > Tc || 2 * (int64_t)hop < Tc || e0 < 0 ||
        n_out < 1 || n_out > ((int64_t)1 << 30) || e0 > WINDOW_MAX * HOP || factor == 0.f) {
        set_error("%s: need 0 <= k <= 2^40, 1 <= hop <= Tc <= 2 hop, Tc <= 2^23, e0 >= 0, 1 <= n_out <= 2^30 and "
                  "factor != 0 (got k=%lld Tc=%d hop=%d e0=%lld n_out=%lld)", who, (long long)k, Tc, hop, (long long)e0,
                  (long long)n_out);
        return ERR_SHAPE;
    }
    return check_istft_window(who, " (not the last: frames from (k+1) hop on wait for chunk k+1)", prev2_c64, prev_c64, cur_c64,
                              k, overlap_geom(Tc, hop), last, L, factor, exponent, e0, n_out, fr);
}

int flowse_istft_decompress_window(const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k, int Tc,
                                   int hop, int last, int64_t L, float factor, float exponent, float* out, int64_t e0,
                                   int64_t n_out, float scale_out, void* stream) {
    if (!cur_c64 || !out) {
        set_error("flowse_istft_decompress_window: null argument");
        return ERR_ARG;
    }
    OutputRange<ChunkWindow<WindowRows>> range{{}, out, e0, n_out, scale_out};
    const int rc = check_overlap_window("istft window", prev2_c64, prev_c64, cur_c64, k, Tc, hop, last, L, factor, exponent, e0,
                                        n_out, &range.frames);
    if (rc != OK) return rc;
    return launch_istft(range, (e0 + n_out - 1) / HOP - e0 / HOP + 1, 1, stream);
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
    const int T = L / HOP + 1;
    if (L <= PADC || !trailing_ok(Tc, H, -1) || K < 1 || K > 65535 || (int64_t)K * H < T || (int64_t)K * H + Tc > (1 << 23)) {
        set_error("flowse_stft_compress_trailing: need L > %d, " TRAILING_GEOMETRY ", 1 <= K <= 65535 and L / %d + 1 <= K H <= "
                  "2^23 - Tc (got L=%d K=%d Tc=%d H=%d)", PADC, HOP, L, K, Tc, H);
        return ERR_SHAPE;
    }
    // row b = chunk b, from frame b H - P on
    return launch_stft(AffineRows{{sig, 0, L, (int64_t)H - Tc, T, scale_in}, 0, H}, Tc, K, out_c64, factor, exponent, stream);
}

int flowse_istft_decompress_trailing(const void* chunks_c64, int K, int Tc, int H, int X, float factor, float exponent,
                                     float* out, int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_trailing: null argument");
        return ERR_ARG;
    }
    const int64_t Tg = (int64_t)K * H;
    if (!trailing_ok(Tc, H, X) || X < 0 || K < 1 || K > 65535 || Tg + Tc > (1 << 23) || Lout < 1 ||
        Lout > (Tg - 1) * HOP + NFFT - PADC || factor == 0.f) {
        set_error("flowse_istft_decompress_trailing: need " TRAILING_GEOMETRY ", 0 <= X <= H, H + X <= Tc, 1 <= K <= 65535, "
                  "K H <= 2^23 - Tc, 1 <= Lout <= 128 (K H - 1) + 255 and factor != 0 (got K=%d Tc=%d H=%d X=%d Lout=%d)", K, Tc,
                  H, X, Lout);
        return ERR_SHAPE;
    }
    const ChunkWindow<StackRows> frames{StackRows{reinterpret_cast<const float2*>(chunks_c64), Tc}, Tg, 0, 0, Tg, K,
                                        trailing_geom(Tc, H, X), factor, exponent};
    return launch_istft(OutputRange<ChunkWindow<StackRows>>{frames, out, 0, Lout, scale_out}, (Lout + HOP - 1) / HOP, 1, stream);
}

int flowse_stft_compress_trailing_window(const float* buf, int64_t s0, int64_t n, float scale_in, int64_t k, int Tc, int H,
                                         int64_t L_total, void* out_c64, float factor, float exponent, void* stream) {
    if (!buf || !out_c64) {
        set_error("flowse_stft_compress_trailing_window: null argument");
        return ERR_ARG;
    }
    if (!trailing_ok(Tc, H, -1) || k < 0 || k > WINDOW_MAX / H - 1) {
        set_error("flowse_stft_compress_trailing_window: need " TRAILING_GEOMETRY " and 0 <= k, (k + 1) H <= 2^40 (got k=%lld "
                  "Tc=%d H=%d)", (long long)k, Tc, H);
        return ERR_SHAPE;
    }
    // the frames that read samples start at max(k H - P, 0): the checks of the plain window over those
    const int64_t frame0 = k * H - (Tc - H), first = frame0 < 0 ? 0 : frame0;
    int64_t T = 0;
    const int rc = check_stft_window("flowse_stft_compress_trailing_window", s0, n, first, (int)(frame0 + Tc - first), L_total, &T);
    if (rc != OK) return rc;
    return launch_stft(AffineRows{{buf, s0, L_total >= 0 ? L_total : INT64_MAX / 4, frame0, T, scale_in}, 0, 0}, Tc, 1, out_c64,
                       factor, exponent, stream);
}

int flowse_istft_decompress_trailing_window(const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k, int Tc,
                                            int H, int X, int last, int64_t L, float factor, float exponent, float* out,
                                            int64_t e0, int64_t n_out, float scale_out, void* stream) {
    const char* who = "flowse_istft_decompress_trailing_window";
    if (!cur_c64 || !out) {
        set_error("%s: null argument", who);
        return ERR_ARG;
    }
    if (!trailing_ok(Tc, H, X) || X < 0 || k < 0 || k > WINDOW_MAX / H - 1 || e0 < 0 || n_out < 1 ||
        n_out > ((int64_t)1 << 30) || e0 > WINDOW_MAX * HOP || factor == 0.f) {
        set_error("%s: need " TRAILING_GEOMETRY ", 0 <= X <= H, H + X <= Tc, 0 <= k, (k + 1) H <= 2^40, e0 >= 0, 1 <= n_out <= "
                  "2^30 and factor != 0 (got k=%lld Tc=%d H=%d X=%d e0=%lld n_out=%lld)", who, (long long)k, Tc, H, X,
                  (long long)e0, (long long)n_out);
        return ERR_SHAPE;
    }
    OutputRange<ChunkWindow<WindowRows>> range{{}, out, e0, n_out, scale_out};
    const int rc = check_istft_window(who, " (not the last: frames from (k+1) H - X on wait for chunk k+1)", prev2_c64, prev_c64,
                                      cur_c64, k, trailing_geom(Tc, H, X), last, L, factor, exponent, e0, n_out, &range.frames);
    if (rc != OK) return rc;
    return launch_istft(range, (e0 + n_out - 1) / HOP - e0 / HOP + 1, 1, stream);
}

// ---- the windows of several sessions in one launch each (flowmse_amd.livepool); `rows`: HOST tables ---------------------
int flowse_stft_compress_window_rows(const flowse_window_row* rows, int R, int Tw, void* out_c64, float factor,
                                     float exponent, void* stream) {
    if (!rows || !out_c64) {
        set_error("flowse_stft_compress_window_rows: null argument");
        return ERR_ARG;
    }
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
        t.row[r] = SignalRow{w.buf, w.s0, w.L_total >= 0 ? w.L_total : INT64_MAX / 4, w.frame0, T, w.scale_in};
    }
    return launch_stft(t, Tw, R, out_c64, factor, exponent, stream);
}

int flowse_istft_decompress_window_rows(const flowse_window_out* rows, int R, int Tc, int hop, float factor, float exponent,
                                        void* stream) {
    if (!rows) {
        set_error("flowse_istft_decompress_window_rows: null argument");
        return ERR_ARG;
    }
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
        ChunkWindow<WindowRows> fr;
        const int rc = check_overlap_window(who, w.prev2_c64, w.prev_c64, w.cur_c64, w.k, Tc, hop, w.last, w.L, factor, exponent,
                                            w.e0, w.n_out, &fr);
        if (rc != OK) return rc;
        t.row[r] = WindowOutRow{fr.rows, fr.T, fr.base, fr.t_lo, fr.t_hi, w.out, w.e0, w.n_out, fr.Kw, w.scale_out};
        const int64_t b = (w.e0 + w.n_out - 1) / HOP - w.e0 / HOP + 1;
        if (b > blocks) blocks = b;
    }
    t.g = overlap_geom(Tc, hop);
    t.factor = factor;
    t.exponent = exponent;
    return launch_istft(t, blocks, R, stream);
}

}  // extern "C"
