// Internal types of the model handle: NCSN++ module list, parameter table, launch plan (model_*.hip), and the six
// functions through which the entries that live beside their kernels reach the handle (at the end).
#pragma once
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/flowse_hip.h"
#include "common.h"

namespace flowse {

// ------------------------------------------------------------------------------------------- structure
enum ModKind { M_GFP, M_LINEAR, M_CONV3, M_RESBLOCK, M_ATTN, M_COMBINE, M_GN };

struct ParamInfo {
    std::string name;
    int ndim;
    int64_t shape[4];
    int64_t offset, numel;
};

struct Module {
    ModKind kind;
    int in_ch = 0, out_ch = 0;
    bool up = false, down = false, shortcut = false;
    int p0 = 0;            // index of the module's first parameter
    // offsets (floats) into the native device weight blob
    int64_t w_gn0_g = -1, w_gn0_b = -1, w_gn1_g = -1, w_gn1_b = -1;
    int64_t w_c0 = -1, w_c1 = -1, w_c1_b = -1, w_c2 = -1, w_c2_b = -1;
    int64_t w_a = -1, w_a_b = -1;      // generic weight / bias (linear, conv3, combine, gfp, gn gamma/beta)
    int64_t w_qkv = -1, w_qkv_b = -1, w_o = -1, w_o_b = -1;
    int dense_row0 = -1;               // first row of this block in the stacked Dense_0 table
    int64_t wq_c0 = -1, wq_c1 = -1;    // offsets (uint16 elements) of the bf16 planes of Conv_0 / Conv_1, if packed
};

struct Tn {
    size_t off = 0;
    int B = 0, H = 0, W = 0, C = 0;
    size_t st_off = 0;      // fused GroupNorm partials written by the producing conv (st_nblk blocks per sample)
    int st_nblk = 0;
    int dt = DT_F32;        // storage type of the elements (DT_*)
    size_t bytes() const { return (size_t)B * H * W * C * dt_size(dt); }
    bool valid() const { return B > 0; }
};

class Arena {
   public:
    size_t alloc(size_t n) {
        n = (n + 255) & ~(size_t)255;
        for (size_t i = 0; i < free_.size(); ++i) {
            if (free_[i].second >= n) {
                const size_t off = free_[i].first;
                if (free_[i].second == n) free_.erase(free_.begin() + i);
                else { free_[i].first += n; free_[i].second -= n; }
                live_[off] = n;
                return off;
            }
        }
        // extend (merge with a trailing free block if it touches the end)
        size_t off = end_;
        if (!free_.empty() && free_.back().first + free_.back().second == end_) {
            off = free_.back().first;
            free_.pop_back();
        }
        end_ = off + n;
        if (end_ > peak_) peak_ = end_;
        live_[off] = n;
        return off;
    }
    void release(size_t off) {
        auto it = live_.find(off);
        if (it == live_.end()) return;
        const size_t n = it->second;
        live_.erase(it);
        size_t i = 0;
        while (i < free_.size() && free_[i].first < off) ++i;
        free_.insert(free_.begin() + i, std::make_pair(off, n));
        if (i + 1 < free_.size() && free_[i].first + free_[i].second == free_[i + 1].first) {
            free_[i].second += free_[i + 1].second;
            free_.erase(free_.begin() + i + 1);
        }
        if (i > 0 && free_[i - 1].first + free_[i - 1].second == free_[i].first) {
            free_[i - 1].second += free_[i].second;
            free_.erase(free_.begin() + i);
        }
    }
    size_t peak() const { return peak_; }

   private:
    std::vector<std::pair<size_t, size_t>> free_;   // sorted by offset
    std::map<size_t, size_t> live_;
    size_t end_ = 0, peak_ = 0;
};

struct Plan {
    int B = 0, F = 0, T = 0;
    size_t ws_bytes = 0;
    std::vector<std::function<int(hipStream_t)>> ops;
    std::vector<std::string> labels;
    std::vector<double> flops, bytes;      // algorithmic work / HBM traffic of each launch
    std::vector<double> issued;            // FLOPs the matrix cores execute for it (Winograd forms: 1/2 or 2/3 of `flops`)
    std::vector<char> dominant;            // 1 = a launch of the dominant kernel: the unsplit 3x3 ResBlock conv with fused
                                           // GroupNorm+SiLU input (conv3x3_f43_kernel<2, false, 2> in the fp32 mode)
    // The launch list holds no per-call argument (those live in the handle's device-resident CallBlock): by default it is
    // issued as plain launches; under FLOWSE_GRAPH=1 it is captured after one eager pass and replayed as a hipGraph.
    int eager_runs = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// One device allocation with its capacity in elements; p is null exactly when n is 0.  Grow-only, never copied.  The
// destructor does not free: free_device_state (model_api.hip) releases every buffer with the owning device current.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    operator T*() const { return p; }
    size_t bytes() const { return n * sizeof(T); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    // Room for `need` elements; growing discards the contents.  sync_first: the device may still be using the old buffer.
    // A failed allocation leaves the buffer empty.
    int reserve(size_t need, bool sync_first) {
        if (need <= n) return OK;
        if (sync_first) FLOWSE_HIP(hipDeviceSynchronize());
        release();
        FLOWSE_HIP(hipMalloc(reinterpret_cast<void**>(&p), need * sizeof(T)));
        n = need;
        return OK;
    }
};

struct ProfAcc {
    int64_t launches = 0;
    double ms = 0.0, flops = 0.0, bytes = 0.0, issued = 0.0;
};

// Everything that is derived from the weights: the device buffers and the host tables that index them.  One set may be
// referred to by several handles (flowse_model_view_create); it is freed with its last holder.  Handles of one set are
// used from one host thread at a time, so the count is a plain int.
struct WeightSet {
    int holders = 1;                       // live handles that refer to this set
    std::vector<Module> mods;
    std::vector<ParamInfo> params;
    int64_t blob_numel = 0;
    int out_w_p = 0;                       // parameter index of output_layer.weight
    int temb_dim = 0, dense_rows = 0;
    int64_t w_dense = -1, w_dense_b = -1;  // stacked Dense_0 (+ folded Conv_0.bias)
    int64_t w_out = -1, w_out_b = -1;
    // device state
    DevBuf<float> d_w;                     // native weight blob
    int precision = 0;                     // 0 fp32 (exact), 1 bf16x3 split (fp32-class), 2 bf16, 3 fp16 operands
    DevBuf<uint16_t> d_wq;                 // bf16 planes of the 3x3 ResBlock convs (precision != 0)
    // 16-bit STORAGE modes (precision 2 / 3 on networks whose wide channel counts are multiples of 32): activations
    // between kernels are bf16 / half; d_w16 is an elementwise 16-bit copy of the packed weight blob d_w (same offsets)
    int act_dt = DT_F32;
    DevBuf<uint16_t> d_w16;
    // The derived copies of the conv weights, one per entry of conv_copy (common.h): at[w] = element offset in buf of the copy
    // of the conv at packed offset w, for exactly the convs whose rule (ConvCopy::gets) held at the last upload.  The mirrors
    // (ConvCopy::mirror) are blob-sized with at[w] = w; the others are packed, each entry rounded up to 64 elements.
    struct Copy {
        DevBuf<char> buf;
        std::map<int64_t, int64_t> at;
    } copies[CW_COPIES];
    bool has_copy(int k, int64_t w) const { return copies[k].at.count(w) != 0; }
    const void* copy_ptr(int k, int64_t w) const {       // null: the conv has no such copy
        const auto it = copies[k].at.find(w);
        return it == copies[k].at.end() ? nullptr : copies[k].buf.p + it->second * conv_copy(k).esize;
    }
    int device = -1;                       // HIP device that owns every d_* buffer of the set and of its handles
    bool storage16() const { return act_dt != DT_F32; }
};

}  // namespace flowse

using namespace flowse;

struct flowse_model {
    flowse_config cfg;
    WeightSet* wt = nullptr;               // never null; shared with the parent when is_view
    bool is_view = false;                  // made by flowse_model_view_create: may not load weights or change the precision
    DevBuf<char> d_ws;                     // activation workspace
    DevBuf<float> d_ts;                    // [N][B] solver times
    std::map<std::tuple<int, int, int>, Plan> plans;
    DevBuf<CallBlock> d_call;              // per-call arguments of the boundary kernels, in device memory
    bool use_graph = false;                // FLOWSE_GRAPH=1: replay each shape's launch list as a hipGraph (slower, measured)
    // Callers on the NULL (legacy default) stream -- PyTorch's default stream IS the NULL stream -- cannot be captured;
    // their work runs on this internal stream instead, fenced against the NULL stream by events on both sides.
    hipStream_t gstream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    int64_t graph_launches = 0;            // hipGraphLaunch calls made by this handle (flowse_model_graph_launches)
    DevBuf<float> d_rk;                    // fixed-step RK scratch: stage input + slope accumulator, 2 x [B,1,F,T] complex64
    DevBuf<char> d_rk45;                   // adaptive RK45 state (flowse_rk45_sample): y, y_new, K1..K7, stage input, norms
    DevBuf<char> d_fm;                     // flowse_fm_loss: x_t, v (complex64 [B,1,F,T] each) and the loss partials; first use
    // single-module handles (flowse_block_create): one ResnetBlockBigGANpp / AttnBlockpp / Combine behind the same
    // weight packer, plan builder and kernels as the full network -- unit parity against the reference's modules
    int block_kind = -1;                   // -1: full network; else FLOWSE_BLOCK_*
    struct BlockCall { const float* in1 = nullptr; const float* in2 = nullptr; const float* temb_act = nullptr;
                       float* out = nullptr; } bcall;
    std::map<std::tuple<int, int, int, int>, Plan> block_plans;      // (B, H, W, C1)
    // optional in-library profiler (flowse_profile_begin / _end): HIP events around selected launches
    int prof_mode = -1;                    // -1 off, 0 dominant kernel only, 1 every op
    std::vector<hipEvent_t> prof_pool;     // reusable events
    size_t prof_used = 0;
    struct Pending { int label; hipEvent_t a, b; double flops, bytes, issued; };
    std::vector<Pending> prof_pending;
    std::vector<std::string> prof_labels;
    std::map<std::string, int> prof_label_ix;
    double prof_tot_flops = 0.0, prof_tot_issued = 0.0;    // over every launch between _begin and _end
    int64_t prof_tot_launches = 0;

    float* W(int64_t off) const { return wt->d_w + off; }
    float* A(size_t off) const { return reinterpret_cast<float*>(d_ws + off); }
    bool storage16() const { return wt->storage16(); }
};

namespace flowse {

// model_build.hip
int build_structure(flowse_model* m);
void add_module(flowse_model* m, Module mod);
Module resblock_module(int in_ch, int out_ch, bool up = false, bool down = false);
Module simple_module(ModKind k, int in_ch, int out_ch);
struct Packer {
    std::vector<float> host;
    struct Conv { int64_t off; int Cout, Cin, taps; };
    std::vector<Conv> convs;               // every conv weight of the blob (the attention projections are 1x1 convs)
    int64_t put(int64_t n) {
        const int64_t off = ((int64_t)host.size() + 63) & ~(int64_t)63;
        host.resize(off + n, 0.f);
        return off;
    }
};
int pack_weights(flowse_model* m, const float* blob, Packer& pk);
int storage_type_for(const flowse_model* m);
// model_plan.hip
int build_plan(flowse_model* m, Plan* plan, int B, int F, int T);
int build_block_plan(flowse_model* m, Plan* plan, int B, int H, int W, int C1);
// model_api.hip, the handle proper: life cycle, weight upload, plan lookup and execution, the stream fence, the profiler.
// These six functions are all that the entries of the other files (rk_fixed.hip, rk45.hip, fmloss.hip) see of it:
// get_plan also grows the workspace (it may synchronise the device); exec_plan may replay a captured graph, run_plan
// always issues plain launches; ensure_stream makes the handle's internal stream and its two fence events.
int get_plan(flowse_model* m, int B, int F, int T, Plan** out);
int exec_plan(flowse_model* m, Plan* p, hipStream_t s);
int run_plan(flowse_model* m, Plan* p, hipStream_t s);
int ensure_stream(flowse_model* m);
int enter_stream(flowse_model* m, hipStream_t caller, hipStream_t* work);
int leave_stream(flowse_model* m, hipStream_t caller, hipStream_t work);

// The stream scope of one C-ABI call: body(s) runs between enter_stream and leave_stream, on the stream enter_stream
// chose.  Returns the body's error if there is one, otherwise leave_stream's.  Whatever may synchronise or allocate
// (get_plan, every reserve) belongs before the scope.
template <class Fn>
inline int on_handle_stream(flowse_model* m, void* stream, Fn body) {
    hipStream_t caller = static_cast<hipStream_t>(stream), s = nullptr;
    if (const int rc = enter_stream(m, caller, &s)) return rc;
    const int rc = body(s);
    const int rc2 = leave_stream(m, caller, s);
    return rc != OK ? rc : rc2;
}

}  // namespace flowse
