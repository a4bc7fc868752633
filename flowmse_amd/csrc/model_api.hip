// Model handle, part 3: plan execution (plain launches, optional hipGraph replay), device state and the C ABI
// (include/flowse_hip.h).
#include "model.h"

namespace flowse {

static void drop_graph(Plan* p) {
    if (p->exec) (void)hipGraphExecDestroy(p->exec);
    if (p->graph) (void)hipGraphDestroy(p->graph);
    p->exec = nullptr;
    p->graph = nullptr;
    p->eager_runs = 0;
}

static void clear_plans(flowse_model* m) {
    for (auto& kv : m->plans) drop_graph(&kv.second);
    m->plans.clear();
    m->block_plans.clear();
}

// every device call of a handle must be made with the handle's device current (the buffers live there)
static int check_device(const flowse_model* m) {
    int dev = 0;
    FLOWSE_HIP(hipGetDevice(&dev));
    if (m->wt->device >= 0 && dev != m->wt->device) {
        set_error("model handle is bound to HIP device %d but device %d is current (reload the weights on the new "
                  "device, or hipSetDevice back)", m->wt->device, dev);
        return ERR_STATE;
    }
    return OK;
}

static int check_ready(const flowse_model* m) {
    if (!m->wt->d_w) {
        set_error("weights not loaded: call flowse_model_load_weights first");
        return ERR_STATE;
    }
    return check_device(m);
}

// Growing the workspace: the stream may still be using the old one, and captured graphs point into it (block handles
// hold none).
static int reserve_workspace(flowse_model* m, size_t bytes) {
    if (bytes <= m->d_ws.n) return OK;
    FLOWSE_HIP(hipDeviceSynchronize());
    for (auto& kv : m->plans) drop_graph(&kv.second);
    return m->d_ws.reserve(bytes, false);
}

int get_plan(flowse_model* m, int B, int F, int T, Plan** out) {
    if (const int rc = check_ready(m)) return rc;
    auto key = std::make_tuple(B, F, T);
    auto it = m->plans.find(key);
    if (it == m->plans.end()) {
        Plan p;
        const int rc = build_plan(m, &p, B, F, T);
        if (rc != OK) return rc;
        it = m->plans.emplace(key, std::move(p)).first;
    }
    *out = &it->second;
    return reserve_workspace(m, it->second.ws_bytes);
}

static int prof_event(flowse_model* m, hipEvent_t* e) {
    if (m->prof_used == m->prof_pool.size()) {
        hipEvent_t ev;
        FLOWSE_HIP(hipEventCreate(&ev));
        m->prof_pool.push_back(ev);
    }
    *e = m->prof_pool[m->prof_used++];
    return OK;
}

static int run_plan(flowse_model* m, Plan* p, hipStream_t s) {
    if (m->prof_mode != -1) {
        for (size_t i = 0; i < p->ops.size(); ++i) {
            m->prof_tot_flops += p->flops[i];
            m->prof_tot_issued += p->issued[i];
        }
        m->prof_tot_launches += (int64_t)p->ops.size();
    }
    for (size_t i = 0; i < p->ops.size(); ++i) {
        const bool prof = m->prof_mode == 1 || (m->prof_mode == 0 && p->dominant[i]);
        flowse_model::Pending pd;
        if (prof) {
            const std::string& name = (m->prof_mode == 0) ? std::string("dominant_conv3x3") : p->labels[i];
            auto it = m->prof_label_ix.find(name);
            if (it == m->prof_label_ix.end()) {
                it = m->prof_label_ix.emplace(name, (int)m->prof_labels.size()).first;
                m->prof_labels.push_back(name);
            }
            pd.label = it->second;
            pd.flops = p->flops[i];
            pd.bytes = p->bytes[i];
            pd.issued = p->issued[i];
            int rc = prof_event(m, &pd.a);
            if (rc != OK) return rc;
            rc = prof_event(m, &pd.b);
            if (rc != OK) return rc;
            FLOWSE_HIP(hipEventRecord(pd.a, s));
        }
        const int rc = p->ops[i](s);
        if (rc != OK) return rc;
        if (prof) {
            FLOWSE_HIP(hipEventRecord(pd.b, s));
            m->prof_pending.push_back(pd);
        }
    }
    return OK;
}

// One network evaluation.  Default: plain launches of the shape's launch list.  FLOWSE_GRAPH=1 (opt-in: measured 5 %
// slower than plain launches at batch 1, equal at batch 8): first call per shape eager (also performs the one-time
// per-device kernel attribute setup), second call captures the same launch list into a hipGraph, afterwards one
// hipGraphLaunch per call.  Profiling (per-launch events) always runs plain launches.
int exec_plan(flowse_model* m, Plan* p, hipStream_t s) {
    if (!m->use_graph || m->prof_mode != -1 || s == nullptr) return run_plan(m, p, s);   // (NULL: see enter_stream)
    if (p->exec) {
        FLOWSE_HIP(hipGraphLaunch(p->exec, s));
        ++m->graph_launches;
        return OK;
    }
    if (p->eager_runs < 1) {
        ++p->eager_runs;
        return run_plan(m, p, s);
    }
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();                    // e.g. the caller's stream is already capturing: stay eager
        m->use_graph = false;
        return run_plan(m, p, s);
    }
    const int rc = run_plan(m, p, s);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc != OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) {                    // capture refused: stay eager for this plan
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        m->use_graph = false;
        return run_plan(m, p, s);
    }
    hipGraphExec_t ex = nullptr;
    if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess || !ex) {
        (void)hipGetLastError();
        (void)hipGraphDestroy(g);
        m->use_graph = false;
        return run_plan(m, p, s);
    }
    p->graph = g;
    p->exec = ex;
    FLOWSE_HIP(hipGraphLaunch(p->exec, s));
    ++m->graph_launches;
    return OK;
}

// The handle's internal stream and its two fence events, made on first use.  The stream is non-blocking: a blocking one
// would serialise against the NULL stream, which is where PyTorch's default stream puts the caller's work.
static int ensure_stream(flowse_model* m) {
    if (!m->gstream) FLOWSE_HIP(hipStreamCreateWithFlags(&m->gstream, hipStreamNonBlocking));
    if (!m->ev_in) FLOWSE_HIP(hipEventCreateWithFlags(&m->ev_in, hipEventDisableTiming));
    if (!m->ev_out) FLOWSE_HIP(hipEventCreateWithFlags(&m->ev_out, hipEventDisableTiming));
    return OK;
}
// Stream the work of one C-ABI call runs on.  A real stream: that stream.  The NULL stream: it cannot be captured, so
// (unless graphs are off / a profile is being taken) the call moves to the handle's internal stream, which first waits
// for everything the caller has enqueued on the NULL stream; leave_stream() makes the NULL stream wait for the call.
int enter_stream(flowse_model* m, hipStream_t caller, hipStream_t* work) {
    *work = caller;
    if (caller != nullptr || !m->use_graph || m->prof_mode != -1) return OK;
    if (const int rc = ensure_stream(m)) return rc;
    FLOWSE_HIP(hipEventRecord(m->ev_in, nullptr));
    FLOWSE_HIP(hipStreamWaitEvent(m->gstream, m->ev_in, 0));
    *work = m->gstream;
    return OK;
}
int leave_stream(flowse_model* m, hipStream_t caller, hipStream_t work) {
    if (work == caller) return OK;
    FLOWSE_HIP(hipEventRecord(m->ev_out, work));
    FLOWSE_HIP(hipStreamWaitEvent(caller, m->ev_out, 0));
    return OK;
}

// f(buffer) for every device buffer the handle itself holds / of a weight set: the one list of each that the release and
// the byte count (flowse_model_device_bytes) go through
template <class M, class Fn>
static void each_owned_buffer(M* m, Fn f) {
    f(m->d_ws); f(m->d_ts); f(m->d_call); f(m->d_rk); f(m->d_rk45); f(m->d_fm);
}
template <class W, class Fn>
static void each_weight_buffer(W* w, Fn f) {
    f(w->d_w); f(w->d_wq); f(w->d_w16); f(w->d_wfrag); f(w->d_wino); f(w->d_wino2); f(w->d_wsm); f(w->d_wsm16);
}

// The buffers only this handle holds: workspace, plans, time table, RK scratch, CallBlock, stream, events, profiler.
// Called with the set's device current and idle.
static void free_owned_state(flowse_model* m) {
    clear_plans(m);
    each_owned_buffer(m, [](auto& b) { b.release(); });
    if (m->gstream) (void)hipStreamDestroy(m->gstream);
    if (m->ev_in) (void)hipEventDestroy(m->ev_in);
    if (m->ev_out) (void)hipEventDestroy(m->ev_out);
    m->gstream = nullptr;
    m->ev_in = m->ev_out = nullptr;
    for (hipEvent_t e : m->prof_pool) (void)hipEventDestroy(e);
    m->prof_pool.clear();
    m->prof_used = 0;
}

// Every device buffer of a weight set; the host tables stay (the next upload rewrites them).
static void free_weight_buffers(WeightSet* w) {
    each_weight_buffer(w, [](auto& b) { b.release(); });
    w->device = -1;
}

// Frees what the handle owns and, when it is the set's only holder, the weight buffers too (the handle keeps its, now
// empty, set).  A handle whose set has other holders only lets go of its own buffers.
static void free_device_state(flowse_model* m) {
    WeightSet* w = m->wt;
    int cur = 0;
    const bool sw = w->device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != w->device;
    if (sw) (void)hipSetDevice(w->device);
    if (w->device >= 0) (void)hipDeviceSynchronize();
    free_owned_state(m);
    if (w->holders == 1) free_weight_buffers(w);
    if (sw) (void)hipSetDevice(cur);
}

// ---------------------------------------------------------------------------------- fixed-step RK, one evaluation at a time
// The network evaluations of one solve over the reference's grid.  A step that ends at (or numerically below) t = 0 is
// the reference's own Euler update: the field divides by t and embeds log t, so no stage may be evaluated at the end
// point of such a step (it is the LAST step of the reference's grid, whose length equals the last grid time,
// sampling/__init__.py:53).
struct RkGrid {
    int stages;
    std::vector<float> nfe_t;               // time of every network evaluation, in order
    struct Eval { int step, stage, of; float h; };
    std::vector<Eval> evals;
    RkGrid(const float* ts, const float* dts, int N, int tableau)
        : stages(tableau == FLOWSE_TABLEAU_RK4 ? 4 : tableau == FLOWSE_TABLEAU_HEUN ? 2 : 1) {
        for (int i = 0; i < N; ++i) {
            const float t = ts[i], h = dts[i];
            const bool lands = (double)t - (double)h <= 1e-6 * std::max(1.0, std::fabs((double)t));
            const int st = lands ? 1 : stages;
            const float dt = -h;
            nfe_t.push_back(t);
            if (st == 2) nfe_t.push_back(t + dt);
            if (st == 4) {
                const float th = t + 0.5f * dt;
                nfe_t.push_back(th);
                nfe_t.push_back(th);
                nfe_t.push_back(t + dt);
            }
            for (int j = 0; j < st; ++j) evals.push_back(Eval{i, j, st, h});
        }
    }
};

// time table and RK scratch of one [B,1,F,T] solve on handle m (growth synchronises the device)
static int reserve_rk(flowse_model* m, const RkGrid& g, int B, int F, int T) {
    if (const int rc = m->d_ts.reserve(g.nfe_t.size() * (size_t)B, true)) return rc;
    const size_t state = (size_t)2 * B * F * T;                 // floats of one complex64 [B,1,F,T] tensor
    return m->d_rk.reserve(g.stages > 1 ? 2 * state : 0, true);
}

struct RkRun {
    flowse_model* m = nullptr;
    Plan* p = nullptr;
    float* x = nullptr;
    const float* y = nullptr;
    int B = 0, F = 0, T = 0;
    size_t k = 0;                                                // index of the next network evaluation
    bool done(const RkGrid& g) const { return k == g.evals.size(); }
    // Enqueues evaluation k (before the first one, the table of times) on s.  may_graph: through exec_plan, which may
    // replay a captured graph; otherwise always plain launches.
    int issue(const RkGrid& g, hipStream_t s, bool may_graph) {
        if (k == 0) {
            // vec_t = ones(B) * t (sampling/__init__.py:55), written on the device by a kernel that receives the times by value
            const int rc = launch_fill_times(m->d_ts, g.nfe_t.data(), (int)g.nfe_t.size(), B, s);
            if (rc != OK) return rc;
        }
        const size_t state = (size_t)2 * B * F * T;
        float* const xs = m->d_rk;                                   // stage input
        float* const acc = m->d_rk ? m->d_rk + state : nullptr;      // x + sum_j b_j h v_j so far
        const RkGrid::Eval& e = g.evals[k];
        const float* const t = m->d_ts + k * B;
        const float h = e.h;
        CallBlock cb{x, y, t, x, 2, h};                              // single-stage step: x += h v(x, t)
        auto stage = [&](const float* in, float* out, const float* acc_in, float* acc_out, float a, float b) {
            cb = CallBlock{in, y, t, out, 3, 0.f, x, acc_in, acc_out, a, b};
        };
        if (e.of == 2) {
            if (e.stage == 0) stage(x, xs, x, acc, h, 0.5f * h);
            else stage(xs, nullptr, acc, x, 0.f, 0.5f * h);
        } else if (e.of == 4) {
            if (e.stage == 0) stage(x, xs, x, acc, 0.5f * h, h / 6.0f);
            else if (e.stage == 1) stage(xs, xs, acc, acc, 0.5f * h, h / 3.0f);
            else if (e.stage == 2) stage(xs, xs, acc, acc, h, h / 3.0f);
            else stage(xs, nullptr, acc, x, 0.f, h / 6.0f);
        }
        ++k;
        const int rc = launch_set_call(m->d_call, cb, s);
        if (rc != OK) return rc;
        return may_graph ? exec_plan(m, p, s) : run_plan(m, p, s);
    }
};

static bool weights_shared(const flowse_model* m, const char* what) {
    if (!m->is_view && m->wt->holders == 1) return false;
    set_error("%s: the weight set is shared by %d handles; destroy the views first", what, m->wt->holders);
    return true;
}

// ------------------------------------------------------------------------- flowse_model_load_weights, table by table
// Each step derives one table of the set from the packed fp32 blob that is already in d_w (and from the packer's lists).
// The weight buffers grow without a synchronisation: the upload synchronises once, before the first of them.

// 16-bit storage modes: the elementwise 16-bit twin of the packed blob (conv weights keep their offsets) and, at the same
// offsets, the fragment-order copies for the producer / consumer 3x3 kernel and the 16-bit small-image kernel
static int upload_16bit_copies(WeightSet* w, Packer& pk) {
    const int64_t n = (int64_t)pk.host.size(), n16 = (n + 3) & ~(int64_t)3;
    if (const int rc = w->d_w16.reserve(n16, false)) return rc;
    if (const int rc = launch_convert(w->d_w, DT_F32, w->d_w16, w->act_dt, n & ~(int64_t)3, nullptr)) return rc;
    w->frag_offs.clear();
    if (const int rc = w->d_wfrag.reserve(n16, false)) return rc;
    for (auto& r : pk.wino) {
        if ((r.Cout % 128) != 0 || (int64_t)r.Cout * 9 * r.Cin * 2 >= (1LL << 31)) continue;
        if (const int rc = launch_pc16_weights(w->d_w16 + r.off, r.Cout, r.Cin, w->d_wfrag + r.off, nullptr)) return rc;
        w->frag_offs.insert(r.off);
    }
    // ... and for every other conv with 32-aligned channel counts (1x1 shortcuts, attention projections, 3x3 with
    // Cout % 128 != 0): the 16-bit small-image kernel reads the same layout
    if (conv16_smallm_ok(1, 4, 4, 32, 0, 32, 1)) {
        for (auto& r : pk.smallm) {
            if (w->frag_offs.count(r.off) || (int64_t)r.Cout * r.taps * r.Cin * 2 >= (1LL << 31)) continue;
            if (const int rc = launch_pc16_weights(w->d_w16 + r.off, r.Cout, r.Cin, w->d_wfrag + r.off, nullptr, r.taps)) return rc;
            w->frag_offs.insert(r.off);
        }
    }
    pk.wino.clear();                         // no fp32 Winograd kernels run on 16-bit activations
    return OK;
}

// F(4,3) Winograd weights, derived on the device
static int upload_f43_weights(WeightSet* w, const Packer& pk) {
    w->wino_of.clear();
    int64_t total = 0;
    for (auto& r : pk.wino) {
        w->wino_of[r.off] = total;
        total += (conv_wino_numel(r.Cout, r.Cin) + 63) & ~(int64_t)63;
    }
    if (const int rc = w->d_wino.reserve(total, false)) return rc;
    for (auto& r : pk.wino)
        if (const int rc = launch_f43_weights(w->d_w + r.off, r.Cout, r.Cin, w->d_wino + w->wino_of[r.off], nullptr)) return rc;
    return OK;
}

// fragment-order copies for the small-M kernels (fp32 activations only), at the same offsets as in d_w
static int upload_smallm_copies(WeightSet* w, const Packer& pk) {
    w->wsm_offs.clear();
    if (w->storage16() || pk.smallm.empty() || !conv_smallm_ok(1, 4, 4, 32, 0, 32, 1)) return OK;
    if (const int rc = w->d_wsm.reserve(pk.host.size(), false)) return rc;
    if (const int rc = w->d_wsm16.reserve(pk.host.size(), false)) return rc;
    for (auto& r : pk.smallm) {
        if ((int64_t)r.Cout * r.taps * r.Cin * 4 >= (1LL << 31)) continue;
        if (const int rc = launch_smallm_weights(w->d_w + r.off, r.Cout, r.taps, r.Cin, w->d_wsm + r.off, nullptr)) return rc;
        if (const int rc = launch_smallm_weights(w->d_w + r.off, r.Cout, r.taps, r.Cin, w->d_wsm16 + r.off, nullptr, true)) return rc;
        w->wsm_offs.insert(r.off);
    }
    return OK;
}

// F(4,3) x F(2,3) weights of the F(4,3) convs (the two-dimensional kernel takes the large images)
static int upload_w2d_weights(WeightSet* w, const Packer& pk) {
    w->wino2_of.clear();
    if (!conv_w2d_enabled()) return OK;
    int64_t total = 0;
    for (auto& r : pk.wino) {
        if ((int64_t)r.Cout * 24 * r.Cin * 4 >= (1LL << 31)) continue;
        w->wino2_of[r.off] = total;
        total += (conv_w2d_numel(r.Cout, r.Cin) + 63) & ~(int64_t)63;
    }
    if (const int rc = w->d_wino2.reserve(total, false)) return rc;
    for (auto& r : pk.wino) {
        const auto it = w->wino2_of.find(r.off);
        if (it == w->wino2_of.end()) continue;
        if (const int rc = launch_w2d_weights(w->d_w + r.off, r.Cout, r.Cin, w->d_wino2 + it->second, nullptr)) return rc;
    }
    return OK;
}

// optional bf16 planes for the 3x3 ResBlock convolutions the halo kernel can take, packed on the host from the caller's blob
static int upload_bf16_planes(WeightSet* w, const float* blob) {
    for (auto& mod : w->mods) mod.wq_c0 = mod.wq_c1 = -1;
    if (w->precision == 0 || w->storage16()) return OK;
    const int terms = w->precision == 1 ? 3 : 1;
    std::vector<uint16_t> q;
    auto plane = [&](int64_t param, int Cout, int Cin) {
        const int64_t off = (int64_t)q.size();
        q.resize(q.size() + conv_bf16_numel(Cout, Cin, terms));
        pack_conv_bf16(blob + w->params[param].offset, Cout, Cin, terms, q.data() + off, w->precision == 3);
        return off;
    };
    for (auto& mod : w->mods) {
        if (mod.kind != M_RESBLOCK || (mod.out_ch % 128) != 0) continue;
        if ((mod.in_ch % 32) == 0) mod.wq_c0 = plane(mod.p0 + 2, mod.out_ch, mod.in_ch);
        mod.wq_c1 = plane(mod.p0 + 8, mod.out_ch, mod.out_ch);
    }
    if (const int rc = w->d_wq.reserve(q.size(), false)) return rc;
    if (!q.empty()) FLOWSE_HIP(hipMemcpy(w->d_wq, q.data(), q.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return OK;
}

// ------------------------------------------------------------------------------------- shared by the per-op test entries
// the fields every conv entry fills
static ConvArgs conv_args(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                          const float* bias2, int bias2_stride, const float* res, float* out, int B, int H, int W, int Cout,
                          int taps, float scale) {
    ConvArgs c;
    c.in1 = in1; c.in2 = in2; c.C1 = C1; c.C2 = C2;
    c.w = w; c.bias = bias; c.bias2 = bias2; c.bias2_stride = bias2_stride; c.res = res; c.out = out;
    c.B = B; c.H = H; c.W = W; c.Cout = Cout; c.taps = taps; c.scale = scale;
    return c;
}

// Statistics and finalize of GroupNorm over cat[in1, in2], in `scratch` as flowse_op_group_norm_scratch_floats sizes it:
// partials [B][nblk][C][2], mean [B][C], scale [B][C].  *gn: what the consumer normalises with.
static int op_gn_prologue(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta, float eps,
                          int B, int HW, float* scratch, hipStream_t s, GnParams* gn) {
    const int C = C1 + C2, nblk = gn_partial_blocks(HW, C);
    float* mean = scratch + (int64_t)B * nblk * C * 2;
    float* scl = mean + (int64_t)B * C;
    *gn = GnParams{mean, scl, beta};
    const int rc = launch_gn_stats(in1, C1, in2, C2, B, HW, scratch, nblk, s);
    if (rc != OK) return rc;
    return launch_gn_finalize(scratch, nblk, C, nullptr, 0, 0, B, HW, std::min(C / 4, 32), gamma, eps, mean, scl, s);
}

// the caller's scratch of a 16-bit entry, handed out in sub-buffers rounded up to 256 bytes
struct Carver {
    char* p;
    static int64_t up(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
    void* take(int64_t bytes) {
        char* q = p;
        p += up(bytes);
        return q;
    }
};

}  // namespace flowse
// =============================================================================================== C ABI
extern "C" {

int flowse_abi_version(void) { return FLOWSE_ABI_VERSION; }

int flowse_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int flowse_model_create(const flowse_config* cfg, flowse_model** out) {
    if (!cfg || !out) {
        set_error("flowse_model_create: null argument");
        return ERR_ARG;
    }
    flowse_model* m = new flowse_model();
    m->wt = new WeightSet();
    m->cfg = *cfg;
    // hipGraph replay of the launch list is opt-in (FLOWSE_GRAPH=1): measured on MI355X / ROCm 7.2 a replayed graph of
    // ~400 short kernel nodes runs 5 % SLOWER than the same launches issued eagerly from the C loop at [1,1,256,256]
    // (8.09 k vs 8.55 k frames/s) and equal at [8,1,256,256]; the host is nowhere near launch-bound (~1.5 ms of launch
    // calls per 6 ms network evaluation at batch 1).
    m->use_graph = getenv("FLOWSE_GRAPH") != nullptr;
    const int rc = build_structure(m);
    if (rc != OK) {
        delete m->wt;
        delete m;
        return rc;
    }
    *out = m;
    return OK;
}

void flowse_model_destroy(flowse_model* m) {
    if (!m) return;
    free_device_state(m);
    if (--m->wt->holders == 0) delete m->wt;
    delete m;
}

int flowse_block_create(int kind, int in_ch, int out_ch, int up, int down, int temb_dim, flowse_model** out) {
    if (!out || kind < FLOWSE_BLOCK_RESNET || kind > FLOWSE_BLOCK_COMBINE || in_ch < 4 || (in_ch & 3) || out_ch < 4 ||
        (out_ch & 3) || (up && down) || (kind == FLOWSE_BLOCK_RESNET && temb_dim < 1) ||
        (kind == FLOWSE_BLOCK_ATTN && in_ch != out_ch) || (kind == FLOWSE_BLOCK_COMBINE && in_ch != 4)) {
        set_error("flowse_block_create: bad argument (kind=%d in_ch=%d out_ch=%d up=%d down=%d temb_dim=%d)", kind, in_ch,
                  out_ch, up, down, temb_dim);
        return ERR_ARG;
    }
    flowse_model* m = new flowse_model();
    m->wt = new WeightSet();
    memset(&m->cfg, 0, sizeof(m->cfg));
    m->use_graph = false;
    m->block_kind = kind;
    m->wt->temb_dim = temb_dim;
    if (kind == FLOWSE_BLOCK_RESNET) add_module(m, resblock_module(in_ch, out_ch, up != 0, down != 0));
    else add_module(m, simple_module(kind == FLOWSE_BLOCK_ATTN ? M_ATTN : M_COMBINE, in_ch, out_ch));
    *out = m;
    return OK;
}

int flowse_block_forward(flowse_model* m, const float* in1, int C1, const float* in2, const float* temb_act, float* out,
                         int B, int H, int W, void* stream) {
    if (!m || m->block_kind < 0 || !in1 || !out || (m->block_kind == FLOWSE_BLOCK_RESNET && !temb_act) ||
        (m->block_kind == FLOWSE_BLOCK_COMBINE && !in2)) {
        set_error("flowse_block_forward: bad argument (not a block handle, or a required pointer is null)");
        return ERR_ARG;
    }
    if (const int rc = check_ready(m)) return rc;
    if (!in2 && m->block_kind == FLOWSE_BLOCK_RESNET) C1 = m->wt->mods[0].in_ch;
    auto key = std::make_tuple(B, H, W, C1);
    auto it = m->block_plans.find(key);
    if (it == m->block_plans.end()) {
        Plan p;
        const int rc = build_block_plan(m, &p, B, H, W, C1);
        if (rc != OK) return rc;
        it = m->block_plans.emplace(key, std::move(p)).first;
    }
    Plan* p = &it->second;
    if (const int rc = reserve_workspace(m, p->ws_bytes)) return rc;
    m->bcall.in1 = in1;
    m->bcall.in2 = in2;
    m->bcall.temb_act = temb_act;
    m->bcall.out = out;
    return run_plan(m, p, static_cast<hipStream_t>(stream));
}

int flowse_model_num_params(const flowse_model* m) { return m ? (int)m->wt->params.size() : 0; }
int flowse_model_num_modules(const flowse_model* m) { return m ? (int)m->wt->mods.size() : 0; }
int64_t flowse_model_blob_numel(const flowse_model* m) { return m ? m->wt->blob_numel : 0; }

int flowse_model_param_info(const flowse_model* m, int index, char* name, int name_cap, int64_t shape[4], int* ndim,
                            int64_t* offset) {
    if (!m || index < 0 || index >= (int)m->wt->params.size()) {
        set_error("flowse_model_param_info: bad index %d", index);
        return ERR_ARG;
    }
    const ParamInfo& p = m->wt->params[index];
    if (name && name_cap > 0) {
        strncpy(name, p.name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (shape)
        for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
    if (ndim) *ndim = p.ndim;
    if (offset) *offset = p.offset;
    return OK;
}

int flowse_model_set_precision(flowse_model* m, int mode) {
    if (!m || mode < 0 || mode > 3) {
        set_error("flowse_model_set_precision: mode must be 0 (fp32), 1 (bf16x3), 2 (bf16) or 3 (fp16)");
        return ERR_ARG;
    }
    if (mode != m->wt->precision) {
        if (weights_shared(m, "flowse_model_set_precision")) return ERR_STATE;
        if (m->wt->d_w) {            // weights must be re-uploaded so that the operand planes match the mode
            if (const int rc = check_device(m)) return rc;      // before any state changes: a failure leaves the handle as is
            FLOWSE_HIP(hipDeviceSynchronize());
            clear_plans(m);
            m->wt->d_w.release();
            m->wt->d_w16.release();  // the 16-bit twin belongs to the mode that is being left
        }
        m->wt->precision = mode;
        m->wt->act_dt = DT_F32;      // recomputed by the next flowse_model_load_weights
        clear_plans(m);
    }
    return OK;
}

int flowse_model_load_weights(flowse_model* m, const float* blob, int64_t numel) {
    if (!m || !blob) {
        set_error("flowse_model_load_weights: null argument");
        return ERR_ARG;
    }
    if (numel != m->wt->blob_numel) {
        set_error("flowse_model_load_weights: blob has %lld floats, model needs %lld", (long long)numel,
                  (long long)m->wt->blob_numel);
        return ERR_ARG;
    }
    if (weights_shared(m, "flowse_model_load_weights")) return ERR_STATE;      // before the packer rewrites shared tables
    Packer pk;
    if (const int prc = pack_weights(m, blob, pk)) return prc;
    int dev = 0;
    FLOWSE_HIP(hipGetDevice(&dev));
    if (m->wt->device >= 0 && m->wt->device != dev) free_device_state(m);      // the handle moves to the current device
    m->wt->device = dev;
    FLOWSE_HIP(hipDeviceSynchronize());
    clear_plans(m);          // closures captured weight offsets of the previous packing
    WeightSet* w = m->wt;
    int rc = m->d_call.reserve(1, false);
    if (rc == OK) rc = w->d_w.reserve(pk.host.size(), false);
    if (rc != OK) return rc;
    FLOWSE_HIP(hipMemcpy(w->d_w, pk.host.data(), pk.host.size() * sizeof(float), hipMemcpyHostToDevice));
    w->act_dt = storage_type_for(m);
    if (w->storage16()) rc = upload_16bit_copies(w, pk);
    if (rc == OK) rc = upload_f43_weights(w, pk);
    if (rc == OK) rc = upload_smallm_copies(w, pk);
    if (rc == OK) rc = upload_w2d_weights(w, pk);
    if (rc != OK) return rc;
    FLOWSE_HIP(hipDeviceSynchronize());
    return upload_bf16_planes(w, blob);
}

int flowse_model_reserve(flowse_model* m, int B, int F, int T, int64_t* workspace_bytes) {
    if (!m) {
        set_error("flowse_model_reserve: null model");
        return ERR_ARG;
    }
    Plan* p = nullptr;
    const int rc = get_plan(m, B, F, T, &p);
    if (rc != OK) return rc;
    if (workspace_bytes) *workspace_bytes = (int64_t)p->ws_bytes;
    return OK;
}

int flowse_vf_forward(flowse_model* m, const void* x, const void* y, const float* t, void* out, int B, int F, int T,
                      int mode, void* stream) {
    if (!m || !x || !y || !t || !out || (mode != 0 && mode != 1)) {
        set_error("flowse_vf_forward: bad argument");
        return ERR_ARG;
    }
    Plan* p = nullptr;
    int rc = get_plan(m, B, F, T, &p);
    if (rc != OK) return rc;
    hipStream_t caller = static_cast<hipStream_t>(stream), s = nullptr;
    rc = enter_stream(m, caller, &s);
    if (rc != OK) return rc;
    CallBlock cb{static_cast<const float*>(x), static_cast<const float*>(y), t, static_cast<float*>(out), mode, 0.f};
    rc = launch_set_call(m->d_call, cb, s);
    if (rc == OK) rc = exec_plan(m, p, s);
    const int rc2 = leave_stream(m, caller, s);
    return rc != OK ? rc : rc2;
}

int flowse_prior_sample(const void* y, const void* z, float sigma, void* x_out, int64_t numel_complex, void* stream) {
    if (!y || !z || !x_out || numel_complex < 0) {
        set_error("flowse_prior_sample: bad argument");
        return ERR_ARG;
    }
    return launch_axpy(static_cast<const float*>(y), static_cast<const float*>(z), sigma, 2 * numel_complex,
                       static_cast<float*>(x_out), static_cast<hipStream_t>(stream));
}

int flowse_axpy(const void* x, const void* k, float dt, void* out, int64_t numel_complex, void* stream) {
    return flowse_prior_sample(x, k, dt, out, numel_complex, stream);
}

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

int flowse_euler_sample(flowse_model* m, void* x_inout, const void* y, const float* ts, const float* dts, int N, int B,
                        int F, int T, void* stream) {
    return flowse_rk_sample(m, x_inout, y, ts, dts, N, FLOWSE_TABLEAU_EULER, B, F, T, stream);
}

// Fixed-step explicit Runge-Kutta over the reference's grid (see include/flowse_hip.h).  With v = dnn(cat[x, y], t)
// (so VF = -v) and h = dts[i] > 0 a step from t to t - h is
//   euler:  x += h v(x, t)
//   heun:   v1 = v(x, t), v2 = v(x + h v1, t - h);                    x += h/2 (v1 + v2)
//   rk4:    v1 = v(x, t), v2 = v(x + h/2 v1, t - h/2), v3 = v(x + h/2 v2, t - h/2), v4 = v(x + h v3, t - h);
//           x += h/6 (v1 + 2 v2 + 2 v3 + v4)
// Every stage is one network evaluation whose head kernel (mode 3) writes the next stage's input and folds the slope
// into the accumulator; no separate axpy launches, no host synchronisation.
int flowse_rk_sample(flowse_model* m, void* x_inout, const void* y, const float* ts, const float* dts, int N, int tableau,
                     int B, int F, int T, void* stream) {
    if (!m || !x_inout || !y || !ts || !dts || N < 1 || tableau < FLOWSE_TABLEAU_EULER || tableau > FLOWSE_TABLEAU_RK4) {
        set_error("flowse_rk_sample / flowse_euler_sample: bad argument");
        return ERR_ARG;
    }
    RkRun run;
    run.m = m;
    run.x = static_cast<float*>(x_inout);
    run.y = static_cast<const float*>(y);
    run.B = B; run.F = F; run.T = T;
    int rc = get_plan(m, B, F, T, &run.p);
    if (rc != OK) return rc;
    const RkGrid grid(ts, dts, N, tableau);
    rc = reserve_rk(m, grid, B, F, T);
    if (rc != OK) return rc;
    hipStream_t caller = static_cast<hipStream_t>(stream), s = nullptr;
    rc = enter_stream(m, caller, &s);
    if (rc != OK) return rc;
    while (rc == OK && !run.done(grid)) rc = run.issue(grid, s, true);
    const int rc2 = leave_stream(m, caller, s);
    return rc != OK ? rc : rc2;
}

// Several fixed-step solves at once, one lane (stream) per distinct handle; see include/flowse_hip.h.  Each item issues
// exactly the launches flowse_rk_sample issues for it, in the same order on one stream, and no kernel of the library
// reads what another launch of another lane writes: the results are those of the single calls, bit for bit.
int flowse_rk_sample_multi(flowse_model* const* handles, int n_items, void* const* x_inout, const void* const* y,
                           const int* B, const int* T, int F, const float* ts, const float* dts, int N, int tableau,
                           void* stream) {
    if (!handles || n_items < 1 || !x_inout || !y || !B || !T || !ts || !dts || N < 1 ||
        tableau < FLOWSE_TABLEAU_EULER || tableau > FLOWSE_TABLEAU_RK4) {
        set_error("flowse_rk_sample_multi: bad argument (null table, n_items < 1, N < 1 or unknown tableau)");
        return ERR_ARG;
    }
    struct Lane { flowse_model* m; std::vector<RkRun> runs; size_t cur = 0; };
    std::vector<Lane> lanes;
    for (int i = 0; i < n_items; ++i) {
        if (!handles[i] || !x_inout[i] || !y[i] || handles[i]->block_kind >= 0) {
            set_error("flowse_rk_sample_multi: item %d has a null pointer or a single-module handle", i);
            return ERR_ARG;
        }
        size_t l = 0;
        while (l < lanes.size() && lanes[l].m != handles[i]) ++l;
        if (l == lanes.size()) {
            if (l == FLOWSE_MAX_LANES) {
                set_error("flowse_rk_sample_multi: more than %d distinct handles (one lane, i.e. one stream, per handle; a "
                          "process has 4 hardware queues by default)", FLOWSE_MAX_LANES);
                return ERR_ARG;
            }
            Lane ln;
            ln.m = handles[i];
            lanes.push_back(ln);
        }
        RkRun run;
        run.m = handles[i];
        run.x = static_cast<float*>(x_inout[i]);
        run.y = static_cast<const float*>(y[i]);
        run.B = B[i]; run.F = F; run.T = T[i];
        lanes[l].runs.push_back(run);
    }
    for (auto& ln : lanes)
        if (ln.m->prof_mode != -1) {
            set_error("flowse_rk_sample_multi: a handle has a profile open (flowse_profile_end first)");
            return ERR_STATE;
        }
    if (n_items == 1) return flowse_rk_sample(handles[0], x_inout[0], y[0], ts, dts, N, tableau, B[0], F, T[0], stream);
    // Everything that can allocate (and therefore synchronise the device or free a buffer) comes before the first launch:
    // plans, then per lane the workspace, time table and RK scratch of its largest item, then streams and events.
    const RkGrid grid(ts, dts, N, tableau);
    for (auto& ln : lanes) {
        for (auto& run : ln.runs) {
            const int rc = get_plan(ln.m, run.B, run.F, run.T, &run.p);
            if (rc != OK) return rc;
        }
        for (auto& run : ln.runs) {
            const int rc = reserve_rk(ln.m, grid, run.B, run.F, run.T);
            if (rc != OK) return rc;
        }
        const int rc = ensure_stream(ln.m);
        if (rc != OK) return rc;
    }
    hipStream_t caller = static_cast<hipStream_t>(stream);
    FLOWSE_HIP(hipEventRecord(lanes[0].m->ev_in, caller));
    for (size_t l = 1; l < lanes.size(); ++l) FLOWSE_HIP(hipStreamWaitEvent(lanes[l].m->gstream, lanes[0].m->ev_in, 0));
    // round-robin, one network evaluation per lane and turn: every lane has work queued within the first evaluation's
    // enqueue time.  Plain launches only (a captured graph with parallel branches is what this path must not make).
    int rc = OK;
    for (bool busy = true; busy && rc == OK;) {
        busy = false;
        for (size_t l = 0; l < lanes.size() && rc == OK; ++l) {
            Lane& ln = lanes[l];
            while (ln.cur < ln.runs.size() && ln.runs[ln.cur].done(grid)) ++ln.cur;
            if (ln.cur == ln.runs.size()) continue;
            rc = ln.runs[ln.cur].issue(grid, l == 0 ? caller : ln.m->gstream, false);
            busy = true;
        }
    }
    // join every lane into the caller's stream, also after a failed launch (what was enqueued still runs)
    for (size_t l = 1; l < lanes.size(); ++l) {
        const hipError_t e1 = hipEventRecord(lanes[l].m->ev_out, lanes[l].m->gstream);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(caller, lanes[l].m->ev_out, 0) : e1;
        if (e2 != hipSuccess && rc == OK) {
            set_error("flowse_rk_sample_multi: joining lane %zu failed: %s", l, hipGetErrorString(e2));
            rc = ERR_HIP;
        }
    }
    return rc;
}

int flowse_model_view_create(flowse_model* parent, flowse_model** out) {
    if (!parent || !out) {
        set_error("flowse_model_view_create: null argument");
        return ERR_ARG;
    }
    if (parent->block_kind >= 0) {
        set_error("flowse_model_view_create: the parent is a single-module handle (flowse_block_create)");
        return ERR_ARG;
    }
    if (!parent->wt->d_w) {
        set_error("flowse_model_view_create: the parent has no weights loaded (flowse_model_load_weights first)");
        return ERR_STATE;
    }
    if (const int rc = check_device(parent)) return rc;
    flowse_model* v = new flowse_model();
    if (const int rc = v->d_call.reserve(1, false)) {
        delete v;
        return rc;
    }
    v->cfg = parent->cfg;
    v->wt = parent->wt;
    v->is_view = true;
    v->use_graph = parent->use_graph;
    ++v->wt->holders;
    *out = v;
    return OK;
}

int64_t flowse_model_device_bytes(const flowse_model* m, int what) {
    if (!m || (what != FLOWSE_BYTES_WEIGHTS && what != FLOWSE_BYTES_OWNED)) return 0;
    int64_t total = 0;
    auto add = [&](const auto& b) { total += (int64_t)b.bytes(); };
    if (what == FLOWSE_BYTES_OWNED) each_owned_buffer(m, add);
    else each_weight_buffer(m->wt, add);
    return total;
}

int flowse_model_weight_holders(const flowse_model* m) { return (m && m->wt->d_w) ? m->wt->holders : 0; }

int64_t flowse_model_graph_launches(const flowse_model* m) { return m ? m->graph_launches : 0; }

int flowse_stft_compress(const float* sig, int B, int L, float scale_in, void* out_c64, int T, int Tpad, float factor,
                         float exponent, void* stream) {
    if (!sig || !out_c64) {
        set_error("flowse_stft_compress: null argument");
        return ERR_ARG;
    }
    return launch_stft_compress(sig, B, L, scale_in, static_cast<float*>(out_c64), T, Tpad, factor, exponent,
                                static_cast<hipStream_t>(stream));
}

int flowse_istft_decompress(const void* spec_c64, int B, int T, int Tpad, float factor, float exponent, float* out,
                            int Lout, float scale_out, void* stream) {
    if (!spec_c64 || !out) {
        set_error("flowse_istft_decompress: null argument");
        return ERR_ARG;
    }
    return launch_istft_decompress(static_cast<const float*>(spec_c64), B, T, Tpad, factor, exponent, out, Lout,
                                   scale_out, static_cast<hipStream_t>(stream));
}

int flowse_stft_compress_chunks(const float* sig, int L, float scale_in, void* out_c64, int K, int Tc, int hop, float factor,
                                float exponent, void* stream) {
    if (!sig || !out_c64) {
        set_error("flowse_stft_compress_chunks: null argument");
        return ERR_ARG;
    }
    return launch_stft_compress_chunks(sig, L, scale_in, static_cast<float*>(out_c64), K, Tc, hop, factor, exponent,
                                       static_cast<hipStream_t>(stream));
}

int flowse_istft_decompress_chunks(const void* chunks_c64, int K, int Tc, int hop, float factor, float exponent, float* out,
                                   int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_chunks: null argument");
        return ERR_ARG;
    }
    return launch_istft_decompress_chunks(static_cast<const float*>(chunks_c64), K, Tc, hop, factor, exponent, out, Lout,
                                          scale_out, static_cast<hipStream_t>(stream));
}

int flowse_stft_compress_rows(const flowse_spec_row* rows, int R, int Tw, void* out_c64, float factor, float exponent,
                              void* stream) {
    if (!rows || !out_c64) {
        set_error("flowse_stft_compress_rows: null argument");
        return ERR_ARG;
    }
    return launch_stft_compress_rows(rows, R, Tw, static_cast<float*>(out_c64), factor, exponent,
                                     static_cast<hipStream_t>(stream));
}

int flowse_istft_decompress_stacks(const void* chunks_c64, int S, int K, int Tc, int hop, float factor, float exponent,
                                   float* out, int Lout, float scale_out, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_stacks: null argument");
        return ERR_ARG;
    }
    return launch_istft_decompress_stacks(static_cast<const float*>(chunks_c64), S, K, Tc, hop, factor, exponent, out, Lout,
                                          scale_out, static_cast<hipStream_t>(stream));
}

int flowse_istft_decompress_ensemble(const void* chunks_c64, int S, int D, int K, int Tc, int hop, int64_t stack_stride,
                                     int64_t draw_stride, float factor, float exponent, float* out, int Lout,
                                     float scale_out, float* tracks, void* stream) {
    if (!chunks_c64 || !out) {
        set_error("flowse_istft_decompress_ensemble: null argument");
        return ERR_ARG;
    }
    return launch_istft_decompress_ensemble(static_cast<const float*>(chunks_c64), S, D, K, Tc, hop, stack_stride,
                                            draw_stride, factor, exponent, out, Lout, scale_out, tracks,
                                            static_cast<hipStream_t>(stream));
}

int flowse_stft_compress_window(const float* buf, int64_t s0, int64_t n, float scale_in, int64_t frame0, int Tc,
                                int64_t L_total, void* out_c64, float factor, float exponent, void* stream) {
    if (!buf || !out_c64) {
        set_error("flowse_stft_compress_window: null argument");
        return ERR_ARG;
    }
    return launch_stft_compress_window(buf, s0, n, scale_in, frame0, Tc, L_total, static_cast<float*>(out_c64), factor,
                                       exponent, static_cast<hipStream_t>(stream));
}

int flowse_istft_decompress_window(const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k, int Tc,
                                   int hop, int last, int64_t L, float factor, float exponent, float* out, int64_t e0,
                                   int64_t n_out, float scale_out, void* stream) {
    if (!cur_c64 || !out) {
        set_error("flowse_istft_decompress_window: null argument");
        return ERR_ARG;
    }
    return launch_istft_decompress_window(static_cast<const float*>(prev2_c64), static_cast<const float*>(prev_c64),
                                          static_cast<const float*>(cur_c64), k, Tc, hop, last, L, factor, exponent, out,
                                          e0, n_out, scale_out, static_cast<hipStream_t>(stream));
}

int flowse_profile_begin(flowse_model* m, int mode) {
    if (!m || (mode != 0 && mode != 1)) {
        set_error("flowse_profile_begin: bad argument");
        return ERR_ARG;
    }
    m->prof_mode = mode;
    m->prof_used = 0;
    m->prof_pending.clear();
    m->prof_labels.clear();
    m->prof_label_ix.clear();
    m->prof_tot_flops = m->prof_tot_issued = 0.0;
    m->prof_tot_launches = 0;
    return OK;
}

int flowse_profile_end(flowse_model* m, char* json, int cap) {
    if (!m || !json || cap < 64) {
        set_error("flowse_profile_end: bad argument");
        return ERR_ARG;
    }
    m->prof_mode = -1;
    std::vector<ProfAcc> acc(m->prof_labels.size());
    for (auto& pd : m->prof_pending) {
        FLOWSE_HIP(hipEventSynchronize(pd.b));
        float ms = 0.f;
        FLOWSE_HIP(hipEventElapsedTime(&ms, pd.a, pd.b));
        ProfAcc& a = acc[pd.label];
        a.launches += 1;
        a.ms += ms;
        a.flops += pd.flops;
        a.bytes += pd.bytes;
        a.issued += pd.issued;
    }
    m->prof_pending.clear();
    m->prof_used = 0;
    std::string out = "{";
    for (size_t i = 0; i < acc.size(); ++i) {
        char buf[384];
        snprintf(buf, sizeof(buf),
                 "%s\"%s\": {\"launches\": %lld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e, \"issued\": %.6e}",
                 i ? ", " : "", m->prof_labels[i].c_str(), (long long)acc[i].launches, acc[i].ms, acc[i].flops,
                 acc[i].bytes, acc[i].issued);
        out += buf;
    }
    {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s\"_all_launches\": {\"launches\": %lld, \"ms\": 0, \"flops\": %.6e, \"bytes\": 0, "
                 "\"issued\": %.6e}", acc.empty() ? "" : ", ", (long long)m->prof_tot_launches, m->prof_tot_flops,
                 m->prof_tot_issued);
        out += buf;
    }
    out += "}";
    if ((int)out.size() + 1 > cap) {
        set_error("flowse_profile_end: report needs %zu bytes", out.size() + 1);
        return ERR_ARG;
    }
    memcpy(json, out.c_str(), out.size() + 1);
    return OK;
}

int flowse_upfirdn2d(const float* input, const float* kernel, int planes, int in_h, int in_w, int kh, int kw, int up_x,
                     int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, float* out,
                     int out_h, int out_w, void* stream) {
    if (!input || !kernel || !out || pad_x0 < 0 || pad_x1 < 0 || pad_y0 < 0 || pad_y1 < 0) {
        set_error("flowse_upfirdn2d: bad argument (null pointer or negative pad)");
        return ERR_ARG;
    }
    return launch_upfirdn2d_nchw(input, kernel, planes, in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1,
                                 pad_y0, pad_y1, out, out_h, out_w, static_cast<hipStream_t>(stream));
}

// The route of an fp32 conv for a per-op entry whose scratch can hold what `o` names (a view of conv_route)
static ConvRoute op_route_f32(int B, int H, int W, int C1, int C2, int Cout, int taps, ConvOffer o) {
    return conv_route(ConvShape{DT_F32, DT_F32, B, H, W, C1, C2, Cout, taps}, o);
}
static ConvOffer op_offer_scratch() {            // flowse_op_conv2d's scratch: the fragment-order weight copy, or the slab
    ConvOffer o;
    o.wsm = o.slab = true;
    return o;
}
static ConvOffer op_offer_f43() {                // flowse_op_conv3x3_f43's scratch: the F(4,3) weights and the slab
    ConvOffer o;
    o.wino = o.slab = true;
    return o;
}

int64_t flowse_op_conv2d_scratch_floats(int B, int H, int W, int Cin, int Cout, int taps) {
    const ConvRoute r = op_route_f32(B, H, W, Cin, 0, Cout, taps, op_offer_scratch());
    if (r.kernel == CK_SMALLM || r.kernel == CK_1X1_STREAM) return (int64_t)Cout * taps * Cin;   // fragment-order weight copy
    return r.ksplit > 1 ? (int64_t)r.ksplit * B * H * W * Cout : 0;
}

int flowse_op_conv2d(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                     const float* bias2, int bias2_stride, const float* res, float* out, int B, int H, int W, int Cout,
                     int taps, float scale, float* splitk_scratch, void* stream) {
    if (!in1 || !w || !out) {
        set_error("flowse_op_conv2d: null argument");
        return ERR_ARG;
    }
    ConvArgs c = conv_args(in1, C1, in2, in2 ? C2 : 0, w, bias, bias2, bias2_stride, res, out, B, H, W, Cout, taps, scale);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (C1 == 4 && !in2) return launch_conv_cin4(c, s);
    if (splitk_scratch) {                            // the model handle's kernel for this shape
        const ConvRoute r = op_route_f32(B, H, W, c.C1, c.C2, Cout, taps, op_offer_scratch());
        if (r.kernel == CK_SMALLM || r.kernel == CK_1X1_STREAM) {
            const bool t16 = r.kernel == CK_SMALLM && conv_smallm_tile16(B, H, W);
            const int rc = launch_smallm_weights(w, Cout, taps, c.C1 + c.C2, splitk_scratch, s, t16);
            if (rc != OK) return rc;
            c.wsm = splitk_scratch;
            c.wsm16 = t16 ? splitk_scratch : nullptr;
        } else {
            c.ksplit = r.ksplit;
            c.partial = c.ksplit > 1 ? splitk_scratch : nullptr;
        }
    }
    return launch_conv(c, s);
}

int64_t flowse_op_group_norm_scratch_floats(int B, int HW, int C) {
    const int nblk = gn_partial_blocks(HW, C);
    return (int64_t)B * nblk * C * 2 + 2 * (int64_t)B * C;
}

int flowse_op_group_norm(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                         float eps, int silu, float* out, int B, int H, int W, float* scratch, void* stream) {
    if (!in1 || !gamma || !beta || !out || !scratch) {
        set_error("flowse_op_group_norm: null argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!in2) C2 = 0;
    GnParams p;
    const int rc = op_gn_prologue(in1, C1, in2, C2, gamma, beta, eps, B, H * W, scratch, s, &p);
    if (rc != OK) return rc;
    return launch_gn_apply(in1, C1, in2, C2, B, H * W, p, silu, out, s);
}

int flowse_op_conv3x3_gn(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                         float eps, int silu, const float* w, const float* bias, const float* bias2, int bias2_stride,
                         const float* res, float* out, int B, int H, int W, int Cout, float scale, float* scratch,
                         void* stream) {
    if (!in1 || !gamma || !beta || !w || !out || !scratch) {
        set_error("flowse_op_conv3x3_gn: null argument");
        return ERR_ARG;
    }
    if (!in2) C2 = 0;
    if (!op_route_f32(B, H, W, C1, C2, Cout, 9, ConvOffer()).gn_on_load) {
        set_error("flowse_op_conv3x3_gn: shape B=%d H=%d W=%d C=%d+%d Cout=%d not covered by the halo kernel", B, H, W,
                  C1, C2, Cout);
        return ERR_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    ConvArgs c = conv_args(in1, C1, in2, C2, w, bias, bias2, bias2_stride, res, out, B, H, W, Cout, 9, scale);
    c.gn_silu = silu;
    const int rc = op_gn_prologue(in1, C1, in2, C2, gamma, beta, eps, B, H * W, scratch, s, &c.gn);
    return rc != OK ? rc : launch_conv(c, s);
}

static int op_conv3x3_winograd(const float* in1, int C1, const float* in2, int C2, const float* gamma,
                               const float* beta, float eps, int silu, const float* w, const float* bias,
                               const float* bias2, int bias2_stride, const float* res, float* out, int B, int H, int W,
                               int Cout, float scale, float* scratch, void* stream, bool two_d = false) {
    if (!in1 || !w || !out || !scratch || (gamma && !beta)) {
        set_error("flowse_op_conv3x3_f43: null argument");
        return ERR_ARG;
    }
    if (!in2) C2 = 0;
    const ConvRoute r = op_route_f32(B, H, W, C1, C2, Cout, 9, op_offer_f43());
    if (two_d ? !conv_w2d_shape_ok(B, H, W, C1, C2, Cout, 9) : (r.kernel != CK_F43 && r.kernel != CK_F43_SPLITK)) {
        set_error("flowse_op_conv3x3_%s: shape B=%d H=%d W=%d C=%d+%d Cout=%d not covered by the Winograd kernel",
                  two_d ? "w2d" : "f43", B, H, W, C1, C2, Cout);
        return ERR_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = C1 + C2, HW = H * W;
    float* wf = scratch + flowse_op_group_norm_scratch_floats(B, HW, C);
    int rc = two_d ? launch_w2d_weights(w, Cout, C, wf, s) : launch_f43_weights(w, Cout, C, wf, s);
    if (rc != OK) return rc;
    ConvArgs c = conv_args(in1, C1, in2, C2, w, bias, bias2, bias2_stride, res, out, B, H, W, Cout, 9, scale);
    if (two_d) c.wino2 = wf;
    else c.wino = wf;
    const int ks = two_d ? 1 : r.ksplit;
    if (ks > 1) {                           // same split plan as the model handle uses for this shape
        c.ksplit = ks;
        c.partial = wf + conv_wino_numel(Cout, C);
    }
    if (gamma) {
        c.gn_silu = silu;
        rc = op_gn_prologue(in1, C1, in2, C2, gamma, beta, eps, B, HW, scratch, s, &c.gn);
        if (rc != OK) return rc;
    }
    // the 2-D entry names its kernel: every shape conv_w2d_shape_ok admits runs it (launch_conv's policy would hand images of
    // up to 2048 pixels to another kernel, or refuse their fused GroupNorm input)
    return two_d ? launch_w2d(c, s) : launch_conv(c, s);
}

int64_t flowse_op_conv3x3_f43_scratch_floats(int B, int H, int W, int C, int Cout) {
    const int ks = op_route_f32(B, H, W, C, 0, Cout, 9, op_offer_f43()).ksplit;   // > 1: F(4,3) runs split over K (small images)
    return flowse_op_group_norm_scratch_floats(B, H * W, C) + conv_wino_numel(Cout, C) +
           (ks > 1 ? (int64_t)ks * B * H * W * Cout : 0);
}

int64_t flowse_op_conv3x3_w2d_scratch_floats(int B, int H, int W, int C, int Cout) {
    return flowse_op_group_norm_scratch_floats(B, H * W, C) + conv_w2d_numel(Cout, C);
}

int flowse_op_conv3x3_w2d(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                          float eps, int silu, const float* w, const float* bias, const float* bias2, int bias2_stride,
                          const float* res, float* out, int B, int H, int W, int Cout, float scale, float* scratch,
                          void* stream) {
    return op_conv3x3_winograd(in1, C1, in2, C2, gamma, beta, eps, silu, w, bias, bias2, bias2_stride, res, out, B, H,
                               W, Cout, scale, scratch, stream, true);
}

int flowse_op_conv3x3_f43(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                          float eps, int silu, const float* w, const float* bias, const float* bias2, int bias2_stride,
                          const float* res, float* out, int B, int H, int W, int Cout, float scale, float* scratch,
                          void* stream) {
    return op_conv3x3_winograd(in1, C1, in2, C2, gamma, beta, eps, silu, w, bias, bias2, bias2_stride, res, out, B, H,
                               W, Cout, scale, scratch, stream);
}

// 16-bit storage per-op entry: fp32 NHWC tensors at the boundary, rounded to bf16 (dt 1) / half (dt 2) inside, conv on
// the 16-bit matrix cores (LDS-halo kernel when it applies, else the flat kernel), result widened back.  Optional fused
// GroupNorm(+SiLU) on the input (halo shapes only) from caller-supplied per-(sample, channel) mean / scale and beta.
// (bias2 / out_f32: the additions of flowse_op_conv2d_16_ex; out_f32 = `res` and `out` are fp32 tensors the conv reads and
// writes directly, out_dt = DT_F32, as the model does for the few convs that leave the 16-bit domain)
static int op_conv2d_16(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                        const float* bias2, int bias2_stride, const float* res, const float* gn_mean, const float* gn_scale,
                        const float* gn_beta, int silu, float* out, int out_f32, int B, int H, int W, int Cout, int taps,
                        float scale, int dt, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!in1 || !w || !out || !scratch || (dt != DT_BF16 && dt != DT_F16) || (taps != 1 && taps != 9)) {
        set_error("flowse_op_conv2d_16: bad argument");
        return ERR_ARG;
    }
    if (!in2) C2 = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t M = (int64_t)B * H * W, C = C1 + C2;
    // the progressive-output heads (C -> 4, ncsnpp.py:345-366): 16-bit input, fp32 residual (the pyramid) and fp32 output, as
    // in the model -- conv3x3_head4_16_kernel
    const bool head = Cout == 4 && taps == 9 && !in2 && conv_supports_head4(B, H, W, C1, 0, Cout, taps);
    const bool direct = head || out_f32;                   // fp32 res / out, used in place
    // (the LDS-halo kernels store the operands' type only: an fp32-output launch of their shapes runs the flat kernel)
    ConvOffer offer;                                       // the scratch holds the 16-bit weights, their fragment-order copy, the slab
    offer.wq = offer.wfrag = offer.slab = true;
    offer.terms = 1;
    offer.wq_f16 = dt == DT_F16;
    offer.bias2 = bias2 != nullptr;
    const ConvRoute r = conv_route(ConvShape{dt, direct ? DT_F32 : dt, B, H, W, C1, C2, Cout, taps}, offer);
    const int ks = r.ksplit;
    const int64_t nw = ((int64_t)Cout * taps * C + 3) & ~(int64_t)3;
    // the carver's round-up per sub-buffer, upper bound over the optional ones
    const auto up = Carver::up;
    const int64_t need = up(2 * M * C1) + up(2 * M * C2) + 2 * up(2 * nw) + 2 * up(2 * M * Cout) +
                         (ks > 1 ? up(4 * (int64_t)ks * M * Cout) : 0);
    if (scratch_bytes < need) {
        set_error("flowse_op_conv2d_16: scratch needs %lld bytes", (long long)need);
        return ERR_ARG;
    }
    if (gn_mean && !r.gn_on_load) {
        set_error("flowse_op_conv2d_16: fused GroupNorm input only on LDS-halo shapes");
        return ERR_SHAPE;
    }
    Carver cv{static_cast<char*>(scratch)};
    void* a1 = cv.take(2 * M * C1);
    void* a2 = C2 ? cv.take(2 * M * C2) : nullptr;
    void* wq = cv.take(2 * nw);
    const bool frag = (taps == 9 && conv16_uses_pc(B, H, W, C1, C2, Cout, taps)) || conv16_smallm_ok(B, H, W, C1, C2, Cout, taps);
    void* wfrag = frag ? cv.take(2 * nw) : nullptr;
    void* r16 = res && !direct ? cv.take(2 * M * Cout) : nullptr;
    void* o16 = direct ? nullptr : cv.take(2 * M * Cout);
    float* part = ks > 1 ? static_cast<float*>(cv.take(4 * (int64_t)ks * M * Cout)) : nullptr;
    if ((size_t)(cv.p - static_cast<char*>(scratch)) > (size_t)scratch_bytes) {
        set_error("flowse_op_conv2d_16: scratch too small");
        return ERR_ARG;
    }
    int rc = launch_convert(in1, DT_F32, a1, dt, M * C1, s);
    if (rc == OK && C2) rc = launch_convert(in2, DT_F32, a2, dt, M * C2, s);
    if (rc == OK) rc = launch_convert(w, DT_F32, wq, dt, nw, s);
    if (rc == OK && frag) rc = launch_pc16_weights(wq, Cout, (int)C, wfrag, s, taps);
    if (rc == OK && r16) rc = launch_convert(res, DT_F32, r16, dt, M * Cout, s);
    if (rc != OK) return rc;
    ConvArgs c = conv_args(static_cast<const float*>(a1), C1, static_cast<const float*>(a2), C2, w, bias, bias2,
                           bias2 ? bias2_stride : 0, static_cast<const float*>(r16), static_cast<float*>(o16), B, H, W, Cout,
                           taps, scale);
    c.ksplit = ks; c.partial = part;
    c.wq = wq; c.terms = 1; c.wq_f16 = dt == DT_F16 ? 1 : 0;
    c.wfrag = wfrag;
    c.in_dt = dt; c.out_dt = dt;
    if (gn_mean) {
        c.gn = GnParams{gn_mean, gn_scale, gn_beta};
        c.gn_silu = silu;
    }
    if (direct) {
        c.res = res;
        c.out = out;
        c.out_dt = DT_F32;
    }
    rc = launch_conv(c, s);
    if (rc != OK || direct) return rc;
    return launch_convert(o16, dt, out, DT_F32, M * Cout, s);
}

int flowse_op_conv2d_16(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                        const float* res, const float* gn_mean, const float* gn_scale, const float* gn_beta, int silu,
                        float* out, int B, int H, int W, int Cout, int taps, float scale, int dt, void* scratch,
                        int64_t scratch_bytes, void* stream) {
    return op_conv2d_16(in1, C1, in2, C2, w, bias, nullptr, 0, res, gn_mean, gn_scale, gn_beta, silu, out, 0, B, H, W, Cout,
                        taps, scale, dt, scratch, scratch_bytes, stream);
}

int flowse_op_conv2d_16_ex(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                           const float* bias2, int bias2_stride, const float* res, const float* gn_mean,
                           const float* gn_scale, const float* gn_beta, int silu, float* out, int out_f32, int B, int H,
                           int W, int Cout, int taps, float scale, int dt, void* scratch, int64_t scratch_bytes,
                           void* stream) {
    if (bias2 && (bias2_stride < Cout || (bias2_stride & 3))) {
        set_error("flowse_op_conv2d_16_ex: bias2_stride must be a multiple of 4 and at least Cout");
        return ERR_ARG;
    }
    return op_conv2d_16(in1, C1, in2, C2, w, bias, bias2, bias2_stride, res, gn_mean, gn_scale, gn_beta, silu, out,
                        out_f32 != 0, B, H, W, Cout, taps, scale, dt, scratch, scratch_bytes, stream);
}

const char* flowse_op_last_conv_route(void) { return conv_last_route(); }

int flowse_op_conv_route(int in_dt, int out_dt, int B, int H, int W, int C1, int C2, int Cout, int taps, int offer_bits,
                         char* text, int cap) {
    if (!text || cap < 64 || in_dt < DT_F32 || in_dt > DT_F16 || (out_dt != DT_F32 && out_dt != in_dt) || B < 1 || H < 1 || W < 1) {
        set_error("flowse_op_conv_route: bad argument");
        return ERR_ARG;
    }
    const ConvShape q{in_dt, out_dt, B, H, W, C1, C2, Cout, taps};
    ConvOffer o;
    o.wino = offer_bits & FLOWSE_OFFER_WINO; o.wino2 = offer_bits & FLOWSE_OFFER_WINO2; o.wsm = offer_bits & FLOWSE_OFFER_WSM;
    o.wfrag = offer_bits & FLOWSE_OFFER_WFRAG; o.wq = offer_bits & FLOWSE_OFFER_WQ;
    o.terms = !o.wq ? 0 : (offer_bits & FLOWSE_OFFER_WQ_SPLIT3) ? 3 : 1;
    o.wq_f16 = offer_bits & FLOWSE_OFFER_WQ_F16;
    o.slab = offer_bits & FLOWSE_OFFER_SLAB; o.gn = offer_bits & FLOWSE_OFFER_GN; o.bias2 = offer_bits & FLOWSE_OFFER_BIAS2;
    o.stats = offer_bits & FLOWSE_OFFER_STATS; o.fold = offer_bits & FLOWSE_OFFER_FOLD;
    int err = conv_shape_check(q);
    ConvRoute r;
    if (err == OK) {
        r = conv_route(q, o);
        if ((err = r.err) != OK) set_error("%s", r.err_text);
    }
    if (err != OK) {
        snprintf(text, cap, "error %d", err);
        return OK;
    }
    const char* issued = r.issued == 0.5 ? "1/2" : r.issued == 3.0 ? "3" : r.issued == 1.0 ? "1" : "1/3";
    snprintf(text, cap, "%s ks=%d reduce=%d stats=%d gn=%d issued=%s", conv_kernel_name(r.kernel), r.ksplit, r.reduce ? 1 : 0,
             r.stats_nblk, r.gn_on_load ? 1 : 0, issued);
    return OK;
}

// Tail of ResnetBlockBigGANpp in 16-bit storage as ONE launch of the producer / consumer kernel:
//   out = (conv3x3(act(GroupNorm(h)); w1) + b1 + conv1x1(cat[x1, x2]; w2) + b2) * scale       (layerspp.py:265-274)
// with the shortcut as extra K steps (ConvArgs::sc1).  fp32 tensors at the boundary as in flowse_op_conv2d_16.
int flowse_op_resblock_tail_16(const float* h, int C, const float* gn_mean, const float* gn_scale, const float* gn_beta,
                               int silu, const float* w1, const float* b1, const float* x1, int XC1, const float* x2,
                               int XC2, const float* w2, const float* b2, float* out, int B, int H, int W, int Cout,
                               float scale, int dt, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!h || !w1 || !x1 || !w2 || !out || !scratch || (dt != DT_BF16 && dt != DT_F16)) {
        set_error("flowse_op_resblock_tail_16: bad argument");
        return ERR_ARG;
    }
    if (!x2) XC2 = 0;
    if (!conv16_uses_pc(B, H, W, C, 0, Cout, 9)) {
        set_error("flowse_op_resblock_tail_16: only shapes conv3x3_pc16_kernel takes (H, W multiples of 16, C %% 32 == 0, "
                  "Cout %% 128 == 0, >= 64 tile x channel-block items)");
        return ERR_SHAPE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t M = (int64_t)B * H * W, XC = (int64_t)XC1 + XC2;
    const int64_t nw1 = ((int64_t)Cout * 9 * C + 3) & ~(int64_t)3, nw2 = ((int64_t)Cout * XC + 3) & ~(int64_t)3;
    const auto up = Carver::up;
    const int64_t need = up(2 * M * C) + up(2 * M * XC1) + up(2 * M * XC2) + 2 * up(2 * nw1) + 2 * up(2 * nw2) + up(2 * M * Cout);
    if (scratch_bytes < need) {
        set_error("flowse_op_resblock_tail_16: scratch needs %lld bytes", (long long)need);
        return ERR_ARG;
    }
    Carver cv{static_cast<char*>(scratch)};
    void* h16 = cv.take(2 * M * C);
    void* a1 = cv.take(2 * M * XC1);
    void* a2 = XC2 ? cv.take(2 * M * XC2) : nullptr;
    void* wq1 = cv.take(2 * nw1);
    void* wf1 = cv.take(2 * nw1);
    void* wq2 = cv.take(2 * nw2);
    void* wf2 = cv.take(2 * nw2);
    void* o16 = cv.take(2 * M * Cout);
    int rc = launch_convert(h, DT_F32, h16, dt, M * C, s);
    if (rc == OK) rc = launch_convert(x1, DT_F32, a1, dt, M * XC1, s);
    if (rc == OK && XC2) rc = launch_convert(x2, DT_F32, a2, dt, M * XC2, s);
    if (rc == OK) rc = launch_convert(w1, DT_F32, wq1, dt, nw1, s);
    if (rc == OK) rc = launch_convert(w2, DT_F32, wq2, dt, nw2, s);
    if (rc == OK) rc = launch_pc16_weights(wq1, Cout, C, wf1, s, 9);
    if (rc == OK) rc = launch_pc16_weights(wq2, Cout, (int)XC, wf2, s, 1);
    if (rc != OK) return rc;
    ConvArgs c = conv_args(static_cast<const float*>(h16), C, nullptr, 0, w1, b1, nullptr, 0, nullptr,
                           static_cast<float*>(o16), B, H, W, Cout, 9, scale);
    c.bias_x = b2;
    c.wq = wq1; c.terms = 1; c.wq_f16 = dt == DT_F16 ? 1 : 0;
    c.wfrag = wf1;
    c.sc1 = a1; c.SC1 = XC1; c.sc2 = a2; c.SC2 = XC2; c.wfrag_sc = wf2;
    c.in_dt = dt; c.out_dt = dt;
    if (gn_mean) {
        c.gn = GnParams{gn_mean, gn_scale, gn_beta};
        c.gn_silu = silu;
    }
    rc = launch_conv(c, s);
    if (rc != OK) return rc;
    return launch_convert(o16, dt, out, DT_F32, M * Cout, s);
}

int flowse_op_pc16_channel_blocks(int mode) {
    pc16_set_channel_blocks(mode);
    return OK;
}

int flowse_op_fir_up(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    GnParams p{nullptr, nullptr, nullptr};
    return launch_fir_up(in, B, H, W, C, p, 0, nullptr, out, static_cast<hipStream_t>(stream));
}
int flowse_op_fir_down(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    GnParams p{nullptr, nullptr, nullptr};
    return launch_fir_down(in, B, H, W, C, p, 0, out, static_cast<hipStream_t>(stream));
}
int flowse_op_attention(const float* qkv, float* out, int B, int L, int C, void* stream) {
    return launch_attention(qkv, B, L, C, out, static_cast<hipStream_t>(stream));
}
// 16-bit attention core: the fp32 tokens rounded to bf16 (dt 1) / half (dt 2) in scratch, attention16_kernel, result widened
int flowse_op_attention_16(const float* qkv, float* out, int B, int L, int C, int dt, void* scratch, int64_t scratch_bytes,
                           void* stream) {
    if (!qkv || !out || !scratch || (dt != DT_BF16 && dt != DT_F16) || B < 1 || L < 1 || C < 1) {
        set_error("flowse_op_attention_16: bad argument");
        return ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * L * C;
    const int64_t need = Carver::up(2 * 3 * n) + Carver::up(2 * n);
    if (scratch_bytes < need) {
        set_error("flowse_op_attention_16: scratch needs %lld bytes", (long long)need);
        return ERR_ARG;
    }
    Carver cv{static_cast<char*>(scratch)};
    void* q16 = cv.take(2 * 3 * n);
    void* o16 = cv.take(2 * n);
    int rc = launch_convert(qkv, DT_F32, q16, dt, 3 * n, s);
    if (rc == OK) rc = launch_attention(q16, B, L, C, o16, s, dt);
    if (rc != OK) return rc;
    return launch_convert(o16, dt, out, DT_F32, n, s);
}
int flowse_op_gfp(const float* t, const float* W, float* out, int B, int E, void* stream) {
    return launch_gfp(t, W, B, E, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
