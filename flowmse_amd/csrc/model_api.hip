// Model handle, part 3, the handle proper: plan lookup and execution (plain launches, optional hipGraph replay), the stream
// fence, device state and weight upload, and the handle's own entries of the C ABI (include/flowse_hip.h): create, destroy
// and view, block handles, parameter info, precision, load_weights, reserve, flowse_vf_forward, the device-bytes and
// holders queries, the profiler.  Every other entry lives beside its kernels (spec.hip, misc.hip, noise.hip, rk45.hip,
// resample.hip, metrics.hip, fmloss.hip), in rk_fixed.hip (fixed-step samplers) or in ops_api.hip (per-op entries).
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

int run_plan(flowse_model* m, Plan* p, hipStream_t s) {
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
int ensure_stream(flowse_model* m) {
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
    f(w->d_w); f(w->d_wq); f(w->d_w16);
    for (auto& c : w->copies) f(c.buf);
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

static bool weights_shared(const flowse_model* m, const char* what) {
    if (!m->is_view && m->wt->holders == 1) return false;
    set_error("%s: the weight set is shared by %d handles; destroy the views first", what, m->wt->holders);
    return true;
}

// ------------------------------------------------------------------------- flowse_model_load_weights, table by table
// Each step derives one table of the set from the packed fp32 blob that is already in d_w (and from the packer's list of
// convs).  The weight buffers grow without a synchronisation: the upload synchronises once, before the first of them.

// 16-bit storage modes: the elementwise 16-bit twin of the packed blob (conv weights keep their offsets)
static int upload_16bit_twin(WeightSet* w, int64_t n) {
    if (const int rc = w->d_w16.reserve((n + 3) & ~(int64_t)3, false)) return rc;
    return launch_convert(w->d_w, DT_F32, w->d_w16, w->act_dt, n & ~(int64_t)3, nullptr);
}

// Copy k of conv_copy for every conv its rule names, derived on the device
static int upload_copy(WeightSet* w, const Packer& pk, int k) {
    const ConvCopy& cp = conv_copy(k);
    WeightSet::Copy& c = w->copies[k];
    c.at.clear();
    int64_t total = 0;
    for (auto& r : pk.convs) {
        if (!cp.gets(r.Cout, r.taps, r.Cin, w->act_dt)) continue;
        c.at[r.off] = cp.mirror ? r.off : total;
        total += (cp.numel(r.Cout, r.taps, r.Cin) + 63) & ~(int64_t)63;
    }
    if (c.at.empty()) return OK;
    if (cp.mirror) total = (int64_t)pk.host.size();
    if (const int rc = c.buf.reserve((size_t)total * cp.esize, false)) return rc;
    for (auto& r : pk.convs) {
        const auto it = c.at.find(r.off);
        if (it == c.at.end()) continue;
        const void* w16 = w->storage16() ? w->d_w16 + r.off : nullptr;
        if (const int rc = cp.make(w->d_w + r.off, w16, r.Cout, r.taps, r.Cin, c.buf.p + it->second * cp.esize, nullptr)) return rc;
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
    if (w->storage16()) rc = upload_16bit_twin(w, (int64_t)pk.host.size());
    for (int k = 0; k < CW_COPIES && rc == OK; ++k) rc = upload_copy(w, pk, k);
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
    return on_handle_stream(m, stream, [&](hipStream_t s) {
        CallBlock cb{static_cast<const float*>(x), static_cast<const float*>(y), t, static_cast<float*>(out), mode, 0.f};
        rc = launch_set_call(m->d_call, cb, s);
        if (rc == OK) rc = exec_plan(m, p, s);
        return rc;
    });
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

}  // extern "C"
