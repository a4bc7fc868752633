// Model handle, part 2: the launch plan.  Mirrors NCSNpp.forward (flowmse/backbones/ncsnpp.py:247-404: the order the
// modules are consumed in).  The forward pass is "traced" once per input shape into a flat list of kernel launches over
// an arena-planned activation workspace: no allocation, no host synchronisation and no shape logic inside the N-step
// solver loop.
#include "model.h"

namespace flowse {

static bool in_list(const int32_t* v, int n, int x) {
    for (int i = 0; i < n; ++i)
        if (v[i] == x) return true;
    return false;
}

// ------------------------------------------------------------------------------------------- plan builder
struct GnBuf {
    size_t mean = 0, scale = 0;
    int64_t beta = -1;
};

// A split-K convolution whose reduction is left to another conv's reduction launch (ConvArgs::partial2)
struct SkPartial {
    size_t part_off = 0;
    int ks = 0;
    int64_t bias = -1;
};
// The 1x1 shortcut Conv_2(x) of a ResnetBlock folded into Conv_1's launch (ConvArgs::sc1, conv3x3_pc16_kernel only)
struct ScFold {
    const Tn* s1 = nullptr;
    const Tn* s2 = nullptr;             // second part of a concat input, or null
    int64_t w = -1, bias = -1;          // packed offsets of Conv_2's weight / bias
};
// The GroupNorm that consumes a split-K conv's output, finished in its reduction launch (launch_splitk_reduce_gn).
// apply: the conv returns act(GroupNorm(out)); else it returns out and leaves per-channel mean / scale in `g`.
struct GnFuse {
    int64_t w_gamma = -1, w_beta = -1;
    bool silu = true, apply = false;
    GnBuf g;
};

// One conv of the plan (Builder::conv).  conv_req() fills what every conv has; a call site names what else differs from
// the defaults.  Everything here is a command: a conv whose route (Builder::route) cannot do what is asked fails the plan.
struct ConvReq {
    std::string label;
    const Tn* a = nullptr;              // input
    const Tn* b2 = nullptr;             // second part of a concat input
    int64_t w = -1, bias = -1;          // packed offsets of weight / bias
    int dense_row0 = -1;                // offset of the block's Dense_0 bias within a sample's row of the table
    int Cout = 0, taps = 0;
    const Tn* res = nullptr;            // residual: out = (conv + res) * scale
    float scale = 1.f;
    bool out_is_res = false;            // in place on `res`
    const GnBuf* gin = nullptr;         // GroupNorm (+ SiLU) of the input on load
    bool gin_silu = false;
    int64_t wq_off = -1;                // offset of the reduced-precision weight copy
    int out_dt = -1;                    // < 0: Builder::alloc's choice
    SkPartial* defer = nullptr;         // leave the split-K slices to another conv's reduction (filled in: where they are)
    const SkPartial* extra = nullptr;   // slices of a deferred conv to sum in this conv's reduction
    GnFuse* gnf = nullptr;              // finish the consuming GroupNorm in the reduction (filled in: g, unless applied)
    const ScFold* fold = nullptr;       // 1x1 shortcut as extra K steps of this launch
    bool no_stats = false;              // nobody normalises the output
    int64_t bias_sc = -1;               // a second per-channel bias from the weight blob
};
static ConvReq conv_req(const char* label, const Tn& a, int64_t w, int Cout, int taps) {
    ConvReq q;
    q.label = label;
    q.a = &a;
    q.w = w;
    q.Cout = Cout;
    q.taps = taps;
    return q;
}

// label suffix: the image size an op runs at
static std::string at(int H, int W) { return "@" + std::to_string(H) + "x" + std::to_string(W); }

struct Builder {
    flowse_model* m;
    Plan* plan;
    Arena arena;
    int B;
    Builder(flowse_model* m_, Plan* plan_, int B_) : m(m_), plan(plan_), B(B_) {}

    // The storage type of a tensor nobody names one for: the model's activation type for wide tensors, fp32 for the
    // 4-channel ones (input pack, pyramids)
    int act_type(int C) const { return C > 4 ? m->wt->act_dt : DT_F32; }
    // A tensor by shape and type only (dt < 0: act_type), for asking how a conv on it will run before it exists (route()).
    // It has no storage: conv() fails the plan when handed one.
    static constexpr size_t NO_STORAGE = ~(size_t)0;
    Tn shape_only(int H, int W, int C, int dt = -1) const {
        Tn t;
        t.B = B; t.H = H; t.W = W; t.C = C;
        t.dt = dt >= 0 ? dt : act_type(C);
        t.off = NO_STORAGE;
        return t;
    }
    Tn alloc(int H, int W, int C, int dt = -1) {
        Tn t = shape_only(H, W, C, dt);
        t.off = arena.alloc(t.bytes());
        return t;
    }
    void release(const Tn& t) {
        if (!t.valid()) return;
        arena.release(t.off);
        if (t.st_nblk > 0) arena.release(t.st_off);
    }
    void drop_stats(Tn& t) {          // the tensor was modified in place: its fused statistics are stale
        if (t.st_nblk > 0) arena.release(t.st_off);
        t.st_nblk = 0;
    }
    bool failed = false;                   // an internal planning inconsistency: build_plan returns ERR_STATE
    void op(const std::string& label, std::function<int(hipStream_t)> f, double flops = 0.0, double bytes = 0.0,
            bool dominant = false, double issued = -1.0) {
        plan->ops.push_back(std::move(f));
        plan->labels.push_back(label);
        plan->flops.push_back(flops);
        plan->bytes.push_back(bytes);
        plan->issued.push_back(issued < 0.0 ? flops : issued);
        plan->dominant.push_back(dominant ? 1 : 0);
    }

    // Where the statistics partials of a GroupNorm's one or two source tensors are: the producing conv's fused ones when
    // present, else a temporary buffer that a gn_stats launch (emitted here) fills.  The temporaries are allocated here,
    // source 0 then source 1, and released by release_temp() once the consuming op is emitted.
    struct StatSrc {
        size_t off[2] = {0, 0};
        int nblk[2] = {0, 0};
        bool temp[2] = {false, false};
    };
    StatSrc stat_sources(const Tn& a, const Tn* b2) {
        flowse_model* M = m;
        const int HW = a.H * a.W, Bn = B;
        StatSrc st;
        const Tn* src[2] = {&a, b2};
        for (int k = 0; k < 2; ++k) {
            if (!src[k]) continue;
            if (src[k]->st_nblk > 0) {
                st.off[k] = src[k]->st_off;
                st.nblk[k] = src[k]->st_nblk;
                continue;
            }
            const int Ck = src[k]->C;
            const int nblk = gn_partial_blocks(HW, Ck);
            st.off[k] = arena.alloc((size_t)Bn * nblk * Ck * 2 * sizeof(float));
            st.nblk[k] = nblk;
            st.temp[k] = true;
            const size_t t_off = src[k]->off, p_off = st.off[k];
            const int sdt = src[k]->dt;
            op("gn_stats" + at(src[k]->H, src[k]->W), [=](hipStream_t s) {
                return launch_gn_stats(M->A(t_off), Ck, nullptr, 0, Bn, HW, M->A(p_off), nblk, s, sdt);
            }, 3.0 * Bn * HW * Ck, (double)dt_size(sdt) * Bn * HW * Ck);
        }
        return st;
    }
    void release_temp(const StatSrc& st) {
        for (int k = 0; k < 2; ++k)
            if (st.temp[k]) arena.release(st.off[k]);
    }
    // statistics + finalize; returns per-(b,c) mean / scale buffers (caller releases)
    GnBuf gn(const Tn& a, const Tn* b2, int64_t w_gamma, int64_t w_beta) {
        flowse_model* M = m;
        const int C1 = a.C, C2 = b2 ? b2->C : 0, C = C1 + C2, HW = a.H * a.W, Bn = B;
        const int G = std::min(C / 4, 32);
        const StatSrc st = stat_sources(a, b2);
        GnBuf g;
        g.mean = arena.alloc((size_t)Bn * C * sizeof(float));
        g.scale = arena.alloc((size_t)Bn * C * sizeof(float));
        g.beta = w_beta;
        const size_t gm = g.mean, gs = g.scale, p0 = st.off[0], p1 = st.off[1];
        const int n0 = st.nblk[0], n1 = st.nblk[1];
        const bool has2 = b2 != nullptr;
        op("gn_finalize" + at(a.H, a.W), [=](hipStream_t s) {
            return launch_gn_finalize(M->A(p0), n0, C1, has2 ? M->A(p1) : nullptr, n1, C2, Bn, HW, G, M->W(w_gamma),
                                      1e-6f, M->A(gm), M->A(gs), s);
        });
        release_temp(st);
        return g;
    }
    // GroupNorm (+ SiLU) materialised into a new tensor.  Small images: statistics finalize and the apply pass are ONE
    // launch (a block per (group, sample) reduces the partials and normalises its HW x C/G elements); otherwise
    // finalize + float4 apply.
    // out_dt < 0: same storage type as the input
    Tn gn_norm(const Tn& a, const Tn* b2, int64_t w_gamma, int64_t w_beta, bool silu, int out_dt = -1) {
        const int C1 = a.C, C2 = b2 ? b2->C : 0, C = C1 + C2, HW = a.H * a.W, Bn = B;
        const int G = std::min(C / 4, 32);
        const int idt = a.dt, odt = out_dt >= 0 ? out_dt : a.dt;
        if ((int64_t)HW * (C / G) > 8192) {
            GnBuf g = gn(a, b2, w_gamma, w_beta);
            Tn o = gn_apply(a, b2, g, silu, odt);
            gn_release(g);
            return o;
        }
        flowse_model* M = m;
        const StatSrc st = stat_sources(a, b2);
        Tn o = alloc(a.H, a.W, C, odt);
        const size_t a_off = a.off, b_off = b2 ? b2->off : 0, o_off = o.off, p0 = st.off[0], p1 = st.off[1];
        const int n0 = st.nblk[0], n1 = st.nblk[1];
        const bool has2 = b2 != nullptr;
        op("gn_norm" + at(a.H, a.W), [=](hipStream_t s) {
            return launch_gn_finalize_apply(M->A(a_off), M->A(p0), n0, C1, has2 ? M->A(b_off) : nullptr,
                                            has2 ? M->A(p1) : nullptr, n1, C2, Bn, HW, G, M->W(w_gamma), M->W(w_beta),
                                            1e-6f, silu ? 1 : 0, M->A(o_off), s, idt, odt);
        }, 8.0 * Bn * HW * C, (double)(dt_size(idt) + dt_size(odt)) * Bn * HW * C);
        release_temp(st);
        return o;
    }
    void gn_release(const GnBuf& g) {
        arena.release(g.mean);
        arena.release(g.scale);
    }
    Tn gn_apply(const Tn& a, const Tn* b2, const GnBuf& g, bool silu, int out_dt = -1) {
        flowse_model* M = m;
        const int C1 = a.C, C2 = b2 ? b2->C : 0, HW = a.H * a.W, Bn = B;
        const int idt = a.dt, odt = out_dt >= 0 ? out_dt : a.dt;
        Tn o = alloc(a.H, a.W, C1 + C2, odt);
        const size_t a_off = a.off, b_off = b2 ? b2->off : 0, o_off = o.off;
        const bool has2 = b2 != nullptr;
        op("gn_apply" + at(a.H, a.W), [=](hipStream_t s) {
            GnParams p{M->A(g.mean), M->A(g.scale), M->W(g.beta)};
            return launch_gn_apply(M->A(a_off), C1, has2 ? M->A(b_off) : nullptr, C2, Bn, HW, p, silu ? 1 : 0,
                                   M->A(o_off), s, idt, odt);
        }, 8.0 * Bn * HW * (C1 + C2), (double)(dt_size(idt) + dt_size(odt)) * Bn * HW * (C1 + C2));
        return o;
    }
    // What the weight set holds for the conv weight at packed offset w, read as storage type idt (wq_off: its bf16 planes)
    ConvOffer offer(int idt, int64_t w, int taps, int64_t wq_off) const {
        const WeightSet& ws = *m->wt;
        ConvOffer of;
        if (idt != DT_F32) {                             // [Cout][taps][Cin] in the storage type, + the fragment-order copy
            of.wq = true;
            of.terms = 1;
            of.wq_f16 = idt == DT_F16;
            of.wfrag = ws.has_copy(CW_WFRAG, w);
        } else {
            of.wino = ws.has_copy(CW_WINO, w);
            of.wino2 = ws.has_copy(CW_WINO2, w);
            of.wsm = ws.has_copy(CW_WSM, w);         // (and CW_WSM16: one rule)
            of.wq = !m->storage16() && wq_off >= 0 && ws.precision != 0 && taps == 9;
            of.terms = !of.wq ? 0 : ws.precision == 1 ? 3 : 1;
            of.wq_f16 = of.wq && ws.precision == 3;
        }
        of.slab = true;                                  // the arena has room for one
        return of;
    }
    // The routing question of a request: its shape, and as the offer what the weight set holds for its weight.  A function
    // of the request alone -- conv() asks it of the request it emits, resblock of the requests it is about to submit, on
    // shape_only() tensors where they do not exist yet.
    struct ConvQuery { ConvShape shape; ConvOffer offer; };
    ConvQuery query(const ConvReq& q) const {
        const Tn& a = *q.a;
        const int odt = q.out_is_res ? q.res->dt : q.out_dt >= 0 ? q.out_dt : act_type(q.Cout);   // = alloc()'s choice in conv()
        ConvOffer of = offer(a.dt, q.w, q.taps, q.wq_off);
        of.gn = q.gin != nullptr;
        of.bias2 = q.dense_row0 >= 0 || q.bias_sc >= 0;
        // statistics of the output where somebody normalises it.  In place on `res`, only Combine's (conv1x1 of the 4-channel
        // pyramid, any storage type of `res`) are used: they are those of the updated tensor
        const bool combine = q.out_is_res && q.taps == 1 && a.C == 4 && !q.b2 && a.dt == DT_F32;
        of.stats = q.Cout >= 16 && !q.no_stats && (!q.out_is_res || combine);
        of.fold = q.fold != nullptr;
        return {ConvShape{a.dt, odt, B, a.H, a.W, a.C, q.b2 ? q.b2->C : 0, q.Cout, q.taps}, of};
    }
    // ... and its answer: which kernel runs, over how many K slices (.ksplit), whether it normalises on load (.gn_on_load)
    ConvRoute route(const ConvReq& q) const { const ConvQuery c = query(q); return conv_route(c.shape, c.offer); }
    // conv: out (new tensor unless `out_is_res`), res optional
    Tn conv(const ConvReq& q) {
        flowse_model* M = m;
        // locals: the launch closures below copy what they use -- they outlive the request and the Builder
        const std::string& label = q.label;
        const Tn& a = *q.a;
        const Tn *b2 = q.b2, *res = q.res;
        const int64_t w = q.w, bias = q.bias, wq_off = q.wq_off, bias_sc = q.bias_sc;
        const int dense_row0 = q.dense_row0, Cout = q.Cout, taps = q.taps, out_dt = q.out_dt;
        const float scale = q.scale;
        const bool out_is_res = q.out_is_res, gin_silu = q.gin_silu;
        const GnBuf* gin = q.gin;
        const SkPartial* extra = q.extra;
        const ScFold* fold = q.fold;
        SkPartial* defer = q.defer;
        GnFuse* gnf = q.gnf;
        const int C1 = a.C, C2 = b2 ? b2->C : 0, H = a.H, Wd = a.W, Bn = B;
        if (bias_sc >= 0 && dense_row0 >= 0) {           // both ride on ConvArgs::bias2
            set_error("internal: a second per-channel bias and a Dense row on one conv (%s)", label.c_str());
            failed = true;
        }
        for (const Tn* t : {q.a, b2, res, fold ? fold->s1 : nullptr, fold ? fold->s2 : nullptr})
            if (t && t->off == NO_STORAGE) {
                set_error("internal: %s submitted on a tensor that was never allocated", label.c_str());
                failed = true;
            }
        const int idt = a.dt;
        const bool in16 = idt != DT_F32;                 // 16-bit storage: the 16-bit matrix-core kernels take it
        const bool has_gin = gin != nullptr, has_fold = fold != nullptr;
        // The one routing question of this conv, asked once.  The answer says which kernel runs, over how many K slices and
        // where its statistics go; the launch closure keeps it.
        const ConvQuery cq = query(q);
        const ConvOffer& of = cq.offer;
        const ConvRoute rt = conv_route(cq.shape, of);
        if (rt.err != OK) {
            set_error("internal: no kernel takes %s@%dx%d (%s)", label.c_str(), H, Wd, rt.err_text);
            failed = true;
        }
        const int ks = rt.ksplit;
        // What the request says about the reduction launch holds only for a conv that has one (and a deferred one leaves no
        // output tensor: checked before anything is allocated)
        if (((defer || extra || gnf) && !(ks > 1)) || (defer && (res || dense_row0 >= 0)) ||
            (gnf && (res || !conv_reduce_gn_ok(Bn, H * Wd, Cout)))) {
            set_error("internal: %s@%dx%d runs over %d K slice(s) and cannot take the reduction planned for it", label.c_str(),
                      H, Wd, ks);
            failed = true;
            defer = nullptr; extra = nullptr; gnf = nullptr;
        }
        Tn o;
        if (!defer) o = out_is_res ? *res : alloc(a.H, a.W, Cout, out_dt);
        const size_t a_off = a.off, b_off = b2 ? b2->off : 0, o_off = o.off, r_off = res ? res->off : 0;
        const bool has2 = b2 != nullptr, hasres = res != nullptr;
        const int odt = o.dt;                            // (a deferred conv has no output tensor: fp32, as its slices are)
        // statistics of the output: where asked for, in the geometry of the kernel that runs -- unless there is no output here
        // (defer) or they are finished inside the reduction (gnf)
        const int st_nblk = of.stats && !defer && !gnf ? rt.stats_nblk : 0;
        if (out_is_res && o.st_nblk > 0) {               // updated in place: the producer's statistics are stale
            arena.release(o.st_off);
            o.st_nblk = 0;
        }
        if (st_nblk > 0) {
            o.st_nblk = st_nblk;
            o.st_off = arena.alloc((size_t)Bn * st_nblk * Cout * 2 * sizeof(float));
        }
        const size_t st_off = o.st_off;
        const GnBuf gbuf = has_gin ? *gin : GnBuf();
        // the derived copies the route's kernel reads: it chose among what offer() found in the weight set (the buffers
        // stay where they are for as long as the plan lives: an upload drops the plans)
        std::array<const void*, CW_COPIES> wcopy{};
        for (int k = 0; k < CW_COPIES; ++k)
            if (rt.reads_weight(k) && !(wcopy[k] = M->wt->copy_ptr(k, w))) {
                set_error("internal: %s@%dx%d runs %s, whose %s copy was not uploaded", label.c_str(), H, Wd,
                          conv_kernel_name(rt.kernel), conv_copy(k).name);
                failed = true;
            }
        const int terms = M->wt->precision == 1 ? 3 : 1;
        const size_t part_off = ks > 1 ? arena.alloc((size_t)ks * Bn * H * Wd * Cout * sizeof(float)) : 0;
        const size_t table_off = M_table_off;     // by value: the Builder dies before the plan runs
        const bool has_extra = extra != nullptr;
        const SkPartial xp = has_extra ? *extra : SkPartial();
        const size_t f1_off = has_fold ? fold->s1->off : 0, f2_off = has_fold && fold->s2 ? fold->s2->off : 0;
        const int FC1 = has_fold ? fold->s1->C : 0, FC2 = has_fold && fold->s2 ? fold->s2->C : 0;
        const int64_t fold_w = has_fold ? fold->w : -1, fold_b = has_fold ? fold->bias : -1;
        const void* wfrag_sc = has_fold ? M->wt->copy_ptr(CW_WFRAG, fold_w) : nullptr;
        // (that the conv itself is a whole-K launch of the producer / consumer kernel is the route's answer to of.fold: rt.err
        // above.  Here: what the route is not asked -- the other riders on the launch, the fold's source, its weight copy)
        if (has_fold && (res || extra || fold->s1->H != H || fold->s1->W != Wd || fold->s1->dt != idt || !wfrag_sc)) {
            set_error("internal: shortcut fold requested for a conv that cannot take it (%s)", label.c_str());
            failed = true;
        }
        const std::string full_label = label + at(H, Wd) + ":" +
                                       std::to_string(C1 + C2) + (has_fold ? "+" + std::to_string(FC1 + FC2) : std::string()) +
                                       ">" + std::to_string(Cout);
        auto make_args = [=]() {
            ConvArgs c;
            c.in1 = M->A(a_off);
            c.in2 = has2 ? M->A(b_off) : nullptr;
            c.C1 = C1;
            c.C2 = C2;
            c.w = M->W(w);
            c.bias = bias >= 0 ? M->W(bias) : nullptr;
            // bias_sc: a second per-channel bias from the weight blob (the same row for every sample: stride 0)
            c.bias2 = dense_row0 >= 0 ? M->A(table_off) + dense_row0 : bias_sc >= 0 ? M->W(bias_sc) : nullptr;
            c.bias2_stride = dense_row0 >= 0 ? M->wt->dense_rows : 0;
            c.res = hasres ? M->A(r_off) : nullptr;
            c.out = M->A(o_off);
            c.B = Bn; c.H = H; c.W = Wd; c.Cout = Cout;
            c.taps = taps;
            c.scale = scale;
            c.ksplit = ks;
            c.partial = ks > 1 ? M->A(part_off) : nullptr;
            if (has_extra) {
                c.partial2 = M->A(xp.part_off);
                c.ksplit2 = xp.ks;
                c.bias_x = xp.bias >= 0 ? M->W(xp.bias) : nullptr;
            }
            c.stats = st_nblk > 0 ? M->A(st_off) : nullptr;
            c.stats_nblk = st_nblk;
            if (has_gin) {
                c.gn = GnParams{M->A(gbuf.mean), M->A(gbuf.scale), M->W(gbuf.beta)};
                c.gn_silu = gin_silu ? 1 : 0;
            }
            if (has_fold) {                               // Conv_2(x) as extra K steps of this launch
                c.sc1 = M->A(f1_off);
                c.SC1 = FC1;
                c.sc2 = FC2 ? M->A(f2_off) : nullptr;
                c.SC2 = FC2;
                c.wfrag_sc = wfrag_sc;
                c.bias_x = fold_b >= 0 ? M->W(fold_b) : nullptr;
            }
            c.in_dt = idt;
            c.out_dt = odt;
            for (int k = 0; k < CW_COPIES; ++k)
                if (wcopy[k]) conv_set_weight(c, k, wcopy[k]);
            if (in16) {                                   // [Cout][taps][Cin] in the storage type: same offsets as d_w
                c.terms = 1;
                c.wq_f16 = idt == DT_F16 ? 1 : 0;
                if (rt.reads_weight(CW_WQ)) conv_set_weight(c, CW_WQ, M->wt->d_w16 + w);
            } else if (rt.reads_weight(CW_WQ)) {           // the bf16 planes
                c.terms = terms;
                c.wq_f16 = M->wt->precision == 3 ? 1 : 0;
                conv_set_weight(c, CW_WQ, M->wt->d_wq + wq_off);
            }
            return c;
        };
        const double flops = 2.0 * Bn * H * Wd * (double)Cout * (taps * (C1 + C2) + (FC1 + FC2));
        const double out_bytes = (double)dt_size(odt) * Bn * H * Wd * Cout * (hasres ? 2 : 1);
        const double in_bytes = (double)dt_size(idt) * ((double)Bn * H * Wd * (C1 + C2 + FC1 + FC2) +
                                                        (double)Cout * (taps * (C1 + C2) + (FC1 + FC2)));
        const double part_bytes = 4.0 * ks * (double)Bn * H * Wd * Cout;
        op(full_label, [=](hipStream_t s) {
            const ConvArgs c = make_args();
            return launch_conv_routed(c, rt, s, false);
        }, flops, in_bytes + (ks > 1 ? part_bytes : out_bytes),
           // the roofline's kernel: a whole-K 3x3 that normalises on load -- of those counted at half the FLOPs (the F(4,3)
           // weights), only the launches that use 128-channel blocks
           has_gin && Cout > 64 && ks == 1 && (rt.issued != 0.5 || conv_f43_wide(Bn, H, Wd, Cout)), flops * rt.issued);
        if (defer) {                                     // the consumer's reduction sums these slices (ConvArgs::partial2)
            defer->part_off = part_off;
            defer->ks = ks;
            defer->bias = bias;
            return Tn();
        }
        if (gnf) {
            const int64_t wg = gnf->w_gamma, wb = gnf->w_beta;
            const bool gsilu = gnf->silu, gapply = gnf->apply;
            GnBuf g;
            if (!gapply) {
                g.mean = arena.alloc((size_t)Bn * Cout * sizeof(float));
                g.scale = arena.alloc((size_t)Bn * Cout * sizeof(float));
                g.beta = wb;
            }
            const size_t gm = g.mean, gs = g.scale;
            op("splitk_reduce_gn" + at(H, Wd), [=](hipStream_t s) {
                return launch_splitk_reduce_gn(make_args(), M->W(wg), M->W(wb), 1e-6f, gsilu ? 1 : 0, gapply ? 1 : 0,
                                               gapply ? nullptr : M->A(gm), gapply ? nullptr : M->A(gs), s);
            }, 8.0 * Bn * H * Wd * Cout, part_bytes + out_bytes);
            gnf->g = g;
        } else if (ks > 1)
            op("splitk_reduce" + at(H, Wd), [=](hipStream_t s) { return launch_splitk_reduce(make_args(), s); }, 0.0,
               part_bytes * (has_extra ? 1.0 + (double)xp.ks / ks : 1.0) + out_bytes);
        if (ks > 1) arena.release(part_off);
        return o;
    }
    size_t M_table_off = 0;     // arena offset of the Dense_0 bias table [B][dense_rows]

    // raw_out (optional): receives the same resampling of the un-normalised input (one read of `a` for both)
    Tn fir(const Tn& a, bool up, const GnBuf* g, bool silu, const Tn* add, bool out_is_add = false,
           Tn* raw_out = nullptr) {
        flowse_model* M = m;
        const int H = a.H, Wd = a.W, C = a.C, Bn = B;
        const int fdt = a.dt;
        Tn o = out_is_add ? *add : (up ? alloc(2 * H, 2 * Wd, C, fdt) : alloc(H / 2, Wd / 2, C, fdt));
        if (raw_out) *raw_out = up ? alloc(2 * H, 2 * Wd, C, fdt) : alloc(H / 2, Wd / 2, C, fdt);
        const size_t a_off = a.off, o_off = o.off, add_off = add ? add->off : 0, r_off = raw_out ? raw_out->off : 0;
        const bool hasg = g != nullptr, hasadd = add != nullptr, hasraw = raw_out != nullptr;
        GnBuf gb = hasg ? *g : GnBuf();
        const double outs = hasraw ? 2.0 : 1.0;
        op((up ? "fir_up" : "fir_down") + at(H, Wd), [=](hipStream_t s) {
            GnParams p{nullptr, nullptr, nullptr};
            if (hasg) p = GnParams{M->A(gb.mean), M->A(gb.scale), M->W(gb.beta)};
            if (up)
                return launch_fir_up(M->A(a_off), Bn, H, Wd, C, p, silu ? 1 : 0, hasadd ? M->A(add_off) : nullptr,
                                     M->A(o_off), s, hasraw ? M->A(r_off) : nullptr, fdt);
            return launch_fir_down(M->A(a_off), Bn, H, Wd, C, p, silu ? 1 : 0, M->A(o_off), s,
                                   hasraw ? M->A(r_off) : nullptr, fdt);
        }, (up ? 8.0 * 4 : 32.0 / 4) * Bn * H * Wd * C * outs,
           (double)dt_size(fdt) * Bn * H * Wd * C * (up ? 1.0 + 4.0 * outs : 1.0 + 0.25 * outs));
        return o;
    }

    // What a ResnetBlock fuses.  Small images run their convs split over K with a separate reduction launch, and two of
    // those launches disappear: Conv_0's reduction also finishes GroupNorm_1 (its group structure is known), and the
    // shortcut Conv_2(x) leaves its slices to Conv_1's reduction, which sums both sets.  Large 16-bit images run the
    // shortcut as extra K steps of Conv_1's launch; large fp32 up blocks run it before the upsampling.
    struct BlockPlan {
        // Conv_2(x): no such conv (identity skip) | a launch of its own | ... at the low resolution, upsampled afterwards |
        // its K slices summed by Conv_1's reduction (SkPartial) | extra K steps of Conv_1's launch (ScFold)
        enum { SC_NONE, SC_OWN, SC_LOW, SC_MERGED, SC_FOLDED } sc = SC_NONE;
        bool gn0_on_load = false;       // Conv_0 normalises x on load; else act(GroupNorm_0(x)) is materialised
        // GroupNorm_1: Conv_0's reduction returns act(GroupNorm_1(.)) | ... returns the pre-norm tensor and per-channel mean /
        // scale for a Conv_1 that normalises on load (GnFuse) | gn() and Conv_1 on load | materialised
        enum { GN1_REDUCE_APPLY, GN1_REDUCE_STATS, GN1_ON_LOAD, GN1_MATERIAL } gn1 = GN1_MATERIAL;
    };

    // ResnetBlockBigGANpp.forward, layerspp.py:245-274: decide what is fused, then emit
    Tn resblock(const Module& mod, const Tn& x1, const Tn* x2) {
        const float rs2 = 0.70710678118654752440f;
        const bool resample = mod.up || mod.down;
        // output geometry of the block (Conv_0 already runs at the resampled size)
        const int Ho = mod.up ? 2 * x1.H : mod.down ? x1.H / 2 : x1.H, Wo = mod.up ? 2 * x1.W : mod.down ? x1.W / 2 : x1.W;
        // What every request for the shortcut Conv_2 / for Conv_0 / for Conv_1 has in common; the call sites name the rest
        auto shortcut = [&](const Tn& s) {
            ConvReq r = conv_req("conv2_1x1", s, mod.w_c2, mod.out_ch, 1);
            r.bias = mod.w_c2_b;
            r.no_stats = true;                           // a residual only: nobody normalises it
            return r;
        };
        auto conv0 = [&](const char* label, const Tn& s) {
            ConvReq r = conv_req(label, s, mod.w_c0, mod.out_ch, 9);
            r.dense_row0 = mod.dense_row0;               // Conv_0.bias rides in the Dense_0 table
            return r;
        };
        auto conv1 = [&](const char* label, const Tn& s) {
            ConvReq r = conv_req(label, s, mod.w_c1, mod.out_ch, 9);
            r.bias = mod.w_c1_b;
            r.scale = rs2;
            return r;
        };

        // ---- decide, before anything is allocated or emitted.  q0 / q1 are the requests for Conv_0 / Conv_1 that are
        // submitted below, here on tensors named by shape and type where these do not exist yet.  A fusion that changes the
        // routing question (GroupNorm on load, the fold) is decided from the route without it and then added to the request:
        // conv()'s own query confirms it, and fails the plan if a route cannot do what this record says.
        const int xc2 = (!resample && x2) ? x2->C : 0;
        const Tn xr_s = shape_only(Ho, Wo, x1.C, x1.dt);             // fir()'s outputs: x resampled, raw and as act(GN_0(x))
        const Tn h0_s = shape_only(x1.H, x1.W, x1.C + xc2, x1.dt);   // gn_norm()'s output
        const Tn h1_s = shape_only(Ho, Wo, mod.out_ch);              // Conv_0's output; GroupNorm_1 keeps shape and type
        BlockPlan bp;
        ConvReq q0 = resample ? conv0("conv0_3x3", xr_s) : conv0("conv0_3x3_gn", x1);
        q0.wq_off = mod.wq_c0;
        if (!resample) {
            q0.b2 = x2;
            bp.gn0_on_load = route(q0).gn_on_load;
            if (!bp.gn0_on_load) q0 = conv0("conv0_3x3", h0_s);
        }
        const bool reduce_gn1 = route(q0).ksplit > 1 && conv_reduce_gn_ok(B, Ho * Wo, mod.out_ch);
        ConvReq q1 = conv1("conv1_3x3_gn", h1_s);
        q1.wq_off = mod.wq_c1;
        const ConvRoute c1 = route(q1);
        if (!c1.gn_on_load) q1 = conv1("conv1_3x3", h1_s);
        bp.gn1 = reduce_gn1 ? (c1.gn_on_load ? BlockPlan::GN1_REDUCE_STATS : BlockPlan::GN1_REDUCE_APPLY)
                            : (c1.gn_on_load ? BlockPlan::GN1_ON_LOAD : BlockPlan::GN1_MATERIAL);
        if (mod.shortcut) {
            ConvReq qs = shortcut(resample ? xr_s : x1);
            if (!resample) qs.b2 = x2;
            const bool merge = c1.ksplit > 1 && route(qs).ksplit > 1;
            // 16-bit storage, Conv_1 on the producer / consumer kernel: no launch, no round trip of Conv_2's output through
            // HBM, one read of x less.  (Next to the route: what the kernel asks of the fold's source and weight.)
            const bool fold = !merge && m->wt->act_dt != DT_F32 && !getenv("FLOWSE_NO_SCFOLD") && c1.kernel == CK_PC16 &&
                              m->wt->has_copy(CW_WFRAG, mod.w_c2) && (x1.C % 32) == 0 && (xc2 % 32) == 0 && x1.C + xc2 >= 96 &&
                              x1.dt == m->wt->act_dt;
            // fp32 up blocks whose shortcut is a launch of its own: Conv_2 has no spatial extent and upsample_2d filters every
            // channel alike, so W . up(x) = up(W . x) -- the 1x1 runs BEFORE the upsampling, on a quarter of the pixels, and the
            // upsampled raw x never exists.  Only the bias does not commute (up(const) is not constant at the image border):
            // Conv_1's epilogue adds it, once per output element.  Up to 2048 low-resolution pixels over the batch the
            // reference's order stays (small-image kernels, shortcuts merged into split-K reductions: not measured in the
            // other order).
            const bool low = mod.up && !merge && !fold && m->wt->act_dt == DT_F32 && x1.dt == DT_F32 &&
                             (int64_t)B * x1.H * x1.W > 2048 && !getenv("FLOWSE_NO_SC_LOW");
            bp.sc = merge ? BlockPlan::SC_MERGED : fold ? BlockPlan::SC_FOLDED : low ? BlockPlan::SC_LOW : BlockPlan::SC_OWN;
        }
        const bool sc_launch = bp.sc == BlockPlan::SC_OWN || bp.sc == BlockPlan::SC_MERGED;
        const bool merged = bp.sc == BlockPlan::SC_MERGED, folded = bp.sc == BlockPlan::SC_FOLDED;

        // ---- emit
        GnFuse gf;
        gf.w_gamma = mod.w_gn1_g;
        gf.w_beta = mod.w_gn1_b;
        gf.silu = true;
        gf.apply = bp.gn1 == BlockPlan::GN1_REDUCE_APPLY;
        if (reduce_gn1) q0.gnf = &gf;
        SkPartial sp;
        Tn h1, xs, xr;
        if (!resample) {
            if (sc_launch) {
                ConvReq r = shortcut(x1);
                r.b2 = x2;
                if (merged) r.defer = &sp;
                xs = conv(r);
            }
            if (bp.gn0_on_load) {
                // Conv_0(act(GroupNorm_0(x))) in one kernel: the normalised tensor never reaches HBM
                GnBuf g0 = gn(x1, x2, mod.w_gn0_g, mod.w_gn0_b);
                q0.gin = &g0;
                q0.gin_silu = true;
                h1 = conv(q0);
                gn_release(g0);
            } else {
                Tn h0 = gn_norm(x1, x2, mod.w_gn0_g, mod.w_gn0_b, true);
                q0.a = &h0;
                h1 = conv(q0);
                release(h0);
            }
        } else if (bp.sc == BlockPlan::SC_LOW) {
            ConvReq r = shortcut(x1);
            r.bias = -1;                                 // Conv_1's epilogue adds it (bias_sc below)
            Tn xl = conv(r);
            xs = fir(xl, true, nullptr, false, nullptr);
            release(xl);
            GnBuf g0 = gn(x1, x2, mod.w_gn0_g, mod.w_gn0_b);
            Tn hr = fir(x1, true, &g0, true, nullptr);
            gn_release(g0);
            q0.a = &hr;
            h1 = conv(q0);
            release(hr);
        } else {
            GnBuf g0 = gn(x1, x2, mod.w_gn0_g, mod.w_gn0_b);
            Tn hr = fir(x1, mod.up, &g0, true, nullptr, false, &xr);      // act(GN(x)) and x resampled in one pass
            gn_release(g0);
            if (sc_launch) {                             // the shortcut Conv_2(x) (layerspp.py:268-270)
                ConvReq r = shortcut(xr);
                if (merged) r.defer = &sp;
                xs = conv(r);
            }
            q0.a = &hr;
            h1 = conv(q0);
            release(hr);
            if (!folded) release(xr);
        }
        ScFold fo;
        if (folded) {
            fo.s1 = resample ? &xr : &x1;
            fo.s2 = resample ? nullptr : x2;
            fo.w = mod.w_c2;
            fo.bias = mod.w_c2_b;
            q1.label = "conv1_3x3_gn_sc";
            q1.fold = &fo;
        }
        q1.res = (merged || folded) ? nullptr : (xs.valid() ? &xs : &x1);
        q1.extra = merged ? &sp : nullptr;
        q1.bias_sc = bp.sc == BlockPlan::SC_LOW ? mod.w_c2_b : -1;   // Conv_2's bias, left out of the low-resolution 1x1
        Tn out;
        if (bp.gn1 == BlockPlan::GN1_REDUCE_APPLY) {     // h1 already is act(GroupNorm_1(Conv_0(.)))
            q1.a = &h1;
            out = conv(q1);
            release(h1);
        } else if (bp.gn1 != BlockPlan::GN1_MATERIAL) {
            GnBuf g1 = bp.gn1 == BlockPlan::GN1_REDUCE_STATS ? gf.g : gn(h1, nullptr, mod.w_gn1_g, mod.w_gn1_b);
            q1.a = &h1;
            q1.gin = &g1;
            q1.gin_silu = true;
            out = conv(q1);
            gn_release(g1);
            release(h1);
            if (folded && resample) release(xr);
        } else {
            Tn h2 = gn_norm(h1, nullptr, mod.w_gn1_g, mod.w_gn1_b, true);
            release(h1);
            q1.a = &h2;
            out = conv(q1);
            release(h2);
        }
        if (merged) arena.release(sp.part_off);
        release(xs);
        return out;
    }

    // AttnBlockpp.forward, layerspp.py:75-91
    Tn attn(const Module& mod, const Tn& x) {
        flowse_model* M = m;
        const float rs2 = 0.70710678118654752440f;
        const int C = x.C, L = x.H * x.W, Bn = B;
        // 16-bit storage modes: the whole sub-block stays in the activation type -- GroupNorm rounds to it, the qkv
        // projection and the output projection run the 16-bit flat kernel, the attention core the 16-bit MFMA kernel
        // (fp32 softmax state / accumulation); fp32 mode: everything fp32
        const int adt = x.dt;
        Tn hn = gn_norm(x, nullptr, mod.w_gn0_g, mod.w_gn0_b, false, adt);
        ConvReq rq = conv_req("attn_qkv", hn, mod.w_qkv, 3 * C, 1);
        rq.bias = mod.w_qkv_b;
        rq.out_dt = adt;
        Tn qkv = conv(rq);
        release(hn);
        Tn o = alloc(x.H, x.W, C, adt);
        const size_t q_off = qkv.off, o_off = o.off;
        op("attention" + at(x.H, x.W), [=](hipStream_t s) { return launch_attention(M->A(q_off), Bn, L, C, M->A(o_off), s, adt); },
           4.0 * Bn * (double)L * L * C, 4.0 * dt_size(adt) * Bn * L * C);
        release(qkv);
        ConvReq ro = conv_req("attn_out", o, mod.w_o, C, 1);
        ro.bias = mod.w_o_b;
        ro.res = &x;
        ro.scale = rs2;
        ro.out_dt = x.dt;
        Tn out = conv(ro);
        release(o);
        return out;
    }
};

// Combine: conv1x1(x) + y in place on y (layerspp.py:55-59)
static ConvReq combine_req(const Module& cb, const Tn& x, const Tn& y) {
    ConvReq r = conv_req("combine_1x1", x, cb.w_a, cb.out_ch, 1);
    r.bias = cb.w_a_b;
    r.res = &y;
    r.out_is_res = true;
    return r;
}

// NCSNpp.forward, ncsnpp.py:247-404
int build_plan(flowse_model* m, Plan* plan, int B, int F, int T) {
    const flowse_config& c = m->cfg;
    const int L = c.num_levels;
    if (F != c.image_size) {
        set_error("F=%d must equal image_size=%d (attention placement, ncsnpp.py:298)", F, c.image_size);
        return ERR_SHAPE;
    }
    if (B < 1 || T < 1 || (T % (1 << (L - 1))) != 0 || (F % (1 << (L - 1))) != 0) {
        set_error("shape B=%d F=%d T=%d: T and F must be multiples of %d (pad_spec)", B, F, T, 1 << (L - 1));
        return ERR_SHAPE;
    }
    plan->B = B; plan->F = F; plan->T = T;
    Builder bd(m, plan, B);
    flowse_model* M = m;
    const int nf = c.nf, td = m->wt->temb_dim;
    size_t mi = 0;
    auto next = [&]() -> const Module& { return m->wt->mods[mi++]; };

    // ---- time embedding (depends only on t)
    const Module& gfp = next();
    const Module& lin1 = next();
    const Module& lin2 = next();
    const size_t e0 = bd.arena.alloc((size_t)B * 2 * nf * 4), e1 = bd.arena.alloc((size_t)B * td * 4),
                 e2 = bd.arena.alloc((size_t)B * td * 4);
    bd.M_table_off = bd.arena.alloc((size_t)B * m->wt->dense_rows * 4);
    const size_t table = bd.M_table_off;
    {
        const int64_t wg = gfp.w_a, w1 = lin1.w_a, b1 = lin1.w_a_b, w2 = lin2.w_a, b2 = lin2.w_a_b;
        bd.op("gfp", [=](hipStream_t s) { return launch_gfp(nullptr, M->W(wg), B, nf, M->A(e0), s, M->d_call); });
        bd.op("temb_linear1", [=](hipStream_t s) {
            return launch_linear(M->A(e0), B, 2 * nf, M->W(w1), M->W(b1), td, 1, M->A(e1), td, s);
        });
        // act(temb) is the only consumer of temb (layerspp.py:263)
        bd.op("temb_linear2", [=](hipStream_t s) {
            return launch_linear(M->A(e1), B, td, M->W(w2), M->W(b2), td, 1, M->A(e2), td, s);
        });
        bd.op("dense_table", [=](hipStream_t s) {
            return launch_linear(M->A(e2), B, td, M->W(M->wt->w_dense), M->W(M->wt->w_dense_b), M->wt->dense_rows, 0,
                                 M->A(table), M->wt->dense_rows, s);
        });
    }
    // ---- feature pack + input conv
    Tn in4 = bd.alloc(F, T, 4);
    {
        const size_t o = in4.off;
        bd.op("pack_input", [=](hipStream_t s) { return launch_pack_input(nullptr, nullptr, B, F, T, M->A(o), s, M->d_call); });
    }
    const Module& cin = next();
    std::vector<Tn> hs;
    {
        ConvReq r = conv_req("conv_in", in4, cin.w_a, nf, 9);
        r.bias = cin.w_a_b;
        hs.push_back(bd.conv(r));
    }
    Tn ipyr = in4;
    // ---- down path
    for (int lv = 0; lv < L; ++lv) {
        for (int b = 0; b < c.num_res_blocks; ++b) {
            Tn h = bd.resblock(next(), hs.back(), nullptr);
            if (in_list(c.attn_resolutions, c.num_attn, h.H)) {
                Tn h2 = bd.attn(next(), h);
                bd.release(h);
                h = h2;
            }
            hs.push_back(h);
        }
        if (lv != L - 1) {
            Tn h = bd.resblock(next(), hs.back(), nullptr);
            Tn ip2 = bd.fir(ipyr, false, nullptr, false, nullptr);
            bd.release(ipyr);
            ipyr = ip2;
            const Module& cb = next();
            h = bd.conv(combine_req(cb, ipyr, h));
            hs.push_back(h);           // (updated in place; its statistics are the Combine kernel's, or dropped)
        }
    }
    bd.release(ipyr);
    // ---- middle
    Tn h = bd.resblock(next(), hs.back(), nullptr);
    {
        Tn h2 = bd.attn(next(), h);
        bd.release(h);
        h = bd.resblock(next(), h2, nullptr);
        bd.release(h2);
    }
    // ---- up path
    Tn pyr;
    for (int lv = L - 1; lv >= 0; --lv) {
        for (int b = 0; b < c.num_res_blocks + 1; ++b) {
            Tn skip = hs.back();
            hs.pop_back();
            Tn h2 = bd.resblock(next(), h, &skip);
            bd.release(h);
            bd.release(skip);
            h = h2;
        }
        if (in_list(c.attn_resolutions, c.num_attn, h.H)) {
            Tn h2 = bd.attn(next(), h);
            bd.release(h);
            h = h2;
        }
        const Module& gnm = next();
        const Module& pcv = next();
        // 16-bit h: the dedicated 4-channel head kernel reads it directly; small images materialise act(GN(h)) in fp32
        // and run the fp32 kernels
        ConvReq rp = conv_req("pyramid_conv", h, pcv.w_a, 4, 9);
        rp.bias = pcv.w_a_b;
        const bool pfuse = bd.route(rp).gn_on_load;      // (asked without the GroupNorm; the request with it confirms)
        GnBuf g;
        if (pfuse) g = bd.gn(h, nullptr, gnm.w_a, gnm.w_a_b);
        Tn ph = pfuse ? h : bd.gn_norm(h, nullptr, gnm.w_a, gnm.w_a_b, true, DT_F32);
        rp.a = &ph;
        rp.gin = pfuse ? &g : nullptr;
        rp.gin_silu = true;
        if (!pyr.valid()) {
            pyr = bd.conv(rp);
        } else {
            Tn up = bd.fir(pyr, true, nullptr, false, nullptr);
            bd.release(pyr);
            rp.res = &up;                                // accumulated in place on the upsampled pyramid
            rp.out_is_res = true;
            pyr = bd.conv(rp);
        }
        if (pfuse) bd.gn_release(g);
        if (!pfuse) bd.release(ph);
        if (lv != 0) {
            Tn h2 = bd.resblock(next(), h, nullptr);
            bd.release(h);
            h = h2;
        }
    }
    bd.release(h);
    if (!hs.empty() || mi != m->wt->mods.size()) {
        set_error("internal: plan consumed %zu of %zu modules, %zu skips left", mi, m->wt->mods.size(), hs.size());
        return ERR_STATE;
    }
    // ---- head (+ solver update)
    {
        const size_t p = pyr.off;
        bd.op("head", [=](hipStream_t s) {
            return launch_head(M->A(p), nullptr, M->W(M->wt->w_out), M->W(M->wt->w_out_b), B, F, T, 0, nullptr, 0.f, nullptr, s,
                               M->d_call);
        });
    }
    plan->ws_bytes = bd.arena.peak();
    return bd.failed ? ERR_STATE : OK;
}

// Plan of a single-module handle: inputs are copied into the arena, the module runs exactly as inside the network
// (Builder::resblock / attn / conv), the result is copied out.
int build_block_plan(flowse_model* m, Plan* plan, int B, int H, int W, int C1) {
    const Module& mod = m->wt->mods[0];
    const bool combine = mod.kind == M_COMBINE;
    const int C2 = combine ? mod.out_ch : mod.in_ch - C1;
    if (B < 1 || H < 1 || W < 1 || C1 < 4 || (C1 & 3) || C2 < 0 || (C2 & 3) || (combine && C1 != 4) ||
        (mod.kind == M_ATTN && C2 != 0) || ((mod.up || mod.down) && C2 != 0) || (mod.down && ((H | W) & 1))) {
        set_error("flowse_block_forward: bad shape B=%d H=%d W=%d C1=%d for a module with in_ch=%d", B, H, W, C1,
                  mod.in_ch);
        return ERR_SHAPE;
    }
    plan->B = B; plan->F = H; plan->T = W;
    Builder bd(m, plan, B);
    flowse_model* M = m;
    const int td = m->wt->temb_dim;
    Tn x1 = bd.alloc(H, W, C1), x2;
    if (C2 > 0) x2 = bd.alloc(H, W, C2);
    {   // the caller's tensors are fp32; in a 16-bit storage mode they are rounded to the activation type on the way in
        const size_t o1 = x1.off, o2 = x2.off;
        const int64_t n1 = (int64_t)B * H * W * C1, n2 = C2 > 0 ? (int64_t)B * H * W * C2 : 0;
        const int d1 = x1.dt, d2 = x2.dt;
        bd.op("block_in", [=](hipStream_t s) {
            int rc = launch_convert(M->bcall.in1, DT_F32, M->A(o1), d1, n1, s);
            if (rc == OK && n2) rc = launch_convert(M->bcall.in2, DT_F32, M->A(o2), d2, n2, s);
            return rc;
        });
    }
    Tn out;
    if (mod.kind == M_RESBLOCK) {
        bd.M_table_off = bd.arena.alloc((size_t)B * m->wt->dense_rows * 4);
        const size_t table = bd.M_table_off;
        bd.op("dense_table", [=](hipStream_t s) {          // Dense_0(act(temb)) + Conv_0.bias (layerspp.py:262-263)
            return launch_linear(M->bcall.temb_act, B, td, M->W(M->wt->w_dense), M->W(M->wt->w_dense_b), M->wt->dense_rows, 0,
                                 M->A(table), M->wt->dense_rows, s);
        });
        out = bd.resblock(mod, x1, C2 > 0 ? &x2 : nullptr);
    } else if (mod.kind == M_ATTN) {
        out = bd.attn(mod, x1);
    } else {                                               // Combine: conv1x1(x) + y (layerspp.py:55-59)
        bd.conv(combine_req(mod, x1, x2));
        out = x2;
    }
    {
        const size_t o = out.off;
        const int64_t n = (int64_t)out.B * out.H * out.W * out.C;
        const int od = out.dt;
        bd.op("block_out", [=](hipStream_t s) { return launch_convert(M->A(o), od, M->bcall.out, DT_F32, n, s); });
    }
    plan->ws_bytes = bd.arena.peak();
    return bd.failed ? ERR_STATE : OK;
}

}  // namespace flowse
