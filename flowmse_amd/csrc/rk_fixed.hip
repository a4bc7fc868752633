// Fixed-step explicit Runge-Kutta samplers of the C ABI (include/flowse_hip.h): flowse_euler_sample, flowse_rk_sample and the
// multi-lane flowse_rk_sample_multi.  Host code only: every stage is one network evaluation of the handle's plan, whose
// head kernel does the solver update.  Reaches the handle through the functions model.h declares.  No kernels here.
#include <algorithm>

#include "model.h"

namespace flowse {

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

}  // namespace flowse

extern "C" {

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
    return on_handle_stream(m, stream, [&](hipStream_t s) {
        while (rc == OK && !run.done(grid)) rc = run.issue(grid, s, true);
        return rc;
    });
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

}  // extern "C"
