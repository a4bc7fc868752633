/*
 * flowse_hip.h -- C ABI of libflowse_hip.so: the MI355X (gfx950) implementation of the flowmse sampling
 * hot path (Euler ODE loop x NCSN++ vector field).
 *
 * Conventions
 *   - Every function returns an int status (0 = FLOWSE_OK); flowse_last_error() returns a thread-local,
 *     human readable message for the last non-zero status.  Nothing throws across the ABI.
 *   - All tensor arguments are RAW DEVICE POINTERS owned by the caller (e.g. torch.Tensor.data_ptr());
 *     weights and workspace are owned by the model handle.  Exception: arguments documented "host".
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls enqueue work and return;
 *     they never synchronise the device (flowse_model_load_weights and flowse_model_reserve may allocate).
 *     The NULL (legacy default) stream cannot be captured into a hipGraph, so with graph replay enabled (FLOWSE_GRAPH=1)
 *     and stream == NULL the model handle runs the call on an internal stream fenced by events against the NULL stream on
 *     both sides: the call is ordered after
 *     everything enqueued on the NULL stream before it, and later NULL-stream work is ordered after the call -- the same
 *     ordering a launch on the NULL stream itself would have had (PyTorch's default stream is the NULL stream).
 *   - One weight-owning handle per GPU per process; calls on one handle must be serialised by the caller (the
 *     reference is single-threaded, single-stream, torch.no_grad()).  Further handles on the same weights are views
 *     (flowse_model_view_create); a parent and its views are used from ONE host thread.
 *   - Boundary tensors follow the reference: complex64 interleaved (re, im), [B, 1, F, T] contiguous
 *     (flowmse/backbones/ncsnpp.py:402-403), F == image_size, T a multiple of 2^(levels-1) (pad_spec,
 *     flowmse/util/other.py:83-90); time t is float32 [B] in (0, 1].
 *   - Per-op entry points (flowse_op_*) use the library's internal activation layout NHWC float32
 *     [B][H][W][C]; they exist for unit parity tests and for callers that fuse their own graphs.
 *
 * The reference has no C ABI for this path except the pybind11 `upfirdn2d` operator
 * (flowmse/backbones/ncsnpp_utils/op/upfirdn2d.cpp:12-22); flowse_upfirdn2d() is its drop-in.  All other
 * entry points replace PyTorch module calls; each one cites the reference code it stands for.
 */
#ifndef FLOWSE_HIP_H
#define FLOWSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLOWSE_OK 0
#define FLOWSE_ERR_ARG 1
#define FLOWSE_ERR_HIP 2
#define FLOWSE_ERR_STATE 3
#define FLOWSE_ERR_SHAPE 4

#define FLOWSE_ABI_VERSION 3
#define FLOWSE_MAX_LEVELS 8
#define FLOWSE_MAX_ATTN 4

/* Constructor arguments of flowmse.backbones.ncsnpp.NCSNpp that shape the graph (ncsnpp.py:45-67).
 * The remaining constructor flags are fixed at the reference defaults (biggan blocks, FIR [1,3,3,1],
 * skip_rescale, output_skip / input_skip progressive branches, 'sum' combine, fourier embedding). */
typedef struct flowse_config {
    int32_t nf;                                /* 128 */
    int32_t num_levels;                        /* len(ch_mult) = 7 */
    int32_t ch_mult[FLOWSE_MAX_LEVELS];        /* (1,1,2,2,2,2,2) */
    int32_t num_res_blocks;                    /* 2 */
    int32_t num_attn;                          /* len(attn_resolutions) = 1 */
    int32_t attn_resolutions[FLOWSE_MAX_ATTN]; /* (16,) */
    int32_t image_size;                        /* 256 = number of frequency bins F */
} flowse_config;

typedef struct flowse_model flowse_model;      /* opaque */

int flowse_abi_version(void);
const char* flowse_last_error(void);
/* Number of visible HIP devices (0 on a CPU-only host; never fails). */
int flowse_device_count(void);

/* ---- model handle -------------------------------------------------------------------------------
 * flowse_model_create builds the module list of NCSNpp.__init__ (ncsnpp.py:97-245) and its parameter
 * table on the host only -- no device is touched, so it also works on a CPU-only machine. */
int flowse_model_create(const flowse_config* cfg, flowse_model** out);
void flowse_model_destroy(flowse_model* m);

/* ---- view handles: several handles on one set of weights ------------------------------------------------------
 * flowse_model_view_create makes a second full handle on the weights `parent` has loaded.  A view is a flowse_model for
 * every per-call entry point (flowse_vf_forward, flowse_rk_sample, flowse_euler_sample, flowse_rk45_sample,
 * flowse_rk_sample_multi, flowse_model_reserve, flowse_profile_*).  It SHARES with its parent every device buffer that is
 * derived from the weights (the packed blob, its 16-bit twin, the bf16 planes, the Winograd and fragment-order copies), the
 * host tables that index them, the precision mode and the device.  It OWNS its workspace, launch plans, time table, RK
 * and RK45 scratch, per-call argument block, internal stream and events, and profiler state -- so a view and its parent
 * can run on different streams at the same time.  Creating a view allocates the per-call argument block (< 4 KiB) and
 * nothing else, and launches nothing; workspace comes with the view's first call or flowse_model_reserve.
 * The weight set is reference-counted: flowse_model_destroy on the parent while views are alive frees what the parent
 * owns and keeps the weights until the last holder is destroyed.  A view of a view is a view of the same set.
 * Errors (every handle is left as it was): null argument -> FLOWSE_ERR_ARG; parent is a single-module handle ->
 * FLOWSE_ERR_ARG; parent has no weights loaded -> FLOWSE_ERR_STATE; the set's device is not current -> FLOWSE_ERR_STATE.
 * While a weight set has more than one holder, flowse_model_load_weights and a flowse_model_set_precision that would
 * CHANGE the mode return FLOWSE_ERR_STATE ("destroy the views first") on every handle of the set; on a view they always
 * do. */
int flowse_model_view_create(flowse_model* parent, flowse_model** out);
/* Device memory in bytes.  FLOWSE_BYTES_WEIGHTS: the weight set the handle refers to (every layout), the same number for
 * a parent and its views.  FLOWSE_BYTES_OWNED: what only this handle holds (workspace, time table, RK scratch, RK45
 * state, flow-matching loss scratch, per-call argument block).  0 for a null handle or an unknown `what`. */
#define FLOWSE_BYTES_WEIGHTS 0
#define FLOWSE_BYTES_OWNED 1
int64_t flowse_model_device_bytes(const flowse_model* m, int what);
/* Number of live handles that refer to the handle's weight set: 1 for a handle without views, 0 before weights are
 * loaded (or for a null handle). */
int flowse_model_weight_holders(const flowse_model* m);

/* ---- single-module handles (unit parity against the reference's modules) -------------------------------------
 * A handle that holds ONE module of the network behind the same weight packer, launch planner and kernels the full
 * model uses: FLOWSE_BLOCK_RESNET = ResnetBlockBigGANpp(in_ch, out_ch, up, down) (layerspp.py:212-274),
 * FLOWSE_BLOCK_ATTN = AttnBlockpp(channels = in_ch = out_ch) (layerspp.py:62-91), FLOWSE_BLOCK_COMBINE =
 * Combine(4 -> out_ch, 'sum') (layerspp.py:44-59).  The parameter table / canonical blob / flowse_model_load_weights
 * calls work as for a model handle, with the reference's module-local keys under "all_modules.0." (GroupNorm_0.weight,
 * Conv_0.weight, Dense_0.weight, NIN_0.W, ...).
 * flowse_block_forward: NHWC float32 device tensors.  RESNET: out = block(cat[in1, in2], temb) with in1 [B,H,W,C1],
 * in2 [B,H,W,in_ch-C1] or NULL (then C1 = in_ch); `temb_act` = SiLU(temb) [B][temb_dim] (the block applies Dense_0 to
 * it, layerspp.py:262-263); out [B,H',W',out_ch] (H' = 2H / H/2 for up / down).  ATTN: out = block(in1).
 * COMBINE: out = Conv_0(in1 [B,H,W,4]) + in2 [B,H,W,out_ch]. */
#define FLOWSE_BLOCK_RESNET 0
#define FLOWSE_BLOCK_ATTN 1
#define FLOWSE_BLOCK_COMBINE 2
int flowse_block_create(int kind, int in_ch, int out_ch, int up, int down, int temb_dim, flowse_model** out);
int flowse_block_forward(flowse_model* m, const float* in1, int C1, const float* in2, const float* temb_act, float* out,
                         int B, int H, int W, void* stream);

/* Parameter table in the order of NCSNpp.parameters() / state_dict() (the order torch_ema's shadow_params
 * use, flowmse/model.py:81-103): output_layer.{weight,bias}, then all_modules.{i}.*.  `name` receives the
 * reference state_dict key; shape[0..ndim) the reference shape; `offset` the element offset of the tensor in
 * the canonical weight blob (all tensors contiguous, reference layout, back to back in table order). */
int flowse_model_num_params(const flowse_model* m);
int flowse_model_num_modules(const flowse_model* m);
int64_t flowse_model_blob_numel(const flowse_model* m);
int flowse_model_param_info(const flowse_model* m, int index, char* name, int name_cap, int64_t shape[4],
                            int* ndim, int64_t* offset);

/* Upload weights.  `blob` is a HOST pointer to flowse_model_blob_numel() floats in canonical order.  The
 * library re-packs into its kernel-native layouts (channel-last conv weights, transposed NIN, fused q/k/v,
 * one stacked Dense_0 matrix) on the current HIP device. */
int flowse_model_load_weights(flowse_model* m, const float* blob, int64_t numel);

/* Precision mode (call BEFORE flowse_model_load_weights; a change drops the uploaded weights).
 * 0 (default): every operand, product and accumulation is fp32 (v_mfma_f32_32x32x2_f32), activations fp32.  3x3
 *   convolutions with Cin % 32 == 0 and Cout % 64 == 0 on images the LDS-halo kernels cover are evaluated in Winograd
 *   form on transformed fp32 operands: whole-K launches of >= 128 blocks of 16 x 16 pixels x 64 channels in the
 *   two-dimensional form F(4,3) vertical x F(2,3) horizontal (conv3x3_w2d_kernel: one third of the multiplies, 3.4e-7 ..
 *   8.8e-7 rel-L2 per layer against the fp64 convolution), the rest in F(4,3) along the vertical axis only
 *   (conv3x3_f43_kernel: half the multiplies, 4e-7 .. 2e-6); FLOWSE_W2D=0 keeps everything on the one-dimensional form,
 *   FLOWSE_NO_WINOGRAD=1 selects the direct form, whose result is bit for bit an fmaf chain.
 * 1 "bf16x3": fp32 activations; the operands of the big 3x3 convs are split x = hi + lo in bf16 and the products
 *   hi*hi + hi*lo + lo*hi accumulated in fp32 (fp32-class accuracy, ~1e-5 end to end).
 * 2 "bf16" (BASELINE config 3) / 3 "fp16" (BASELINE config 5): 16-bit STORAGE modes -- every wide activation tensor
 *   between kernels is bf16 / IEEE half, all matrix products run on the 16-bit matrix cores (a 16-bit twin of the packed
 *   weights is kept) -- including the attention core (16-bit q / k / v and P, v_mfma_f32_32x32x16, attention16_kernel)
 *   -- while accumulators, GroupNorm statistics, the softmax state (running max / sum), time-embedding tables, split-K
 *   slabs and the 4-channel pyramid tensors stay fp32.  Applies to networks whose wide channel counts are
 *   multiples of 32 (the released configuration); otherwise storage stays fp32 and only the operands of the 3x3 convs
 *   with Cout % 128 == 0 become 16-bit.
 * The boundary tensors (x, y, out: complex64; t: float32) are the same in every mode. */
int flowse_model_set_precision(flowse_model* m, int mode);

/* Optional: plan buffers for a shape ahead of time (otherwise done lazily by the first call).
 * `workspace_bytes` (may be NULL) receives the activation workspace size. */
int flowse_model_reserve(flowse_model* m, int B, int F, int T, int64_t* workspace_bytes);

/* ---- vector field --------------------------------------------------------------------------------
 * mode 0: out = dnn(cat[x, y], t)     == NCSNpp.forward          (ncsnpp.py:247-404)
 * mode 1: out = -dnn(cat[x, y], t)    == VFModel.forward(x,t,y)  (flowmse/model.py:164-170)
 * x, y, out: complex64 [B,1,F,T] device; t: float32 [B] device. */
int flowse_vf_forward(flowse_model* m, const void* x, const void* y, const float* t, void* out, int B, int F,
                      int T, int mode, void* stream);

/* ---- sampler --------------------------------------------------------------------------------------
 * x <- y + sigma * z                                            (FLOWMATCHING.prior_sampling, odes.py:93-100) */
int flowse_prior_sample(const void* y, const void* z, float sigma, void* x_out, int64_t numel_complex,
                        void* stream);
/* The same with z generated inside the kernel from a counter-based stream (no z tensor exists): row b of
 * y / x_out [B,1,F,T] complex64 gets the noise of utterance key keys_dev[b] (B 64-bit words in device memory) under
 * `seed`.  Philox4x32-10, counter (t >> 1, f, lo32(key), hi32(key)), key (lo32(seed), hi32(seed)); words (0, 1) give
 * the value at even t, words (2, 3) at odd t; u1 = ((w_a >> 9) + 0.5) 2^-23, u2 = (w_b >> 8) 2^-24,
 * z = sqrtf(-logf(u1)) (cospif(2 u2) + i sinpif(2 u2)), x = y + fl(z sigma) per part.  The value at (f, t) does not
 * depend on B, the row's position or T ("Keyed noise stream").  T must be even and the pointers
 * 16-byte aligned.  Enqueues only; no host synchronisation. */
int flowse_prior_sample_keyed(const void* y, const uint64_t* keys_dev, uint64_t seed, float sigma, void* x_out, int B,
                              int F, int T, void* stream);
/* The bare noise z [B,1,F,T] complex64 of the stream above. */
int flowse_op_keyed_noise(const uint64_t* keys_dev, uint64_t seed, void* z_out_c64, int B, int F, int T, void* stream);
/* The same two calls for rows that do not start at frame 0 of their utterance (the chunks of a long recording,
 * flowse_stft_compress_chunks): frame0_dev holds one int32 per row in device memory, the ABSOLUTE frame the row starts
 * at, and counter word 0 becomes (frame0[b] + t) >> 1 -- nothing else in the stream changes, so row b equals frames
 * frame0[b] .. frame0[b] + T - 1 of the offset-free stream of its key, bit for bit, and rows of one key that overlap
 * get the same noise where they do.  Each offset must be even (an odd one would pair the words of a frame differently),
 * >= 0 and <= INT32_MAX - T: the call copies the B offsets to the host and checks them BEFORE it launches, which
 * synchronises `stream` once -- unlike the offset-free calls it is not free of host synchronisation and cannot be
 * captured into a graph.  A bad offset returns FLOWSE_ERR_ARG and writes nothing. */
int flowse_prior_sample_keyed_at(const void* y, const uint64_t* keys_dev, const int32_t* frame0_dev, uint64_t seed,
                                 float sigma, void* x_out, int B, int F, int T, void* stream);
int flowse_op_keyed_noise_at(const uint64_t* keys_dev, const int32_t* frame0_dev, uint64_t seed, void* z_out_c64, int B,
                             int F, int T, void* stream);
/* N Euler steps in place on x (ode_solver loop, flowmse/sampling/__init__.py:45-57, with
 * EulerODEsolver.update_fn, sampling/odesolvers.py:42-47):  for i: x <- x + VF(x, ts[i], y) * (-dts[i]).
 * ts, dts: HOST float32 arrays of length N (the caller reproduces torch.linspace and the step rule, including
 * the final step dts[N-1] = ts[N-1]); they are consumed before the call returns (passed to the device as kernel
 * arguments, no asynchronous host copy).  No host synchronisation.  The launch list of a shape holds no per-call
 * argument; with FLOWSE_GRAPH=1 (read at flowse_model_create) it is captured on its second use and each network
 * evaluation becomes one hipGraph launch, counted by flowse_model_graph_launches().  The default is plain launches from
 * this C loop: measured on MI355X / ROCm 7.2 the replay is 5 % slower at [1,1,256,256] and equal at [8,1,256,256]. */
int flowse_euler_sample(flowse_model* m, void* x_inout, const void* y, const float* ts, const float* dts, int N,
                        int B, int F, int T, void* stream);
/* The same loop with a fixed-step explicit Runge-Kutta update per grid step (BASELINE config 5's "N = 25 RK solver").
 * The reference has no fixed-step RK -- its only Runge-Kutta is scipy's adaptive RK45 black box
 * (flowmse/sampling/__init__.py:64-114) -- so this is the reference's white-box loop (sampling/__init__.py:45-57, same
 * grid and step rule) with the update of an ODEsolverRegistry plugin (sampling/odesolvers.py:9-34) in place of
 * EulerODEsolver.update_fn.  tableau: FLOWSE_TABLEAU_EULER (== flowse_euler_sample), _HEUN (explicit trapezoid, 2
 * network evaluations per step) or _RK4 (classical, 4 per step).  A step that ends at t = 0 -- the last step of the
 * reference's grid -- is taken as the reference's Euler update: the field divides by t (ncsnpp.py:398) and embeds
 * log t, so no stage is ever evaluated at t <= 0.  Stages are chained through the head kernel (next stage input and
 * slope accumulation fused into it): no extra launches, no host synchronisation; each evaluation is the shape's launch
 * list issued as plain launches (default) or, under FLOWSE_GRAPH=1, one hipGraph launch. */
#define FLOWSE_TABLEAU_EULER 0
#define FLOWSE_TABLEAU_HEUN 1
#define FLOWSE_TABLEAU_RK4 2
int flowse_rk_sample(flowse_model* m, void* x_inout, const void* y, const float* ts, const float* dts, int N,
                     int tableau, int B, int F, int T, void* stream);
/* Several fixed-step solves in one call, on up to FLOWSE_MAX_LANES streams.  Item i is exactly what
 * flowse_rk_sample(handles[i], x_inout[i], y[i], ts, dts, N, tableau, B[i], F, T[i], .) computes -- bit for bit: every
 * item issues the same launches in the same order on one stream, every launch of the library is deterministic, and no
 * kernel waits on or accumulates into memory another launch owns.  One time grid for all items, one shape per item.
 * handles, x_inout, y, B, T: HOST arrays of length n_items (the x_inout[i] / y[i] are device pointers).
 * A LANE is a distinct handle (a parent and its views, flowse_model_view_create).  Items that name the same handle run
 * in array order on that lane's stream; items of different lanes may overlap on the GPU.  At most FLOWSE_MAX_LANES
 * distinct handles -- a process has 4 hardware queues by default, and the library does not change that -- all on the
 * device that is current.  The point is throughput at small batch (measured: 1.29x on four [1,1,256,256] items and
 * 1.31x on mixed lengths with two lanes); each item's own latency goes UP while the aggregate rate
 * rises.  The reading behind it -- launches of 128 blocks or fewer at the low-resolution levels leave room for another
 * lane, the large 3x3 launches hold every compute unit -- is an estimate from the per-op table, not a traced fact.
 * Streams: the lane of handles[0] runs on `stream` (NULL included), every other lane on its handle's internal
 * non-blocking stream.  On entry one event recorded on `stream` is waited for by every other lane; on exit `stream`
 * waits for one event per other lane, so whatever the caller enqueues on, or frees to, `stream` afterwards is ordered
 * behind all lanes.  No host synchronisation once the first launch is out: every plan is built and every lane's
 * workspace, time table and RK scratch are sized for the lane's largest item BEFORE the first launch (growth
 * synchronises the device, as in the single call).  Launches are enqueued round-robin over the lanes, one network
 * evaluation per turn.  This path always issues plain launches, also on FLOWSE_GRAPH=1 handles.
 * n_items == 1 is flowse_rk_sample on that item (graph replay included).
 * Errors: a null table or item pointer, n_items < 1, N < 1, an unknown tableau, a single-module handle, more than
 * FLOWSE_MAX_LANES distinct handles -> FLOWSE_ERR_ARG, checked before any device call; a handle with a profile open
 * (flowse_profile_begin) or without weights, or the wrong device current -> FLOWSE_ERR_STATE.  The call must NOT be
 * made while `stream` is being captured into a graph (hipStreamBeginCapture, torch.cuda.graph): the fences would pull
 * the other lanes into the capture as parallel branches, the graph this path exists to avoid; the library does not
 * check for it.  If a launch fails,
 * enqueuing stops, every lane is still joined into `stream`, and the first error is returned. */
#define FLOWSE_MAX_LANES 4
int flowse_rk_sample_multi(flowse_model* const* handles, int n_items, void* const* x_inout, const void* const* y,
                           const int* B, const int* T, int F, const float* ts, const float* dts, int N, int tableau,
                           void* stream);
/* Adaptive Dormand-Prince 5(4): the reference's black-box sampler (flowmse/sampling/__init__.py:64-114,
 * scipy.integrate.solve_ivp(ode_func, (t0, t_bound), x, method="RK45", rtol, atol)) with the state on the device.  The
 * controller is a line-by-line port of scipy 1.15's RungeKutta._step_impl / rk_step / select_initial_step and
 * OdeSolver.step, all scalars in double, and takes the same steps: y / y_new are complex128 as in scipy, the slopes
 * K1..K7 complex64 (network outputs), each network input complex64(stage state) as the reference's ode_func casts it,
 * and the stage combinations repeat numpy's operation order (only the RMS norm's summation order differs, ~1e-16
 * relative; it is a fixed partition and order, so two identical solves are bitwise identical).
 * x_inout: complex64 [B,1,F,T], start state in, complex64(y at the last accepted time) out.  The batch is ONE ODE
 * system with one error norm, as in the reference.  first_step <= 0: scipy's select_initial_step, else the given
 * first step (0 < first_step <= |t_bound - t0|); max_step may be +inf.  nfev_out counts network evaluations as scipy's
 * nfev does (1 for f0, 1 for the initial-step probe unless first_step is given, 6 per attempted step); status_out 0 =
 * finished at t_bound, -1 = step size fell below scipy's minimum (scipy's status -1; x holds the last accepted state),
 * -2 = the next attempted step would exceed max_nfev (a fail-fast cap scipy does not have).  t_accepted (may be NULL
 * when t_cap == 0) receives the first t_cap accepted times (scipy's solution.t[1:]); n_accepted the number of them.
 * Each evaluation is the shape's launch list with VF = -dnn (flowse_vf_forward mode 1; plain launches or, under
 * FLOWSE_GRAPH=1, one hipGraph launch), its time ones(B) * t passed by value.  Synchronisation: unlike the samplers
 * above this call is NOT free of host synchronisation -- the step controller reads one 8-byte error norm back per
 * attempted step (and one per norm of select_initial_step: three), waiting on the stream each time.  The work
 * buffers (2 x complex128 + 8 x complex64 per element) are allocated per handle on first use; growing them
 * synchronises the device once. */
int flowse_rk45_sample(flowse_model* m, void* x_inout, const void* y, double t0, double t_bound, double rtol,
                       double atol, double first_step, double max_step, int64_t max_nfev, int B, int F, int T,
                       int64_t* nfev_out, int* status_out, double* t_accepted, int t_cap, int* n_accepted,
                       void* stream);
/* Number of hipGraphLaunch calls this handle has issued so far (0 while every evaluation ran as plain launches). */
int64_t flowse_model_graph_launches(const flowse_model* m);
/* One generic explicit update from a caller-held slope: x <- x + dt * k (complex64 as float pairs). */
int flowse_axpy(const void* x, const void* k, float dt, void* out, int64_t numel_complex, void* stream);

/* ---- spectrogram transforms either side of the sampler -------------------------------------
 * flowse_stft_compress: sig float32 [B][L] -> complex64 [B,1,256,Tpad].  Equals pad_spec(spec_fwd(stft(sig * scale_in)))
 * of the reference (data_module.py:149-162,199-201; util/other.py:83-90) for n_fft 510, hop 128, periodic hann,
 * center=True (reflect): T = L / 128 + 1 frames, frames T..Tpad-1 are zero.  spec_fwd = factor * |z|^exponent *
 * exp(j arg z) (transform_type "exponent"; exponent 1 = plain scaling).
 * flowse_istft_decompress: the inverse chain istft(spec_back(spec), length = Lout) * scale_out
 * (data_module.py:164-175,203-205; model.py:190-191) over frames 0..T-1 of a spectrogram whose frame pitch is Tpad.
 * The reference runs the iSTFT over ALL frames of the padded sample (model.py:190-191, evaluate.py:132), i.e.
 * T == Tpad there: the zero-padded frames are no longer zero after enhancement and reach the last ~127 samples. */
int flowse_stft_compress(const float* sig, int B, int L, float scale_in, void* out_c64, int T, int Tpad, float factor,
                         float exponent, void* stream);
int flowse_istft_decompress(const void* spec_c64, int B, int T, int Tpad, float factor, float exponent, float* out,
                            int Lout, float scale_out, void* stream);
/* ---- one recording as overlapping chunks (opt-in; NOT the reference's computation for a long file) ----------
 * A recording of L samples has T = L / 128 + 1 frames.  It is held as K chunks of Tc frames that start `hop` frames apart:
 * chunk k covers the recording's frames [k hop, k hop + Tc), the last To = Tc - hop of which it shares with chunk k + 1;
 * Tg = (K - 1) hop + Tc frames in all.  Geometry accepted by both calls: 1 <= hop <= Tc <= 2 hop (at most two chunks over
 * any frame), 1 <= K <= 65535, Tg <= 2^23; anything else returns FLOWSE_ERR_SHAPE and launches nothing.
 * flowse_stft_compress_chunks: sig float32 [L] -> complex64 [K,1,256,Tc], the rows an ordinary [K,1,256,Tc] sampler call
 * takes.  Frame t of chunk k is frame k hop + t of flowse_stft_compress(sig, B = 1), computed by the same kernel with the
 * same arithmetic (bit-identical; frames >= T are zero, like pad_spec's); shared frames are computed twice -- there is no
 * global spectrogram and no gather pass.  Needs Tg >= T (every frame of the recording lies in a chunk) and L > 255.
 * flowse_istft_decompress_chunks: the inverse chain of flowse_istft_decompress over the Tg frames of the recording,
 * where frame t is taken from the chunks by the seam rule: k = min(t / hop, K - 1), j = t - k hop; for k > 0 and j < To
 * the linear cross-fade a + w (b - a) of a = chunk k-1 at frame j + hop and b = chunk k at frame j with
 * w = (j + 0.5) / To, evaluated in fp32 on the COMPRESSED complex value (before spec_back); otherwise chunk k at frame j.
 * All Tg frames take part in the overlap-add, as all Tpad frames do in flowse_istft_decompress.  Chunks cut from one
 * spectrogram give that spectrogram's waveform bit for bit (b - a is an exact zero there).  out: float32 [Lout],
 * 1 <= Lout <= 128 (Tg - 1) + 255. */
int flowse_stft_compress_chunks(const float* sig, int L, float scale_in, void* out_c64, int K, int Tc, int hop, float factor,
                                float exponent, void* stream);
int flowse_istft_decompress_chunks(const void* chunks_c64, int K, int Tc, int hop, float factor, float exponent, float* out,
                                   int Lout, float scale_out, void* stream);

/* ---- rows and stacks from many recordings (opt-in: flowmse_amd.pooled, `enhance --pool`) ----------------------
 * The two chunk calls above for sampler calls whose rows come from SEVERAL recordings (or channels of one file).
 * flowse_stft_compress_rows: the R input rows [R,1,256,Tw] of ONE sampler call in one launch.  `rows` is a HOST table of R
 * descriptors; row r holds frames [frame0, frame0 + Tw) of flowse_stft_compress(sig_r, B = 1, L_r, scale_in_r), computed by
 * the same per-frame code as the calls above (bit-identical to the matching row of flowse_stft_compress_chunks; frames
 * >= L_r / 128 + 1 are zero).  Two rows may name the same signal.  The table is copied into the kernel's argument block
 * (FLOWSE_MAX_SPEC_ROWS x 24 bytes): the call does not allocate, upload or synchronise, and the caller may reuse the table
 * as soon as it returns.  R outside 1..FLOWSE_MAX_SPEC_ROWS, L_r <= 255, Tw < 1, frame0 + Tw > 2^23 -> FLOWSE_ERR_SHAPE;
 * a null table, output or sig_r, frame0 < 0 -> FLOWSE_ERR_ARG; nothing is launched and the output is left untouched.
 * flowse_istft_decompress_stacks: flowse_istft_decompress_chunks for S stacks of equal geometry in one launch:
 * chunks_c64 [S*K,1,256,Tc], rows ordered (stack, chunk) -> out float32 [S][Lout], row s bit-identical to
 * flowse_istft_decompress_chunks on stack s.  1 <= S <= 65535; the other checks are those of the chunk call. */
#define FLOWSE_MAX_SPEC_ROWS 64
typedef struct flowse_spec_row {
    const float* sig;                          /* device, float32 [L] */
    int32_t L;                                 /* samples, > 255 */
    int32_t frame0;                            /* first frame of the row, >= 0 */
    float scale_in;                            /* the signal is multiplied by this (1 / its file's peak) */
} flowse_spec_row;
int flowse_stft_compress_rows(const flowse_spec_row* rows, int R, int Tw, void* out_c64, float factor, float exponent,
                              void* stream);
int flowse_istft_decompress_stacks(const void* chunks_c64, int S, int K, int Tc, int hop, float factor, float exponent,
                                   float* out, int Lout, float scale_out, void* stream);

/* ---- windows of a recording that is still arriving (opt-in: flowmse_amd.live, `enhance --live`) ------------------
 * The chunk calls above on what a live session holds: a window of the samples and the last chunks it sampled.  Stateless;
 * all sample, frame and chunk indices are 64-bit.  Both calls only enqueue on `stream`; they allocate nothing and do not
 * synchronise.  Null buf / out_c64 / cur_c64 / out -> FLOWSE_ERR_ARG; every FLOWSE_ERR_SHAPE below is answered before any
 * launch, with the values in flowse_last_error(), and leaves the output untouched.
 * flowse_stft_compress_window: buf float32 [n] holds samples [s0, s0 + n) of the recording -> the ONE row complex64
 * [1,1,256,Tc] of frames [frame0, frame0 + Tc), computed by the per-frame code of the calls above: with frame0 = k hop it is
 * row k of flowse_stft_compress_chunks on the whole recording, bit for bit.  L_total = -1 while the recording is open: no
 * right reflection, no zero frames.  L_total >= 0 (> 255, >= s0 + n) once it has ended: frames >= L_total / 128 + 1 are
 * zero and the frames over the end reflect about sample L_total - 1, as in every other call.  A sample index a frame needs
 * that lies outside the window -> FLOWSE_ERR_SHAPE: the reflection about sample 0 (frames 0 and 1) needs s0 == 0, an open
 * recording needs 128 (frame0 + Tc - 1) + 254 < s0 + n.
 * flowse_istft_decompress_window: the output samples [e0, e0 + n_out) of flowse_istft_decompress_chunks on the whole stack,
 * bit for bit, from the chunks k-2 (prev2_c64), k-1 (prev_c64) and k (cur_c64), each complex64 [1,256,Tc]; a chunk the range
 * does not read may be null.  last != 0: chunk k is the recording's last (K = k + 1, Tg = k hop + Tc) and L its length,
 * e0 + n_out <= L <= 128 (Tg - 1) + 255; last == 0: L is not read, and frames from (k + 1) hop on are not final (they wait
 * for chunk k + 1).  The samples [128 k hop - 255, 128 (k + 1) hop - 255) that become final with chunk k lie under frames
 * from k hop - 3 on; the seam rule takes those from chunks k - 1 and k when Tc - 2 To >= 3, and from chunk k - 2 as well
 * when To = Tc / 2 (frames k hop - 3 .. k hop - 1 are then blended frames of chunk k - 1).  A range under a frame that needs
 * a chunk other than those given -> FLOWSE_ERR_SHAPE.  1 <= hop <= Tc <= 2 hop, k <= 2^40, 1 <= n_out <= 2^30. */
int flowse_stft_compress_window(const float* buf, int64_t s0, int64_t n, float scale_in, int64_t frame0, int Tc,
                                int64_t L_total, void* out_c64, float factor, float exponent, void* stream);
int flowse_istft_decompress_window(const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k, int Tc,
                                   int hop, int last, int64_t L, float factor, float exponent, float* out, int64_t e0,
                                   int64_t n_out, float scale_out, void* stream);

/* ---- the windows of several live sessions in one launch each (opt-in: flowmse_amd.livepool, `--live --live_channels C`) --
 * The two window calls above for sampler calls whose rows come from SEVERAL sessions and channels.  `rows` is a HOST table
 * of R descriptors, each the arguments of the single-window call; it is copied into the kernel's argument block, so the
 * calls do not allocate, upload or synchronise, and the caller may reuse the table as soon as they return.
 * flowse_stft_compress_window_rows: the R input rows complex64 [R,1,256,Tw] of ONE sampler call; row r is, bit for bit, what
 * flowse_stft_compress_window(buf, s0, n, scale_in, frame0, Tw, L_total, ...) writes (the same per-frame code).  Two rows
 * may name one buffer.
 * flowse_istft_decompress_window_rows: R output ranges of one geometry (Tc, hop); range r is, bit for bit, what
 * flowse_istft_decompress_window(prev2_c64, prev_c64, cur_c64, k, Tc, hop, last, L, ..., out, e0, n_out, scale_out) writes.
 * The ranges may have different lengths (the grid covers the longest; the blocks past a row's range store nothing), and
 * every row's own k, last, L, e0 and n_out decide its frames and chunks.  The ranges must not overlap in memory.
 * Every row passes the checks of the single-window call, all rows before any launch: the first row that fails answers
 * FLOWSE_ERR_ARG (a null buf, cur_c64 or out) or FLOWSE_ERR_SHAPE with its index and values in flowse_last_error(), and
 * every output is left untouched.  A null table or out_c64 -> FLOWSE_ERR_ARG; R outside 1..FLOWSE_MAX_WINDOW_ROWS ->
 * FLOWSE_ERR_SHAPE. */
#define FLOWSE_MAX_WINDOW_ROWS 16
typedef struct flowse_window_row {             /* one input row: the arguments of flowse_stft_compress_window */
    const float* buf;                          /* device, float32 [n]: samples [s0, s0 + n) of the recording */
    int64_t s0, n, frame0, L_total;            /* L_total = -1 while the recording is open */
    float scale_in;
} flowse_window_row;
typedef struct flowse_window_out {             /* one output range: the arguments of flowse_istft_decompress_window */
    const void *prev2_c64, *prev_c64, *cur_c64;    /* device, complex64 [1,256,Tc]; a chunk the range does not read may be null */
    float* out;                                /* device, float32 [n_out] */
    int64_t k, L, e0, n_out;
    int32_t last;
    float scale_out;
} flowse_window_out;
int flowse_stft_compress_window_rows(const flowse_window_row* rows, int R, int Tw, void* out_c64, float factor,
                                     float exponent, void* stream);
int flowse_istft_decompress_window_rows(const flowse_window_out* rows, int R, int Tc, int hop, float factor, float exponent,
                                        void* stream);

/* ---- trailing chunks (opt-in: flowmse_amd.chunked.enhance_trailing, `enhance --hop_frames H`; NOT the reference's
 * computation) -------------------------------------------------------------------------------------------------------
 * A non-causal network on a stream with a latency set by a small hop: chunks of Tc frames (a multiple of 64) slide by H
 * frames (even, 4 <= H <= Tc); the older P = Tc - H frames of a chunk are context only.  Chunk k holds the recording's
 * frames [k H - P, k H + H); frames < 0 (the first chunks are right-aligned against zero frames before the recording) and
 * frames >= T = L / 128 + 1 are zero.  K chunks make Tg = K H >= T frames.  Seam rule, with a cross-fade of X frames
 * (0 <= X <= H, H + X <= Tc): frame t belongs to chunk k = min((t + X) / H, K - 1) at j = t - k H + P; for k > 0 and
 * t < k H its value is a + w (b - a), a = chunk k - 1 at j + H, b = chunk k at j, w = (t - (k H - X) + 0.5) / X, taken on
 * the compressed value before spec_back; otherwise chunk k at j (chunked.blend_trailing_reference states it in float64).
 * All four calls only enqueue on `stream`, allocate nothing and do not synchronise.  Null pointers -> FLOWSE_ERR_ARG; a
 * geometry outside the above, and every FLOWSE_ERR_SHAPE below, is answered before any launch with the entry's name and
 * the values in flowse_last_error(), and leaves the output untouched.
 * flowse_stft_compress_trailing: the K rows complex64 [K,1,256,Tc] of ONE recording sig float32 [L] in one launch, by the
 * per-frame code of flowse_stft_compress_chunks: every frame 0 <= t < T is frame t of flowse_stft_compress(sig, B = 1) bit
 * for bit.  L > 255, 1 <= K <= 65535, T <= K H <= 2^23 - Tc.
 * flowse_istft_decompress_trailing: seam rule + spec_back + inverse STFT + rescale in one launch: chunks_c64
 * [K,1,256,Tc] -> out float32 [Lout], 1 <= Lout <= 128 (Tg - 1) + 255.  All Tg frames take part in the overlap-add, as in
 * flowse_istft_decompress_chunks, and the per-sample code is the same: chunks cut from one spectrogram [1,1,256,Tg] give
 * flowse_istft_decompress of it bit for bit.  An output sample reads at most 4 frames from at most 2 chunks.
 * flowse_stft_compress_trailing_window: row k alone, complex64 [1,1,256,Tc], from buf float32 [n] = samples [s0, s0 + n)
 * of the recording; bit for bit row k of flowse_stft_compress_trailing on the whole recording.  L_total = -1 while the
 * recording is open (no right reflection, no zero frames past the end), else its length (> 255, >= s0 + n).  The window
 * must hold every sample the frames [max(k H - P, 0), min(k H + H, T)) read (flowse_stft_compress_window has the rules);
 * (k + 1) H <= 2^40.
 * flowse_istft_decompress_trailing_window: the output samples [e0, e0 + n_out) of flowse_istft_decompress_trailing on the
 * whole stack, bit for bit, from the chunks k-2 (prev2_c64), k-1 (prev_c64) and k (cur_c64), each complex64 [1,256,Tc]; a
 * chunk the range does not read may be null.  last != 0: chunk k is the last (K = k + 1) and L the recording's length,
 * e0 + n_out <= L <= 128 (Tg - 1) + 255; last == 0: L is not read, and frames from (k + 1) H - X on are not final.  The
 * samples [128 (k H - X) - 255, 128 ((k + 1) H - X) - 255) that become final with chunk k lie under frames from
 * k H - X - 3 on: chunks k - 1 and k when H - X >= 3, chunk k - 2 as well otherwise.  A range under a frame that needs a
 * chunk other than those given -> FLOWSE_ERR_SHAPE.  1 <= n_out <= 2^30, (k + 1) H <= 2^40.  All sample, frame and chunk
 * indices of the two window calls are 64-bit; both are stateless. */
int flowse_stft_compress_trailing(const float* sig, int L, float scale_in, void* out_c64, int K, int Tc, int H, float factor,
                                  float exponent, void* stream);
int flowse_istft_decompress_trailing(const void* chunks_c64, int K, int Tc, int H, int X, float factor, float exponent,
                                     float* out, int Lout, float scale_out, void* stream);
int flowse_stft_compress_trailing_window(const float* buf, int64_t s0, int64_t n, float scale_in, int64_t k, int Tc, int H,
                                         int64_t L_total, void* out_c64, float factor, float exponent, void* stream);
int flowse_istft_decompress_trailing_window(const void* prev2_c64, const void* prev_c64, const void* cur_c64, int64_t k, int Tc,
                                            int H, int X, int last, int64_t L, float factor, float exponent, float* out,
                                            int64_t e0, int64_t n_out, float scale_out, void* stream);

/* ---- ensembles of draws (opt-in: flowmse_amd.ensemble, `--samples D`; NOT the reference's computation, which draws once)
 * flowse_istft_decompress_ensemble: flowse_istft_decompress_stacks over D draws per stack.  Chunk k of draw d of stack s is
 * row s * stack_stride + d * draw_stride + k of chunks_c64 (rows of 256 * Tc complex64 values; offsets in 64 bits).  The
 * linear spectrum of a draw is Z_d = spec_back(seam rule on the draw's compressed rows): the blend is done per draw, before
 * the decompression.  The call transforms the mean M = (1 / D) sum_d Z_d, summed in fp32 in the order d = 0 .. D - 1:
 *   out [S][Lout] = istft(M, Lout) * scale_out, over all Tg frames, formed by the code of the stacks call; D = 1 with
 *   stack_stride = K gives that call's output bit for bit (z * 1 is exact).
 *   tracks (may be null; must be null for D = 1): float32 [S][2][Tg], for every frame t of the Tg
 *     tracks[s][0][t] = dev[t] = sum_f sum_d |Z_d[f,t] - M[f,t]|^2 / (D - 1)      (256 bins)
 *     tracks[s][1][t] = pow[t] = sum_f |M[f,t]|^2
 *   The deviations are taken from the finished mean in a second pass over the draws (never sum |Z_d|^2 - D |M|^2), each
 *   sum in a fixed order without atomics: two calls give the same bits.
 * Two layouts in one signature: stacks [S][D][K] have stack_stride = D K, draw_stride = K; rows ordered (draw, stack) with
 * K = 1 have stack_stride = 1, draw_stride = S.  D outside 1..FLOWSE_MAX_DRAWS, tracks given at D = 1, negative strides,
 * strides under which two of the S D K rows coincide, or the shape errors of the stacks call -> FLOWSE_ERR_SHAPE with the
 * values in flowse_last_error(); null chunks or out -> FLOWSE_ERR_ARG; either is answered before any device call.  The call
 * allocates nothing and does not synchronise. */
#define FLOWSE_MAX_DRAWS 64
int flowse_istft_decompress_ensemble(const void* chunks_c64, int S, int D, int K, int Tc, int hop, int64_t stack_stride,
                                     int64_t draw_stride, float factor, float exponent, float* out, int Lout,
                                     float scale_out, float* tracks, void* stream);

/* ---- sample-rate conversion ahead of the STFT and after the iSTFT (opt-in; the reference reads 16 kHz files only) ----
 * Rational-ratio polyphase FIR resampling, zero phase, defined as what scipy.signal.resample_poly(x, up, down) computes
 * with its defaults (window ("kaiser", 5.0), padtype "constant"):
 *   g = gcd(up, down), up /= g, down /= g, R = max(up, down), half = 10 R
 *   h[k]  = up * firwin(2 half + 1, 1 / R, window = ("kaiser", 5.0))[k],  k = 0 .. 2 half
 *   L_out = ceil(L up / down)
 *   out[n] = sum over m in [0, L) with |n down - m up| <= half of  x[m] h[half + n down - m up]
 * Every entry takes a reduced or an unreduced pair (sr_out, sr_in will do) and reduces it itself.  Ratios with R > 1024
 * after reduction return FLOWSE_ERR_SHAPE; 8 / 11.025 / 12 / 22.05 / 24 / 32 / 44.1 / 48 / 88.2 / 96 / 176.4 / 192 kHz
 * against 16 kHz are within it, both ways (largest table: 20481 taps).
 * Host only, no GPU call, usable without a device:
 *   flowse_resample_num_taps: 2 half + 1, or -FLOWSE_ERR_ARG (a rate < 1) / -FLOWSE_ERR_SHAPE (R > 1024).
 *   flowse_resample_taps: h[0 .. 2 half] in double into `taps` (a HOST buffer of `cap` doubles): the windowed sinc with the
 *   Kaiser window's I0 by its power series, normalised to unit gain at DC as firwin does, times up (within 1e-12 of
 *   scipy's).  cap < 2 half + 1 or a null buffer -> FLOWSE_ERR_ARG.
 * flowse_resample_poly: B rows of L float32 samples (device, [B][L]), each on its own, into rows of L_out samples
 * (device, [B][L_out]); L_out != ceil(L up / down) or B > 65535 -> FLOWSE_ERR_SHAPE, a null pointer or B, L < 1 ->
 * FLOWSE_ERR_ARG, all checked before anything is launched.  One launch: with P = ceil((2 half + 1) / up) and the table
 * H[p][j] = fp32(h[p + j up]) (zero past 2 half), c = half + n down, p = c mod up, q = c div up,
 *   out[n] = fmaf chain over j = 0 .. P-1 of H[p][j] x[q - j],  x zero outside [0, L),
 * c and q in 64 bits (n down passes 2^31 five minutes into a 44.1 kHz recording).  up == down is a device copy.  The table
 * of a reduced ratio is built once per process and device and uploaded on the stream of the first call that needs it (that
 * call allocates; later calls on other streams wait for the upload by event).  Enqueues only, no host synchronisation --
 * but for the first call of a ratio on a device: it designs the taps on the host, allocates, and copies the table from
 * pageable memory, which the runtime may wait for, and it records an event, so make it outside stream capture (one short
 * call per ratio warms the cache).  Every later call for that ratio may be captured.
 * flowse_resample_poly_window: the outputs [n0, n0 + n_out) of ONE row from a window of it, for a signal that is still
 * arriving or too long to hold: win (device, float32 [n_win]) holds the samples [m0, m0 + n_win), out (device, float32
 * [n_out]) receives out[n0 ..], each bit for bit what flowse_resample_poly writes at that index for the whole signal (one
 * tap loop serves both kernels).  L_total is the row's length once it is known (the signal is closed: x is zero at and
 * past L_total) and -1 while it is open.  m0, n0, c, q and every sample index are 64-bit on the host and on the device.
 * Checked before anything is launched, with the numbers in flowse_last_error(), the output untouched:
 *   a null pointer, a negative m0, n_win, n0 or n_out, L_total < -1 -> FLOWSE_ERR_ARG; the ratio as in every entry;
 *   m0, n_win, n0 or L_total > 2^50, n_out > 2^31 - 1 -> FLOWSE_ERR_SHAPE;
 *   closed: m0 + n_win > L_total or n0 + n_out > ceil(L_total up / down) -> FLOWSE_ERR_SHAPE;
 *   open: an output with q >= m0 + n_win (it reads a sample that has not arrived) -> FLOWSE_ERR_SHAPE;
 *   the samples the outputs read, [q(n0) - (P - 1), q(n0 + n_out - 1)] clamped to the signal -- all P taps of every
 *   output, the zero table entries past 2 half included -- not inside the window -> FLOWSE_ERR_SHAPE.
 * n_out == 0 returns FLOWSE_OK and launches nothing.  up == down copies the samples [n0, n0 + n_out) out of the window
 * (which must hold them).  One launch, in the same four forms and under the same test as flowse_resample_poly; the table
 * is that call's: the first call for a ratio on a device (through either entry) uploads it and must not be made under
 * stream capture, every later one enqueues only.
 * flowse_resample_poly_window_rows: the window call above for R rows at ONE ratio in one launch (flowmse_amd.resample.flush,
 * flowmse_amd.livepool): the channels of a session, the sessions of a pool.  `rows` is a HOST table of R descriptors, each
 * the arguments of the single-window call; it is copied into the kernel's argument block, so the call does not allocate,
 * upload or synchronise (but for the ratio's table, as above), and the caller may reuse the table as soon as it returns.
 * Row r receives, bit for bit, what flowse_resample_poly_window(win, m0, n_win, L_total, up, down, out, n0, n_out) writes:
 * one device function is the body of both kernels, in the same four forms under the same test.  The grid is
 * (ceil(largest n_out / run), R): a block past its row's n_out returns at once, and a row with n_out == 0 is legal and is
 * skipped.  Two rows may name one window; the output ranges must not overlap in memory.  Every row passes the checks of the
 * single-window call, all rows before anything is enqueued: the first row that fails answers FLOWSE_ERR_ARG (a null win
 * or out, a negative count) or FLOWSE_ERR_SHAPE with `row %d` and its values in flowse_last_error(), and every output is
 * left untouched.  A null table -> FLOWSE_ERR_ARG; R outside 1..FLOWSE_MAX_RESAMPLE_ROWS -> FLOWSE_ERR_SHAPE.  up == down
 * copies per row, as the single call does.  All n_out == 0 returns FLOWSE_OK and launches nothing. */
#define FLOWSE_MAX_RESAMPLE_ROWS 32
typedef struct flowse_resample_row {           /* one row: the arguments of flowse_resample_poly_window */
    const float* win;                          /* device, float32 [n_win]: samples [m0, m0 + n_win) of this row's signal */
    int64_t m0, n_win, L_total;                /* L_total = -1 while the signal is open */
    float* out;                                /* device, float32 [n_out]: outputs [n0, n0 + n_out) */
    int64_t n0, n_out;
} flowse_resample_row;
int flowse_resample_poly_window_rows(const flowse_resample_row* rows, int R, int up, int down, void* stream);
int flowse_resample_num_taps(int up, int down);
int flowse_resample_taps(int up, int down, double* taps, int cap);
int flowse_resample_poly(const float* sig, int B, int L, int up, int down, float* out, int L_out, void* stream);
int flowse_resample_poly_window(const float* win, int64_t m0, int64_t n_win, int64_t L_total, int up, int down, float* out,
                                int64_t n0, int64_t n_out, void* stream);

/* ---- evaluation metrics on the device: ESTOI and SI-SDR / SI-SIR / SI-SAR (opt-in: evaluate --metrics device) ----
 * ESTOI is DEFINED here, step by step after pystoi.stoi(x, y, 16000, extended=True) (pystoi 0.3 / 0.4); the package is
 * not available where this library is built and tested, so equality with it has NOT been checked -- the float64
 * restatement flowmse_amd.metrics.estoi_reference is what the kernels are held to.  All arithmetic float64; inputs are
 * float32 waveforms at 16 kHz of equal length L (clean x, processed y); EPS = 2^-52.
 *   1. 10 kHz: fc = 1/16, t = -290 .. 290, h[t] = kaiser(581, 0.1102 (60 - 8.7))[t] 2 5 fc sinc(2 fc t), h /= sum h;
 *      x10 = scipy.signal.resample_poly(x, 5, 8, window = h): x10[n] = sum_m x[m] 5 h[290 + 8 n - 5 m], L10 = ceil(5 L / 8).
 *   2. w = hanning(258)[1:-1]; first-pass frames start at 128 i < L10 - 256 (f0 = ceil((L10 - 256) / 128) of them);
 *      e[i] = 20 log10(|w x10[128 i : 128 i + 256]| + EPS) on the CLEAN signal; frame i is kept iff max(e) - 40 - e[i] < 0;
 *      both signals are rebuilt by overlap-adding their K kept windowed frames at hop 128.
 *   3. The rebuilt signals are framed the same way (K - 1 frames, w again), 512-point DFT, 15 third-octave bands with bin
 *      ranges [7,9) [9,11) [11,14) [14,17) [17,22) [22,27) [27,34) [34,43) [43,55) [55,69) [69,87) [87,109) [109,138)
 *      [138,174) [174,219): X_tob[b][j] = sqrt(sum over the band of |X[k][j]|^2).
 *   4. K - 1 < 30 or L10 <= 256: the result is 1e-5.
 *   5. Segments m = 30 .. K - 1 take columns [m - 30, m) of both band matrices (15 x 30); each is normalised: row mean
 *      over time subtracted, rows divided by (|row| + EPS), column mean over bands subtracted, columns divided by
 *      (|col| + EPS); d = sum(x_n y_n) / 30 / (number of segments).
 * The kept count K is decided on the device: later grids are sized for f0 frames, and blocks past K leave.  No
 * floating-point atomics: the same input gives the same bits.
 * Energy ratios (reference utils.py:26-35) in float64 with n = noisy - clean, two passes: <est,s>, <s,s>, <est,n>, <n,n>
 * give a_s and a_n; then |est - a_s s|^2, |a_n n|^2, |est - a_s s - a_n n|^2 element by element; out3 = SI-SDR, SI-SIR,
 * SI-SAR in dB.
 *   flowse_estoi_num_taps: 581.  flowse_estoi_taps: h of step 1 (sum 1; the resampler applies 5 h) in double into a HOST
 *   buffer of `cap` doubles; host only, no device needed; cap < 581 or a null buffer -> FLOWSE_ERR_ARG.
 *   flowse_metrics_workspace_bytes: bytes of device workspace either call needs for length L (one workspace serves both,
 *   and any shorter L); -FLOWSE_ERR_ARG for L < 1 or L > 2^24.
 *   flowse_estoi / flowse_energy_ratios: signals, workspace and out (1 / 3 doubles) are DEVICE memory owned by the caller.
 *   L < 1, L > 2^24, a null pointer or workspace_bytes below flowse_metrics_workspace_bytes(L) -> FLOWSE_ERR_ARG with a
 *   message, nothing launched.  The calls enqueue on `stream`, allocate nothing and never synchronise -- but for the first
 *   flowse_estoi on a device, which builds the tap / window / twiddle table on the host, allocates it and copies it from
 *   pageable memory (the runtime may wait for that) and records an event: make that call outside stream capture.  Calls
 *   that share a workspace must be ordered by the caller (one stream, or events). */
int flowse_estoi_num_taps(void);
int flowse_estoi_taps(double* taps, int cap);
int64_t flowse_metrics_workspace_bytes(int L);
int flowse_estoi(const float* clean, const float* proc, int L, void* workspace, int64_t workspace_bytes, double* out,
                 void* stream);
int flowse_energy_ratios(const float* est, const float* clean, const float* noisy, int L, void* workspace,
                         int64_t workspace_bytes, double* out3, void* stream);

/* ---- flow-matching objective: the number a checkpoint is trained on (opt-in: VFModel._step, evaluate --valid_loss) ----
 * Forward only.  Restated from the reference's VFModel._step (flowmse/model.py:130-143); for a row with clean spectrogram
 * x0, noisy y (complex64 [B,1,F,T]), time t (float32 [B], device) and noise z:
 *   sigma(t) = (1 - t) sigma_min + t sigma_max                            odes.py:86-88
 *   x_t      = (1 - t) x0 + t y + sigma(t) z                              odes.py:83-84, model.py:134-137
 *   u        = (sigma_max - sigma_min) z + (y - x0)                       odes.py:102-107, model.py:138-140
 *   v        = VFModel.forward(x_t, t, y) = -dnn(cat[x_t, y], t)          model.py:141, 164-170
 *   loss_b   = 0.5 * sum_{f,frame} |v - u|^2      (FLOWSE_LOSS_MSE)       model.py:118-128
 *            = 0.5 * sum_{f,frame} |v - u|        (FLOWSE_LOSS_MAE)
 *   loss     = mean_b loss_b
 * The time a training step draws, t_b = min((1 - rand)(T_rev - t_eps) + t_eps, T_rev) (model.py:132-133), is the
 * caller's: flowmse_amd.util.noise.loss_times restates it on the keyed stream.
 * z is a tensor (z != NULL) or generated in registers from the keyed stream of flowse_prior_sample_keyed (keys_dev != NULL:
 * B 64-bit words in device memory, with `seed`; frame offsets are 0); exactly one of the two is non-NULL.  T must be even
 * and the complex64 pointers 16-byte aligned.  Bad arguments return FLOWSE_ERR_ARG with the entry's name in the message
 * and launch nothing.  Every entry only enqueues: no host synchronisation (flowse_fm_loss grows the handle's buffers first
 * where it must, as every per-call entry does).
 * flowse_fm_pair: x_t into xt_out and, when target_out != NULL, u into target_out, both complex64 [B,1,F,T], in fp32 with
 *   the reference's operation order: a = 1 - t, sig = a sigma_min + t sigma_max, x_t = (a x0 + t y) + sig z,
 *   u = (sigma_max - sigma_min) z + (y - x0); each operation rounds once.
 * flowse_fm_loss_rows: from a field vf (complex64 [B,1,F,T]) the B row losses and their mean into out[0 .. B] (B + 1
 *   doubles, device).  u and d = vf - u are formed in float64 from the fp32 inputs and summed in float64: per row in
 *   fixed blocks whose number depends on (F, T) only, each block a strided per-thread sum and a fixed-order tree, the
 *   blocks then in index order, the rows of the mean in row order.  No atomics: a row's value does not depend on B or on
 *   its position, and the same input gives the same bits.  `workspace`: flowse_fm_loss_workspace_bytes(B, F, T) bytes of
 *   device memory (-FLOWSE_ERR_ARG for a bad shape).
 * flowse_fm_loss: flowse_fm_pair, then the shape's launch list in mode 1 (flowse_vf_forward's path, per-row t), then
 *   flowse_fm_loss_rows, on one stream; bit-identical to the three calls made separately.  x_t, v and the partials live in
 *   one buffer of the handle that is allocated by the first call (counted by FLOWSE_BYTES_OWNED; growing it synchronises
 *   the device once).  Works in every precision mode: the boundary tensors are complex64 in all of them. */
#define FLOWSE_LOSS_MSE 0
#define FLOWSE_LOSS_MAE 1
int flowse_fm_pair(const void* x0, const void* y, const float* t_dev, const void* z, const uint64_t* keys_dev, uint64_t seed,
                   float sigma_min, float sigma_max, void* xt_out, void* target_out, int B, int F, int T, void* stream);
int64_t flowse_fm_loss_workspace_bytes(int B, int F, int T);
int flowse_fm_loss_rows(const void* vf, const void* x0, const void* y, const void* z, const uint64_t* keys_dev, uint64_t seed,
                        float sigma_min, float sigma_max, int loss_type, double* out, void* workspace, int64_t workspace_bytes,
                        int B, int F, int T, void* stream);
int flowse_fm_loss(flowse_model* m, const void* x0, const void* y, const float* t_dev, const void* z, const uint64_t* keys_dev,
                   uint64_t seed, float sigma_min, float sigma_max, int loss_type, double* out, int B, int F, int T,
                   void* stream);

/* ---- in-library kernel timing (used by bench.py for the live roofline figure) -------------------------
 * Between _begin and _end every selected launch of this handle is bracketed by HIP events on the launch
 * stream (and the handle launches eagerly instead of replaying its hipGraph).  mode 0: only launches of the dominant
 * kernel -- the 3x3 ResBlock convolutions with fused GroupNorm+SiLU input and Cout > 64 (conv3x3_w2d_kernel<2, .> in
 * the fp32 mode, conv3x3_pc16_kernel<2, ., .> in the 16-bit storage modes) -- reported under the key
 * "dominant_conv3x3"; mode 1: every launch, keyed by op label.  _end synchronises
 * on the recorded events and writes a JSON object {label: {"launches", "ms", "flops", "bytes", "issued"}} into `json`:
 * algorithmic flops / bytes of the bracketed launches, and `issued` = the flops the matrix cores execute for them
 * (1/3 of the algorithmic direct-convolution flops per launch of the two-dimensional Winograd form, 1/2 per launch of
 * the one-dimensional F(4,3) form, all of them otherwise).  The extra key "_all_launches"
 * totals launches / flops / issued over EVERY launch made between _begin and _end (no timing). */
int flowse_profile_begin(flowse_model* m, int mode);
int flowse_profile_end(flowse_model* m, char* json, int cap);

/* ---- upfirdn2d: drop-in for the reference's native operator ------------------------------------------
 * Reference: upfirdn2d(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
 * (op/upfirdn2d.cpp:12-22; kernels op/upfirdn2d_kernel.cu:49-207).  input: float32 [planes, in_h, in_w]
 * (= NCHW with planes = N*C), kernel: float32 [kh, kw] device, out: [planes, out_h, out_w] with
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh) / down_y + 1 (same for w).  Pads must be >= 0. */
int flowse_upfirdn2d(const float* input, const float* kernel, int planes, int in_h, int in_w, int kh, int kw,
                     int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                     float* out, int out_h, int out_w, void* stream);

/* ---- per-op entry points (NHWC float32 device tensors) ------------------------------------------------
 * conv: out = (conv_{taps}(cat[in1,in2]; w) + bias + bias2[b] + res) * scale.  w: [Cout][taps][C1+C2] (channel
 * last), taps 9 (3x3, pad 1) or 1; in2/bias/bias2/res may be NULL.  Stands for ddpm_conv3x3 / ddpm_conv1x1 /
 * NIN (layers.py:100-124, 546-555) with the ResnetBlockBigGANpp epilogue (layerspp.py:262-274). */
int flowse_op_conv2d(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                     const float* bias2, int bias2_stride, const float* res, float* out, int B, int H, int W,
                     int Cout, int taps, float scale, float* splitk_scratch, void* stream);
/* Small images are computed split-K (K sliced over extra thread blocks, deterministic two-pass reduction) when
 * `splitk_scratch` holds flowse_op_conv2d_scratch_floats(...) floats (0 = this shape never splits); with
 * splitk_scratch == NULL the single-pass kernel is used. */
int64_t flowse_op_conv2d_scratch_floats(int B, int H, int W, int Cin, int Cout, int taps);
/* The same contract on the 16-bit matrix cores with 16-bit activation storage (BASELINE configs 3 / 5; dt 1 = bf16,
 * 2 = IEEE half): the fp32 tensors are rounded to dt on the way in, the conv runs as in the 16-bit modes of the model
 * handle (producer / consumer LDS-halo kernel for the 3x3 shapes it covers -- its fragment-order copy of the weights is
 * made here per call --, per-tap halo kernel or flat kernel (+ split-K) otherwise), the result is widened back.
 * Optional fused GroupNorm(+SiLU) of the input from per-(sample, channel) gn_mean / gn_scale [B][C1+C2] and gn_beta
 * [C1+C2] (LDS-halo shapes only).  `scratch`: device memory; sufficient for every shape: 2*(in + 2*w + res + out
 * elements) + 4*ksplit*out elements + 4 KB bytes (each of the up to seven sub-buffers is rounded up to 256 bytes; the
 * error message of a too-small call states the exact byte count).  Cout == 4 with taps == 9 on >= 64 tiles of
 * 16 x 16 pixels is the progressive-output head (ncsnpp.py:345-366): 16-bit input, but `res` (the pyramid) and `out` stay fp32
 * as in the model (conv3x3_head4_16_kernel; fused GroupNorm input allowed). */
int flowse_op_conv2d_16(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                        const float* res, const float* gn_mean, const float* gn_scale, const float* gn_beta, int silu,
                        float* out, int B, int H, int W, int Cout, int taps, float scale, int dt, void* scratch,
                        int64_t scratch_bytes, void* stream);
/* flowse_op_conv2d_16 plus the two epilogue inputs the model's 16-bit modes also use: a per-sample bias table `bias2`
 * (element (b, co) at bias2[b * bias2_stride + co], fp32, may be NULL; stride a multiple of 4, >= Cout) and, with
 * out_f32 != 0, fp32 output: `res` and `out` are then read and written by the convolution as fp32 tensors (out_dt = fp32,
 * no conversion at the boundary, no second rounding) -- the form of the few convs that leave the 16-bit domain.  Shapes of
 * the LDS-halo kernels, which store the operands' type only, run the flat kernel when out_f32 is set. */
int flowse_op_conv2d_16_ex(const float* in1, int C1, const float* in2, int C2, const float* w, const float* bias,
                           const float* bias2, int bias2_stride, const float* res, const float* gn_mean,
                           const float* gn_scale, const float* gn_beta, int silu, float* out, int out_f32, int B, int H,
                           int W, int Cout, int taps, float scale, int dt, void* scratch, int64_t scratch_bytes,
                           void* stream);
/* Which kernel the calling thread's last convolution launch ran (any entry point that launches one: the per-op entries
 * above and below, a forward pass while it is being recorded): the kernel family -- "flat", "flat_splitk", "halo", "f43",
 * "f43_splitk", "w2d", "1x1_stream", "head4", "head4_16", "cin4", "cin4_stats", "cin4_mfma", "flat16", "flat16_splitk",
 * "halo16", "halo_bf16x3", "pc16" -- or, for the small-image kernels (at most 2048 pixels), the instance: "smallm<1>", "smallm<2>", "smallm_tile16",
 * "smallm16b<NT2, bf16|f16, out16|out32>" with NT2 = 1 or 2.  Written by the launcher next to the launch, never derived
 * from the shape a second time; a host-side, thread-local record ("" before the first launch): replaying a captured
 * graph does not change it.  The pointer stays valid for the thread's lifetime; the text changes with the next launch. */
const char* flowse_op_last_conv_route(void);
/* What a convolution of this shape WOULD run: the library's one routing decision (the plan of a model handle and every
 * per-op entry go through it, the convs of a 4-channel input included), as one line of text.  Host only: no HIP call, works
 * with no GPU present.  in_dt / out_dt: storage types (0 fp32, 1 bf16, 2 half; out_dt = in_dt or 0 -- or, for an fp32 input
 * of four channels (C1 = 4, C2 = 0: the input layer and the Combine 1x1, whose input stays fp32 in the 16-bit modes), any of
 * the three: "cin4_mfma", "cin4_stats" (only where statistics are asked for) or "cin4", always whole K, and "flat" for the
 * widths those kernels do not take); (C1, C2): the parts of a concat input; offer_bits: what the caller could hand to the
 * launch, FLOWSE_OFFER_* below.  Writes
 *   "<kernel> ks=<K slices> reduce=<0|1> stats=<blocks per sample> gn=<0|1> issued=<1/3|1/2|1|3> reads=<copies>"
 * -- kernel: the family flowse_op_last_conv_route reports after that launch ("smallm" / "smallm16b" without the instance);
 * reduce: a separate reduction launch follows; stats: geometry of the fused GroupNorm statistics (0: none); gn: the kernel
 * can normalise its input on load; issued: issued / nominal FLOPs as the profile counts them; reads: the weight copies the
 * kernel dereferences next to the packed fp32 weights, joined by "+" -- "wq" (the 16-bit weights: the operand itself for a
 * 16-bit input, whether offered or not), "wino", "wino2", "wsm", "wsm16" (the 16 x 16-tile fragment order, offered with
 * FLOWSE_OFFER_WSM), "wfrag" -- or "-" for none; always among what was offered -- or "error <status>" for a
 * request no kernel takes (flowse_last_error has launch_conv's text).  cap >= 64; the longest answer has 70 characters. */
enum {
    FLOWSE_OFFER_WINO = 1,        /* F(4,3) weights */
    FLOWSE_OFFER_WINO2 = 2,       /* F(4,3) x F(2,3) weights */
    FLOWSE_OFFER_WSM = 4,         /* fp32 fragment-order copy (small-image and streaming 1x1 kernels) */
    FLOWSE_OFFER_WFRAG = 8,       /* 16-bit fragment-order copy (producer / consumer and 16-bit small-image kernels) */
    FLOWSE_OFFER_WQ = 16,         /* 16-bit weights: one plane ... */
    FLOWSE_OFFER_WQ_SPLIT3 = 32,  /* ... or the split-bf16 pair (with FLOWSE_OFFER_WQ) */
    FLOWSE_OFFER_WQ_F16 = 64,     /* the planes hold IEEE half */
    FLOWSE_OFFER_SLAB = 128,      /* a split-K slab may be used */
    FLOWSE_OFFER_GN = 256,        /* the input is normalised on load */
    FLOWSE_OFFER_BIAS2 = 512,     /* a per-sample bias is present */
    FLOWSE_OFFER_STATS = 1024,    /* fused statistics of the output are asked for */
    FLOWSE_OFFER_FOLD = 2048      /* a folded 1x1 shortcut rides along */
};
int flowse_op_conv_route(int in_dt, int out_dt, int B, int H, int W, int C1, int C2, int Cout, int taps, int offer_bits,
                         char* text, int cap);
/* Tail of ResnetBlockBigGANpp (layerspp.py:265-274) in 16-bit storage as ONE launch of the producer / consumer kernel:
 *   out = (conv3x3(act(GroupNorm(h)); w1) + b1 + conv1x1(cat[x1, x2]; w2) + b2) * scale
 * The 1x1 shortcut Conv_2(x) runs as extra K steps of Conv_1's launch (the form the 16-bit model modes use wherever
 * Conv_1 is on that kernel; FLOWSE_NO_SCFOLD=1 at plan time restores the separate launch).  h: [B][H][W][C] with per-
 * (sample, channel) gn_mean / gn_scale [B][C] and gn_beta [C] (NULL: no normalisation); w1 [Cout][9][C]; x1 / x2 (NULL)
 * the shortcut's input channels (XC1, XC2 multiples of 32, >= 96 in all), w2 [Cout][1][XC1 + XC2].  Shapes: H, W
 * multiples of 16, C % 32 == 0, Cout % 128 == 0, at least 64 (16 x 16 tile, 128-channel block) items, else
 * FLOWSE_ERR_SHAPE.  `scratch`: 2 * (h + x1 + x2 + 2 w1 + 2 w2 + out elements) + 4 KB bytes. */
int flowse_op_resblock_tail_16(const float* h, int C, const float* gn_mean, const float* gn_scale, const float* gn_beta,
                               int silu, const float* w1, const float* b1, const float* x1, int XC1, const float* x2,
                               int XC2, const float* w2, const float* b2, float* out, int B, int H, int W, int Cout,
                               float scale, int dt, void* scratch, int64_t scratch_bytes, void* stream);
/* Test / A-B hook, process-wide: channel-block width of conv3x3_pc16_kernel.  -1 (default): 128-channel blocks, 64-channel
 * blocks for launches with fewer than 3/4 of a (16 x 16 tile, 128-channel block) item per compute unit; 0: always 128;
 * 1: always 64 (also FLOWSE_PC16_NARROW=0 / 1 in the environment).  Results differ only in summation grouping of the
 * GroupNorm partial statistics (the convolution sums are identical). */
int flowse_op_pc16_channel_blocks(int mode);
/* Test hook, thread-local: a sink for the GroupNorm statistics a conv kernel fuses into its output stage.  While armed
 * (buf, floats > 0), every per-op conv entry -- flowse_op_conv2d, _conv3x3_gn, _conv3x3_f43, _conv3x3_w2d, _conv2d_16,
 * _conv2d_16_ex, _resblock_tail_16 -- launches with the partials of its OUTPUT written to buf, [B][nblk][Cout][2] floats of
 * (mean, M2) per (sample, pixel block, channel): the layout flowse_op_gn_finalize consumes.  nblk is the route's of exactly
 * the arguments the entry launches (the "stats=" of flowse_op_conv_route for them); flowse_op_stats_sink_blocks() returns it
 * after the call, 0 where that route writes no statistics (the launch then runs without).  A sink too small for
 * B * nblk * Cout * 2 floats: FLOWSE_ERR_ARG, nothing launched.  Only the GROUP sums of the partials are specified: a
 * kernel may spread a group's (mean, M2) over its channels as it likes.  (NULL, 0) disarms; disarmed, nothing changes. */
int flowse_op_stats_sink(float* buf, int64_t floats);
int flowse_op_stats_sink_blocks(void);
/* The stand-alone statistics kernel: partial [B][nblk][C1 + C2][2] of cat[in1, in2] ([B][HW][C*] fp32, in2 may be NULL) in
 * nblk blocks of ceil(HW / nblk) pixels.  dt 1 / 2: the input is first rounded to bf16 / half into `scratch` (256 bytes of
 * slack per tensor) and read from there, as the 16-bit storage modes do; dt 0 needs no scratch. */
int flowse_op_gn_stats(const float* in1, int C1, const float* in2, int C2, int B, int HW, int dt, void* scratch,
                       int64_t scratch_bytes, float* partial, int nblk, void* stream);
/* Merge of one or two partial sets (set 1: channels [0, C1), nblk1 blocks; set 2, may be NULL: [C1, C1 + C2), nblk2 blocks;
 * each in blocks of ceil(HW / nblk) pixels, the last one short) into per-(sample, channel) mean and scale = rstd * gamma
 * [B][C1 + C2] over G groups.  With `out` (and in1, beta; in2 where C2 > 0) the one-launch form for small images instead:
 * out = act((cat[in1, in2] - mean) * scale + beta), mean / scale not written. */
int flowse_op_gn_finalize(const float* p1, int nblk1, int C1, const float* p2, int nblk2, int C2, int B, int HW, int G,
                          const float* gamma, float eps, float* mean, float* scale, const float* in1, const float* in2,
                          const float* beta, int silu, float* out, void* stream);
/* Fused ResnetBlock half:  out = (conv3x3(act(GroupNorm(cat[in1,in2]))) + bias + bias2[b] + res) * scale
 * (layerspp.py:246-249 / :265-267) with the normalisation + SiLU applied while the input tile is staged into LDS.
 * Only for shapes the halo kernel covers (H % 8 == 0, W % 16 == 0, C1 % 32 == 0, C2 % 32 == 0, image large
 * enough not to be split-K): otherwise FLOWSE_ERR_SHAPE.  `scratch`: flowse_op_group_norm_scratch_floats(). */
int flowse_op_conv3x3_gn(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                         float eps, int silu, const float* w, const float* bias, const float* bias2,
                         int bias2_stride, const float* res, float* out, int B, int H, int W, int Cout, float scale,
                         float* scratch, void* stream);
/* The same fused ResnetBlock half computed with the F(4,3) Winograd form of the 3x3 filter along its vertical axis: 6
 * multiplies per four outputs instead of 12 (half of the direct-convolution FLOPs on the matrix cores; fp32 error ~3x the
 * direct sum's) -- the kernel the model handle uses for every 3x3 convolution with Cout % 64 == 0 on images large enough
 * for the halo tiling (FLOWSE_NO_WINOGRAD=1 selects the direct kernel).  gamma == NULL: plain convolution without the
 * GroupNorm + SiLU input stage.  `w` is the packed [Cout][9][Cin] weight as for flowse_op_conv2d; the transformed
 * weights are derived into `scratch` (flowse_op_conv3x3_f43_scratch_floats floats).  Other shapes: FLOWSE_ERR_SHAPE. */
int flowse_op_conv3x3_f43(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                          float eps, int silu, const float* w, const float* bias, const float* bias2,
                          int bias2_stride, const float* res, float* out, int B, int H, int W, int Cout, float scale,
                          float* scratch, void* stream);
int64_t flowse_op_conv3x3_f43_scratch_floats(int B, int H, int W, int C, int Cout);
/* The same contract in the TWO-dimensional Winograd form F(4,3) (vertical) x F(2,3) (horizontal): 24 multiplies per
 * 4 x 2 output patch instead of 72 (one third of the direct-convolution FLOPs on the matrix cores; fp32 error ~1.5x the
 * 1-D form's).  Covers H % 16 == 0, W % 16 == 0, channel counts multiples of 32, Cout % 64 == 0; other shapes:
 * FLOWSE_ERR_SHAPE.  The model handle uses it for launches of at least 128 blocks of 16 x 16 pixels x 64 channels (below
 * 256 of them with 32-channel blocks, so that every CU gets one) unless FLOWSE_W2D=0. */
int flowse_op_conv3x3_w2d(const float* in1, int C1, const float* in2, int C2, const float* gamma, const float* beta,
                          float eps, int silu, const float* w, const float* bias, const float* bias2,
                          int bias2_stride, const float* res, float* out, int B, int H, int W, int Cout, float scale,
                          float* scratch, void* stream);
int64_t flowse_op_conv3x3_w2d_scratch_floats(int B, int H, int W, int C, int Cout);
/* GroupNorm(min(C/4,32) groups, eps) [+ SiLU] over cat[in1,in2] (layerspp.py:219,231; ncsnpp.py:337).
 * `scratch` must hold flowse_op_group_norm_scratch_floats(B,H*W,C1+C2) floats. */
int64_t flowse_op_group_norm_scratch_floats(int B, int HW, int C);
int flowse_op_group_norm(const float* in1, int C1, const float* in2, int C2, const float* gamma,
                         const float* beta, float eps, int silu, float* out, int B, int H, int W, float* scratch,
                         void* stream);
/* FIR x2 resampling with [1,3,3,1] (up_or_down_sampling.py:195-257). up: out [B,2H,2W,C]; down: [B,H/2,W/2,C] */
int flowse_op_fir_up(const float* in, float* out, int B, int H, int W, int C, void* stream);
int flowse_op_fir_down(const float* in, float* out, int B, int H, int W, int C, void* stream);
/* softmax(q k^T C^-1/2) v over L tokens; qkv [B][L][3C], out [B][L][C] (layerspp.py:82-86). */
int flowse_op_attention(const float* qkv, float* out, int B, int L, int C, void* stream);
/* The same on the 16-bit matrix cores (attention16_kernel, as in the bf16 / fp16 storage modes of the model handle; dt 1 =
 * bf16, 2 = IEEE half): qkv is rounded to dt on the way in, the result widened back.  `scratch`: device memory of at least
 * 2*(4*B*L*C) + 512 bytes. */
int flowse_op_attention_16(const float* qkv, float* out, int B, int L, int C, int dt, void* scratch, int64_t scratch_bytes,
                           void* stream);
/* GaussianFourierProjection(log t) (layerspp.py:39-41, ncsnpp.py:259): out [B][2E] */
int flowse_op_gfp(const float* t, const float* W, float* out, int B, int E, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOWSE_HIP_H */
