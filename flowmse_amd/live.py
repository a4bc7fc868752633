"""Live enhancement: a recording is enhanced while it arrives, and the bytes are those of the finished file.

``LiveEnhancer`` takes the samples of ONE recording in pushes of any sizes and returns enhanced samples as soon as they
are final.  **Contract:** the concatenation of everything ``push`` and ``finish`` returned is, bit for bit, what
``chunked.enhance_long(model, y, chunk_frames, overlap_frames, batch=1, noise_key=key, noise_seed=seed, ...)`` returns
for the whole recording ``y`` with the same solver, ``N``, ``T_rev``, ``t_eps`` and precision, when the enhancer's
``norm`` equals the recording's ``max|y|``.  That includes a recording that fits one chunk (``K = 1``), which
``enhance_long`` hands to ``enhance_waveform`` with ``T`` padded to a multiple of 64.  "Live" is not "streams": ``--streams``
and the HIP-stream lanes of ``flowmse_amd.parallel`` are concurrent sampler calls and have nothing to do with this module.

Why it holds.  Chunk ``k`` of ``enhance_long`` depends on ``Tc`` frames of input and nothing after them; the seam rule looks
back one chunk; the keyed noise is addressed at absolute frames; a frame's value depends on (samples, scale, t) only and a
sample's value on the frames over it only.  The two window entries of the library (``flowse_stft_compress_window``,
``flowse_istft_decompress_window``) run the per-frame and per-sample device code of the chunk calls on what is held here.

Schedule (``n_fft = 510``, ``hop_length = 128``, ``center=True``).  ``stft_frame`` reads ``[128 t - 255, 128 t + 254]``,
reflected at both ends, and ``istft_gather`` puts frame ``t`` over the same output samples; so frame ``t`` is computable
without right padding once ``128 t + 255`` samples have arrived.  ``flowmse_amd.schedule`` holds one object per geometry
that answers five questions for chunk ``k``, and tests/test_schedule_host.py holds its answers to those index ranges:

1. Which frames does it hold, and when is it ready (``n_k``: its last frame is computable)?  A chunk that became ready this
   way is never the recording's last: ``L >= n_k`` gives ``L // 128 + 1`` frames, more than end with chunk ``k``.
2. Which output samples are final once it is sampled and is not the last (``s < E_k``, ``E_{-1} = 0``)?  The samples
   ``[E_{k-1}, E_k)`` are emitted then.
3. How much history does that range need?  It lies under frames from three before the first frame that became final.  If
   those are plain frames of chunk ``k - 1``, chunks ``k - 1`` and ``k`` suffice; if they are BLENDED frames of chunk
   ``k - 1``, whose other half is chunk ``k - 2``, two previous chunks are kept and the window entry takes all three.
4. Which samples does it read, and which may go after it?  Those before ``128 f - 256`` (clamped at 0), ``f`` the first
   frame of chunk ``k + 1``: one more than that chunk reads while the recording is open.  If the recording ends at a
   multiple of 128 exactly one frame past chunk ``k`` (possible at ``To = 0``), that frame's right reflection reads sample
   ``L - 256``.
5. What is the worst algorithmic latency ``max_k (n_k - E_{k-1})`` (``latency_samples``)?  The sampler's compute time comes on top.

===================  ==========================================  ====================================================
..                   overlap (``hop = Tc - To``; the default)    trailing (``hop_frames=H``, ``fade_frames=X``; ``P = Tc - H``)
===================  ==========================================  ====================================================
frames of chunk k    ``[k hop, k hop + Tc)``                     ``[k H - P, k H + H)``, those ``< 0`` zero
keyed noise from     stream frame ``k hop``                      stream frame ``k H``
``n_k``              ``128 (k hop + Tc - 1) + 255``              ``128 (k H + H - 1) + 255``
``E_k``              ``128 (k + 1) hop - 255``                   ``128 ((k + 1) H - X) - 255``, clamped at 0
two chunks kept if   ``Tc - 2 To < 3``, i.e. ``To = Tc / 2``     ``H - X < 3``: ``(8, 8)``, ``(4, 2)``, ...
dropped after k      before ``128 (k + 1) hop - 256``            before ``128 ((k + 1) H - P) - 256``
held before a push   the backlog                                 at most ``128 Tc + 382`` samples
latency              ``128 Tc + 382``: 2.07 s at ``Tc = 256``,   ``128 (H + X) + 382``: 0.184 s at ``(16, 4)``,
                     0.54 s at ``Tc = 64``                       0.104 s at ``(8, 2)``
``K``                ``plan_chunks(T, Tc, To)[0]``               ``ceil(T / H)``; there is no ``K = 1`` case
===================  ==========================================  ====================================================

(``Tc - 2 To`` is a multiple of 4, so ``To = Tc / 2`` is the only overlap geometry with blended history.)

``finish()`` fixes ``L`` (``L > 255``, as every call of the package requires) and ``K`` from ``T = L // 128 + 1``, samples the
chunks that were waiting for samples that never came -- in order, at batch width 1, now with the right reflection and the
zero frames ``>= T`` of ``flowse_stft_compress_chunks`` -- and emits ``[E_{last emitted}, L)``.

State: the sample buffer (one linear device tensor whose capacity follows the largest push), one or two previous chunks
(512 KB each at ``Tc = 256``) and nothing else; every push returns all it produced, so no output is ever pending.
``norm`` must be known before the first chunk: a positive float (a capture device's full scale, say), or ``"first"`` =
``max|y|`` over the samples ``[0, n_0)`` that make chunk 0 ready (the whole recording if it ends earlier; 1.0 if that is 0)
-- a value that depends on the signal alone, not on the push sizes, read back from the device once.  With a float ``norm``
the host waits for the device only in the copy of the emitted samples, with ``as_tensor=True`` never (beyond what one
``enhance_long`` sampler call does).

Other rates (``input_rate != 16000``; ``flowmse_amd.resample.StreamResampler``, one ``flowse_resample_poly_window`` launch
per push that finalises an output, bit for bit ``flowse_resample_poly`` on the finished signal).  Pushes go through a
resampler to 16 kHz; the 16 kHz samples that it makes final feed the path above unchanged, and ``finish()`` appends its
last outputs, so that the 16 kHz recording has ``ceil(L 16000 / input_rate)`` samples.  With ``output_rate="input"`` the
emitted 16 kHz samples go through a second resampler back, and the total is trimmed to the input's sample count at
``finish()``.  **Contract:** the concatenated output is, bit for bit, the waveform of ``enhance.enhance_recording(model, y,
input_rate, output_rate, chunk_frames, overlap_frames, batch=1, noise_key, noise_seed, ...)`` when ``norm`` equals
``max|y16|`` of the resampled recording, which is what ``enhance_long`` normalises by.  ``norm="first"`` is the peak of the
16 kHz samples ``[0, n_0)``.  ``samples_in`` and ``samples_out`` count at the caller's rates.  The schedule gains two steps:
16 kHz sample ``m`` is final once input sample ``q_in(m) = (half + m down) div up`` has arrived (``stream_plan``), so chunk
``k`` runs at ``q_in(n_k - 1) + 1`` input samples, and of the ``E`` 16 kHz samples returned ``stream_plan(E, 16000 ->
input)`` are final at the input rate; ``latency_samples`` takes the worst case over ``k`` (at 48 kHz in and out:
``3 (128 Tc + 382) + 58`` samples, 58 being the two filters' ``28 + 30``).  With the defaults nothing of this exists: the
object makes the calls it made before and returns the same bytes.

Trailing chunks (``hop_frames=H``, ``fade_frames=X``; opt-in, NOT the reference's computation).  The latency above is the
chunk: what chunk ``k`` makes final starts at its first frame.  With ``hop_frames`` the chunk of ``Tc`` frames slides by a
small hop ``H`` instead; its older ``P = Tc - H`` frames are context only and only its tail is kept (``chunked.plan_trailing``
has the geometry and the seam rule, ``chunked.enhance_trailing`` is the file call).  **Contract:** the concatenated output
is, bit for bit, ``enhance_trailing(model, y, chunk_frames, hop_frames, fade_frames, batch=1, noise_key=key,
noise_seed=seed, ...)`` of the finished recording when ``norm`` equals ``max|y|``, whatever the push sizes; through the
library's ``flowse_stft_compress_trailing_window`` and ``flowse_istft_decompress_trailing_window``.  The schedule is the
table's right column:

* The first chunks are right-aligned against zero frames, so the latency holds from the first sample on, and a recording
  shorter than one hop is one right-aligned chunk.
* After chunk ``k`` (not the last) the ``X`` frames before ``(k + 1) H`` wait for the cross-fade into chunk ``k + 1``.  What is
  emitted lies under frames from ``k H - X - 3`` on, which chunk ``k - 1`` owns (``(k H - 3) // H = k - 1``).
* The sampler's compute time is spent ``Tc / H`` times as often (``Tc / H`` network rows per ``H`` frames).
* The buffer is sized to what is held before a push plus the largest push, from the first push on.
* A stream so long that ``k H + Tc`` passes ``2^31 - 2``, the last frame the keyed noise addresses, is refused by name.
* ``input_rate`` / ``output_rate`` work unchanged through the resamplers around this 16 kHz path, and ``latency_samples`` takes
  the worst case over ``k`` by the method above with this schedule's ``n_k`` and ``E_k``.

Not in this geometry: ``LivePool`` / ``--live_channels`` (trailing rows of several sessions in one call are the obvious
follow-up; ``LivePool.open`` refuses the keywords by name), ``--streams``, several GPUs, ensembles.  ``H`` and ``X`` were not
chosen by listening -- no released checkpoint is at hand -- so the defaults are chosen values, not tuned ones.

Out of scope: ``--streams`` lanes, several GPUs, time-varying or non-rational rates, noise that is not keyed, and any CPU or
oracle path -- the oracle composition is ``enhance_long``'s, and this module is pinned to ``enhance_long``.  Rows of several
sessions pooled into one sampler call, and several channels, are ``flowmse_amd.livepool``'s, which asks the same
schedule object; a ``LiveEnhancer`` stays one mono stream at width 1.
"""
import numpy as np
import torch

from flowmse_amd.chunked import CHUNK_FRAMES, NOISE_FRAME_MAX, OVERLAP_FRAMES, plan_chunks
from flowmse_amd.schedule import HOP, KEEP, PADC, RATE, schedule_for            # noqa: F401  (HOP .. RATE: importable from here)


def live_plan(n_samples, Tc=CHUNK_FRAMES, To=OVERLAP_FRAMES, finished=False, hop_frames=None, fade_frames=0):
    """``(chunks_ready, samples_final)`` after ``n_samples`` samples of a recording (module docstring): how many chunks a
    ``LiveEnhancer`` has sampled and how many output samples it has returned.  ``finished``: the recording has ended at
    ``n_samples`` -- all ``K`` chunks, all samples.  Host arithmetic only; geometry errors are ``plan_chunks``'.  With
    ``hop_frames`` the trailing schedule (``To`` is not read; geometry errors are ``plan_trailing``'s)."""
    return schedule_for(Tc, To, hop_frames, fade_frames, "live_plan").plan(n_samples, finished)


PCM_FORMATS = {"s16le": 2, "f32le": 4}                    # bytes per sample


def pcm_decode(data, fmt):
    """Raw little-endian mono PCM -> float32 samples.  ``s16le``: value / 32768; ``f32le``: the values themselves.  Bytes
    past the last whole sample are ignored."""
    width = PCM_FORMATS[fmt]
    data = data[:len(data) - len(data) % width]
    if fmt == "f32le":
        return np.frombuffer(data, dtype="<f4").astype(np.float32)
    return np.frombuffer(data, dtype="<i2").astype(np.float32) / np.float32(32768.0)


def pcm_encode(x, fmt):
    """float32 samples -> raw little-endian mono PCM.  ``s16le``: ``x * 32768`` rounded to nearest (ties to even) and
    saturated to [-32768, 32767], so that decode -> encode returns the bytes; a sample that is not finite becomes 0.
    ``f32le``: the values themselves."""
    x = np.asarray(x, dtype=np.float32)
    if fmt == "f32le":
        return x.astype("<f4").tobytes()
    if fmt != "s16le":
        raise KeyError(fmt)
    v = np.rint(x.astype(np.float64) * 32768.0)
    v = np.where(np.isfinite(v), v, 0.0)
    return np.clip(v, -32768.0, 32767.0).astype("<i2").tobytes()


def pcm_deinterleave(x, channels):
    """Interleaved samples ``[n * channels]`` (frame after frame, as PCM devices deliver them) -> ``[channels, n]``, contiguous.
    Samples past the last whole frame are ignored."""
    channels = int(channels)
    if channels < 1:
        raise ValueError(f"pcm_deinterleave: channels must be >= 1, got {channels}")
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError(f"pcm_deinterleave takes 1-D interleaved samples, got {x.shape}")
    n = x.shape[0] // channels
    return np.ascontiguousarray(x[:n * channels].reshape(n, channels).T)


def pcm_interleave(x):
    """``[channels, n]`` -> interleaved ``[n * channels]``, the inverse of ``pcm_deinterleave``."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"pcm_interleave takes [channels, n] samples, got {x.shape}")
    return np.ascontiguousarray(x.T).reshape(-1)


def latency_samples(Tc=CHUNK_FRAMES, input_rate=RATE, output_rate="16000", To=OVERLAP_FRAMES, hop_frames=None, fade_frames=0):
    """Worst algorithmic latency in samples at ``input_rate``.  At 16 kHz: ``max_k (n_k - E_{k-1}) = 128 Tc + 382``; it does
    not depend on the overlap.  At another rate it follows from the three schedules (module docstring, "Other rates"): chunk
    ``k`` runs when ``A_k = q_in(n_k - 1) + 1`` input samples have arrived, and what was returned before it covers
    ``R_k`` input samples, ``stream_plan(E_{k-1}, 16000 -> input)`` under ``output_rate="input"`` and
    ``E_{k-1} input_rate div 16000`` at 16 kHz output; the value is ``max_k (A_k - R_k)``.  Both terms are floors over the
    reduced ``up`` of the input ratio, so ``k = 0 .. up`` covers every case.  With ``hop_frames`` (and ``fade_frames``) the
    trailing schedule: ``128 (H + X) + 382`` at 16 kHz, and the same method with its ``n_k`` and ``E_k`` at another rate."""
    return schedule_for(Tc, To, hop_frames, fade_frames, "latency_samples").latency(input_rate, output_rate)


def check_norm(norm, who):
    """``norm`` of a stream: ``"first"`` or a positive finite float, refused under the caller's name ``who``."""
    if not (norm == "first" if isinstance(norm, str) else float(norm) > 0.0 and np.isfinite(float(norm))):
        raise ValueError(f"{who}: norm is a positive float or 'first', got {norm!r}")
    return norm if isinstance(norm, str) else float(norm)


def require_hip_model(model, device, who):
    """``(device, data_module)`` of a HIP-backed ``VFModel`` on a cuda device with the released STFT, for the module ``who``;
    anything else is a ``RuntimeError``: there is no CPU fallback."""
    dm = getattr(model, "data_module", None)
    if not (torch.cuda.is_available() and callable(getattr(model, "rk_sample_", None))
            and hasattr(getattr(model, "dnn", None), "reserve")):
        raise RuntimeError(f"{who} runs on the MI355X HIP kernels only: a HIP-backed VFModel on a 'cuda' device (there is no "
                           "CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who} runs on the MI355X HIP kernels only, got device {device} (there is no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if not (hasattr(dm, "fused_ok") and dm.fused_ok(torch.empty(0, device=device))):
        raise RuntimeError(f"{who} needs the HIP spectrogram kernels: the released STFT configuration (n_fft 510, hop 128, hann, "
                           "'exponent')")
    return device, dm


class SampleBuffer:
    """The samples ``[s0, s0 + n)`` of ``C`` channels, at the front of one ``[C, capacity]`` float32 device tensor ``data``
    that grows once per new largest backlog and never shrinks."""

    def __init__(self, channels, device):
        self.data = torch.empty(int(channels), 0, dtype=torch.float32, device=device)
        self.s0 = self.n = 0

    capacity = property(lambda self: self.data.size(1))

    def append(self, x, min_capacity=0):
        """``x``: ``[C, m]`` (or ``[m]`` at one channel) on the device, m > 0.  A buffer that has to grow takes at least
        ``min_capacity + m``."""
        m = x.size(-1)
        if self.n + m > self.capacity:                      # contents move to the front of the new tensor
            grown = torch.empty(self.data.size(0), max(self.n, min_capacity) + m, dtype=torch.float32, device=self.data.device)
            grown[:, :self.n] = self.data[:, :self.n]
            self.data = grown
        self.data[:, self.n:self.n + m] = x
        self.n += m

    def drop(self, upto):
        """Forget the samples before ``upto``: the rest moves to the front of the same tensor."""
        cut = min(upto, self.s0 + self.n) - self.s0
        if cut <= 0:
            return
        if cut < self.n:
            rest = self.data[:, cut:self.n].clone()
            self.data[:, :rest.size(1)] = rest
        self.s0 += cut
        self.n -= cut

    def view(self, lo, hi):
        """Samples ``[lo, hi)`` of every channel, ``s0 <= lo``: a view."""
        return self.data[:, lo - self.s0:hi - self.s0]


class LiveEnhancer:
    """One recording, enhanced as it arrives (module docstring).  ``model``: a HIP-backed ``VFModel`` on ``device`` (default:
    the current one); ``key`` / ``seed``: the keyed noise stream, as ``enhance_long``'s ``noise_key`` / ``noise_seed``;
    ``norm``: a positive float or ``"first"``.  The precision is the model's (``model.dnn.set_precision``).  ``input_rate``:
    the sample rate of what is pushed (default 16000; any ratio ``resample.rational`` admits); ``output_rate``: ``"16000"``
    returns the network's rate, ``"input"`` the input's (module docstring, "Other rates")."""

    def __init__(self, model, *, norm, key, seed=0, chunk_frames=CHUNK_FRAMES, overlap_frames=OVERLAP_FRAMES, N=5, T_rev=1.0,
                 t_eps=0.03, odesolver="euler", device=None, input_rate=RATE, output_rate="16000", hop_frames=None,
                 fade_frames=0):
        plan_chunks(1, chunk_frames, overlap_frames)       # checked in either geometry, and first
        self.sched = schedule_for(chunk_frames, overlap_frames, hop_frames, fade_frames, "LiveEnhancer")
        self.Tc, self.To = int(chunk_frames), int(overlap_frames)
        self.input_rate = int(input_rate)
        if output_rate not in ("16000", "input"):
            raise ValueError(f"LiveEnhancer: output_rate is '16000' or 'input', got {output_rate!r}")
        self.output_rate = output_rate
        if self.input_rate != RATE:
            from flowmse_amd.resample import rational
            rational(self.input_rate, RATE)                       # an unsupported ratio is refused here, by name
        if key is None:
            raise ValueError("LiveEnhancer: key is required (keyed noise only; util.noise.utterance_key makes one)")
        self._norm_arg = check_norm(norm, "LiveEnhancer")
        self.device, self._dm = require_hip_model(model, device, "flowmse_amd.live")
        self.model = model
        self._solver = dict(N=int(N), T_rev=T_rev, t_eps=t_eps)
        self._odesolver, self._seed = odesolver, int(seed)
        self.H = self.X = None                              # hop_frames: the trailing schedule (module docstring)
        if hop_frames is None:
            self._stft, self._istft = self._overlap_calls(self.Tc, self.sched.hop)
        else:
            self.H, self.X = self.sched.H, self.sched.X
            self._stft, self._istft = self._window_calls(
                self.Tc, "flowse_stft_compress_trailing_window", lambda k: (k, self.Tc, self.H),
                "flowse_istft_decompress_trailing_window", (self.Tc, self.H, self.X), self._refuse_past_noise)
        with torch.cuda.device(self.device):
            model.dnn.reserve(1, 256, self.Tc)
        self._buf = SampleBuffer(1, self.device)
        self._rs_in = self._rs_out = None                   # input_rate != 16000: the resamplers around the 16 kHz path
        if self.input_rate != RATE:
            from flowmse_amd.resample import StreamResampler
            self._rs_in = StreamResampler(self.input_rate, RATE, self.device)
            if output_rate == "input":
                self._rs_out = StreamResampler(RATE, self.input_rate, self.device)
        self.reset(key)

    # ---- public state -----------------------------------------------------------------------------------------
    @property
    def latency_samples(self):
        return self.sched.latency(self.input_rate, self.output_rate)

    def state_bytes(self):
        """Device bytes this object holds between pushes: the sample buffer (its capacity), the previous chunks and the
        buffers of the resamplers, if any.  No output is pending between calls.  The model's workspace is the model's
        (``reserve(1, 256, Tc)``)."""
        kept = [c for c in (self._prev, self._prev2) if c is not None]
        rs = sum(r.state_bytes() for r in (self._rs_in, self._rs_out) if r is not None)
        return self._buf.capacity * 4 + sum(c.numel() * 8 for c in kept) + rs

    def reset(self, key=None):
        """Forget the recording (the buffer keeps its capacity); ``key``: the next recording's, default the same one."""
        if key is not None:
            self.key = int(key)
        self.samples_in = self.samples_out = 0              # at the caller's rates
        self._in16 = self._out16 = 0                        # at 16 kHz: what the chunk schedule counts
        for r in (self._rs_in, self._rs_out):
            if r is not None:
                r.reset()
        self._buf.s0 = self._buf.n = 0                      # the buffer holds samples [s0, s0 + n) of the recording
        self._k = 0                                         # next chunk to sample
        self._prev = self._prev2 = None
        self._finished = False
        self.norm = None if isinstance(self._norm_arg, str) else self._norm_arg

    # ---- feeding ----------------------------------------------------------------------------------------------
    def push(self, samples, as_tensor=False):
        """Append ``samples`` (float32, 1-D or [1, n], n >= 0: numpy, CPU tensor or device tensor) and return the enhanced
        samples that became final: float32 numpy (possibly empty), or with ``as_tensor`` a 1-D device tensor."""
        if self._finished:
            raise RuntimeError("LiveEnhancer.push after finish(): call reset() to start another recording")
        if self._rs_in is not None:                         # the 16 kHz samples this push made final feed the path below
            with torch.cuda.device(self.device):
                samples = self._rs_in.push(samples, as_tensor=True)
            self.samples_in = self._rs_in.samples_in
        self._append(samples)
        out = []
        with torch.cuda.device(self.device):
            while self._in16 >= self.sched.ready_at(self._k):
                out.append(self._chunk(self._k, None))
        return self._deliver(out, as_tensor)

    def finish(self, as_tensor=False):
        """The recording has ended: sample what was waiting and return the remaining samples up to ``L = samples_in``."""
        if self._finished:
            raise RuntimeError("LiveEnhancer.finish called twice: call reset() to start another recording")
        if self._rs_in is not None:                         # the 16 kHz recording ends at out_len(samples_in)
            from flowmse_amd.resample import stream_plan
            L = stream_plan(self.samples_in, self._rs_in.up, self._rs_in.down, finished=True)
        else:
            L = self._in16
        if L <= PADC:
            raise ValueError(f"LiveEnhancer.finish: a recording needs more than {PADC} samples (n_fft // 2 of the centred "
                             f"STFT), got {L}")
        if self._rs_in is not None:
            with torch.cuda.device(self.device):
                self._append(self._rs_in.finish(as_tensor=True))
        K, single = self.sched.chunks(L // HOP + 1), self.sched.single_width(L // HOP + 1)
        out = []
        with torch.cuda.device(self.device):
            if single is not None and K == 1:               # chunk 0 never became ready: enhance_waveform's one padded row
                out.append(self._single(L, single))
            while self._k < K:
                out.append(self._chunk(self._k, L, last=self._k == K - 1))
        self._finished = True
        self._prev = self._prev2 = None
        self._buf.drop(self._buf.s0 + self._buf.n)
        return self._deliver(out, as_tensor, last=True)

    # ---- internals --------------------------------------------------------------------------------------------
    def _append(self, samples):
        if isinstance(samples, np.ndarray):
            samples = torch.from_numpy(np.ascontiguousarray(samples))
        if not torch.is_tensor(samples) or samples.dtype != torch.float32:
            raise TypeError("LiveEnhancer.push takes float32 samples (numpy array or tensor), got "
                            f"{getattr(samples, 'dtype', type(samples).__name__)}")
        if samples.dim() == 2 and samples.size(0) == 1:
            samples = samples[0]
        if samples.dim() != 1:
            raise ValueError(f"LiveEnhancer.push takes one channel, 1-D or [1, n], got {tuple(samples.shape)}")
        if samples.numel() == 0:
            return
        self._buf.append(samples.to(self.device), self.sched.min_capacity)   # grows once per new largest push
        self._in16 += samples.numel()

    def _normalised(self, lo, hi):
        """Samples [lo, hi) of the recording divided by ``norm`` as ``enhance_long`` divides them: on the device, one
        elementwise torch division by the Python float."""
        if self.norm is None:                               # norm="first": the peak of [0, n_0), or of all there is
            peak = self._buf.view(0, min(self.sched.ready_at(0), self._in16))[0].abs().max().item()
            self.norm = peak if peak > 0.0 else 1.0
        return self._buf.view(lo, hi)[0] / self.norm

    def _sample(self, Y, frame0):
        from flowmse_amd.sampling import get_white_box_solver
        kw = dict(noise_keys=[self.key], noise_seed=self._seed)
        if frame0 is not None:
            kw["noise_frame0"] = [frame0]
        return get_white_box_solver(self._odesolver, self.model.ode, self.model, Y=Y, Y_prior=Y, **self._solver, **kw)()[0]

    def _window_calls(self, Tc, stft_entry, stft_ints, istft_entry, istft_ints, refuse=None):
        """The two window entries of one geometry, bound to its integers: ``stft(lo, hi, k, L_total)`` -> chunk ``k``'s
        ``[1,1,256,Tc]`` rows from the samples ``[lo, hi)``, and ``istft(prev2, prev, cur, k, last, L, e0, e1)`` -> the output
        samples ``[e0, e1)``.  ``stft_ints(k)`` and ``istft_ints`` are what the entries take between the window and
        ``L_total``, and between ``k`` and ``last``; ``refuse(k)`` may raise before anything is read."""
        from flowmse_amd import _lib

        def stft(lo, hi, k, L_total):
            if refuse is not None:
                refuse(k)
            win = self._normalised(lo, hi)
            Y = torch.empty(1, 1, 256, Tc, dtype=torch.complex64, device=self.device)
            _lib.check(getattr(_lib.lib, stft_entry)(_lib.ptr(win), lo, hi - lo, 1.0, *stft_ints(k), L_total, _lib.ptr(Y),
                                                     float(self._dm.spec_factor), float(self._dm.spec_abs_exponent),
                                                     _lib.current_stream()))
            return Y

        def istft(prev2, prev, cur, k, last, L, e0, e1):
            out = torch.empty(e1 - e0, dtype=torch.float32, device=self.device)
            if e1 > e0:                                     # trailing: E_0 = 0 when the fade reaches back to the first frames
                _lib.check(getattr(_lib.lib, istft_entry)(_lib.ptr(prev2), _lib.ptr(prev), _lib.ptr(cur), k, *istft_ints,
                                                          int(last), L, float(self._dm.spec_factor),
                                                          float(self._dm.spec_abs_exponent), _lib.ptr(out), e0, e1 - e0,
                                                          float(self.norm), _lib.current_stream()))
            return out
        return stft, istft

    def _overlap_calls(self, Tc, hop):
        return self._window_calls(Tc, "flowse_stft_compress_window", lambda k: (k * hop, Tc),
                                  "flowse_istft_decompress_window", (Tc, hop))

    def _refuse_past_noise(self, k):
        if k * self.H + self.Tc > NOISE_FRAME_MAX:
            raise ValueError(f"LiveEnhancer: the noise stream is addressed up to frame {NOISE_FRAME_MAX}; chunk {k} ends at "
                             f"stream frame k hop_frames + chunk_frames = {k * self.H + self.Tc}")

    def _chunk(self, k, L, last=False):
        """Sample chunk ``k`` (``L`` None: the recording is open) and return the samples that became final with it."""
        sched = self.sched
        lo = sched.window_lo(k)
        hi = sched.ready_at(k) if L is None else min(sched.ready_at(k), L)
        if L is not None:                                   # the right reflection may read one sample before the first frame
            lo = max(min(lo, L - KEEP), self._buf.s0)
        cur = self._sample(self._stft(lo, hi, k, -1 if L is None else L), sched.noise_frame0(k))
        e0 = self._out16
        e1 = L if last else sched.final_after(k)
        out = self._istft(self._prev2, self._prev, cur, k, last, L if last else 0, e0, e1)
        self._out16 = e1
        self._prev2, self._prev = (self._prev if sched.keep_two else None), cur
        self._k = k + 1
        self._buf.drop(sched.drop_before(k))
        return out

    def _single(self, L, Tpad):
        """K = 1: one row of ``T`` padded to a multiple of 64, the keyed stream from frame 0, every padded frame in the
        overlap-add -- ``enhance_waveform``'s computation through the window entries."""
        stft, istft = self._overlap_calls(Tpad, Tpad)
        out = istft(None, None, self._sample(stft(0, L, 0, L), None), 0, True, L, 0, L)
        self._out16 = L
        self._k = 1
        return out

    def _deliver(self, out, as_tensor, last=False):
        if self._rs_in is None:                             # 16 kHz in and out: the caller's counters are the schedule's
            self.samples_in, self.samples_out = self._in16, self._out16
        elif self._rs_out is None:
            self.samples_out = self._out16
        else:
            out = [self._back(out, last)]
        if not out:
            return torch.empty(0, dtype=torch.float32, device=self.device) if as_tensor else np.empty(0, dtype=np.float32)
        x = out[0] if len(out) == 1 else torch.cat(out)
        return x if as_tensor else x.cpu().numpy()

    def _back(self, out, last):
        """``output_rate="input"``: the emitted 16 kHz samples through the second resampler; at the end its remaining
        outputs, the total trimmed to the input's sample count as ``enhance_recording`` trims.  Before the end the count
        returned stays below ``samples_in`` (an output at the input rate is final later than the input sample under it)."""
        with torch.cuda.device(self.device):
            parts = [self._rs_out.push(out[0] if len(out) == 1 else torch.cat(out), as_tensor=True)] if out else []
            if last:
                parts.append(self._rs_out.finish(as_tensor=True))
        x = torch.cat(parts) if parts else torch.empty(0, dtype=torch.float32, device=self.device)
        x = x[:max(self.samples_in - self.samples_out, 0)]
        self.samples_out += x.numel()
        return x
