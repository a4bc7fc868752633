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

Schedule (``n_fft = 510``, ``hop_length = 128``, ``center=True``; ``hop = Tc - To`` is the chunk hop in frames).  Checked
against the index ranges of the kernels (``stft_frame`` reads ``[128 t - 255, 128 t + 254]``, reflected at both ends;
``istft_gather`` puts frame ``t`` over the output samples ``[128 t - 255, 128 t + 254]``):

* Frame ``t`` is computable without right padding once ``128 t + 255`` samples have arrived.
* Chunk ``k`` (frames ``[k hop, k hop + Tc)``) is ready at ``n_k = 128 (k hop + Tc - 1) + 255`` samples.  A chunk that
  became ready this way is never the recording's last: ``L >= n_k`` gives ``L // 128 + 1 > k hop + Tc`` frames.
* Once chunk ``k`` is sampled and is not the last, frames ``< (k + 1) hop`` are final and so are the output samples
  ``s < E_k = 128 (k + 1) hop - 255``; the samples ``[E_{k-1}, E_k)`` (``E_{-1} = 0``) are emitted then.  They lie under
  frames from ``k hop - 3`` on.  With ``Tc - 2 To >= 3`` those are plain frames of chunk ``k - 1``, and chunks ``k - 1`` and
  ``k`` suffice.  With ``To = Tc / 2`` (the only other geometry ``plan_chunks`` admits: ``Tc - 2 To`` is a multiple of 4)
  frames ``k hop - 3 .. k hop - 1`` are BLENDED frames of chunk ``k - 1``, whose other half is chunk ``k - 2``: then two
  previous chunks are kept, and the window entry takes all three.
* Worst algorithmic latency ``n_k - E_{k-1} = 128 Tc + 382`` samples (``latency_samples``): 2.07 s at ``Tc = 256``, 0.54 s at
  ``Tc = 64``.  The sampler's compute time comes on top.
* After chunk ``k`` the samples before ``128 (k + 1) hop - 256`` are dropped (clamped at 0).  One more than chunk ``k + 1``
  reads while the recording is open: if it ends at a multiple of 128 exactly one frame past chunk ``k`` (possible at
  ``To = 0``), that frame's right reflection reads sample ``L - 256``.

``finish()`` fixes ``L`` (``L > 255``, as every call of the package requires) and ``K = plan_chunks(L // 128 + 1, Tc, To)[0]``,
samples the chunks that were waiting for samples that never came -- one or two, in order, at batch width 1, now with the
right reflection and the zero frames ``>= T`` of ``flowse_stft_compress_chunks`` -- and emits ``[E_{last emitted}, L)``.

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
library's ``flowse_stft_compress_trailing_window`` and ``flowse_istft_decompress_trailing_window``.  Schedule, checked against
the same index ranges:

* Chunk ``k`` holds frames ``[k H - P, k H + H)`` (those ``< 0`` are zero: the first chunks are right-aligned, so the latency
  holds from the first sample on) and is ready at ``n_k = 128 (k H + H - 1) + 255`` samples.  A chunk that became ready this
  way is never the last: ``L >= n_k`` gives ``L // 128 + 1 > (k + 1) H`` frames, so ``K = ceil(T / H) >= k + 2``.
* After chunk ``k`` (not the last) frames ``< (k + 1) H - X`` are final -- the ``X`` frames before ``(k + 1) H`` wait for the
  cross-fade into chunk ``k + 1`` -- and so are the samples ``s < E_k = 128 ((k + 1) H - X) - 255``, clamped at 0; the samples
  ``[E_{k-1}, E_k)`` are returned then.  They lie under frames from ``k H - X - 3`` on, which chunk ``k - 1`` owns
  (``(k H - 3) // H = k - 1``); those are plain frames of it when ``H - X >= 3``, and chunk ``k - 1`` suffices as history.
  Otherwise (``(8, 8)``, ``(4, 2)``, ...) they are faded frames whose other half is chunk ``k - 2``: two previous chunks are kept.
* Worst algorithmic latency ``n_k - E_{k-1} = 128 (H + X) + 382`` samples: 0.184 s at ``(16, 4)``, 0.104 s at ``(8, 2)``; the
  sampler's compute time comes on top, and it is spent ``Tc / H`` times as often (``Tc / H`` network rows per ``H`` frames).
* After chunk ``k`` the samples before ``128 ((k + 1) H - P) - 256`` are dropped (clamped at 0): one more than the first
  frame of chunk ``k + 1`` reads, for the same right reflection as above.  Before a push at most ``128 Tc + 382`` samples are
  held, so the buffer is sized to that plus the largest push from the first push on.
* ``finish()`` fixes ``L`` and ``K = ceil(T / H)``, samples the waiting chunks with the right reflection and the zero frames
  ``>= T``, and returns ``[E_last, L)``.  There is no ``K = 1`` case: a recording shorter than one hop is one right-aligned
  chunk.  A stream so long that ``k H + Tc`` passes ``2^31 - 2``, the last frame the keyed noise addresses, is refused by name.
* ``input_rate`` / ``output_rate`` work unchanged through the resamplers around this 16 kHz path, and ``latency_samples`` takes
  the worst case over ``k`` by the method above with this schedule's ``n_k`` and ``E_k``.

Not in this geometry: ``LivePool`` / ``--live_channels`` (trailing rows of several sessions in one call are the obvious
follow-up; ``LivePool.open`` refuses the keywords by name), ``--streams``, several GPUs, ensembles.  ``H`` and ``X`` were not
chosen by listening -- no released checkpoint is at hand -- so the defaults are chosen values, not tuned ones.

Out of scope: ``--streams`` lanes, several GPUs, time-varying or non-rational rates, noise that is not keyed, and any CPU or
oracle path -- the oracle composition is ``enhance_long``'s, and this module is pinned to ``enhance_long``.  Rows of several
sessions pooled into one sampler call, and several channels, are ``flowmse_amd.livepool``'s, which imports this module's
arithmetic; a ``LiveEnhancer`` stays one mono stream at width 1.
"""
import numpy as np
import torch

from flowmse_amd.chunked import CHUNK_FRAMES, NOISE_FRAME_MAX, OVERLAP_FRAMES, plan_chunks, plan_trailing

HOP, PADC = 128, 255                # hop_length and n_fft // 2 of the released STFT, the only one the kernels cover
RATE = 16000                        # the network's sample rate
KEEP = PADC + 1                     # samples kept before the next chunk's first frame centre (module docstring)


def _ready_at(k, Tc, hop):
    """``n_k``: the sample count at which chunk ``k`` is ready."""
    return HOP * (k * hop + Tc - 1) + PADC


def _ready_trailing(k, H):
    """``n_k`` of the trailing schedule: chunk ``k`` ends with frame ``k H + H - 1``."""
    return HOP * (k * H + H - 1) + PADC


def _final_trailing(k, H, X):
    """``E_k`` of the trailing schedule (``E_{-1} = 0``): the output samples final once chunk ``k`` is sampled."""
    return max(HOP * ((k + 1) * H - X) - PADC, 0) if k >= 0 else 0


def live_plan(n_samples, Tc=CHUNK_FRAMES, To=OVERLAP_FRAMES, finished=False, hop_frames=None, fade_frames=0):
    """``(chunks_ready, samples_final)`` after ``n_samples`` samples of a recording (module docstring): how many chunks a
    ``LiveEnhancer`` has sampled and how many output samples it has returned.  ``finished``: the recording has ended at
    ``n_samples`` -- all ``K`` chunks, all samples.  Host arithmetic only; geometry errors are ``plan_chunks``'.  With
    ``hop_frames`` the trailing schedule (``To`` is not read; geometry errors are ``plan_trailing``'s)."""
    n = int(n_samples)
    if n < 0:
        raise ValueError(f"live_plan: n_samples must be >= 0, got {n}")
    if hop_frames is not None:
        H, X = int(hop_frames), int(fade_frames)
        plan_trailing(1, Tc, H, X)
        if finished:
            return plan_trailing(n // HOP + 1, Tc, H, X)[0], n
        if n < _ready_trailing(0, H):
            return 0, 0
        ready = (n - _ready_trailing(0, H)) // (HOP * H) + 1
        return ready, _final_trailing(ready - 1, H, X)
    _, hop, _ = plan_chunks(1, Tc, To)
    if finished:
        return plan_chunks(n // HOP + 1, Tc, To)[0], n
    n0 = _ready_at(0, int(Tc), hop)
    if n < n0:
        return 0, 0
    ready = (n - n0) // (HOP * hop) + 1
    return ready, HOP * ready * hop - PADC


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
    Tc = int(Tc)
    trailing = hop_frames is not None
    if trailing:
        H, X = int(hop_frames), int(fade_frames)
        plan_trailing(1, Tc, H, X)
    if int(input_rate) == RATE:
        return HOP * (H + X) + 382 if trailing else HOP * Tc + 382
    from flowmse_amd.resample import rational, stream_plan
    if not trailing:
        _, hop, _ = plan_chunks(1, Tc, To)
    up, down = rational(input_rate, RATE)
    half = 10 * max(up, down)
    worst = 0
    for k in range(up + 1):
        if trailing:
            arrived = (half + (_ready_trailing(k, H) - 1) * down) // up + 1
            e = _final_trailing(k - 1, H, X)
        else:
            arrived = (half + (_ready_at(k, Tc, hop) - 1) * down) // up + 1
            e = HOP * k * hop - PADC if k else 0
        returned = stream_plan(e, down, up) if output_rate == "input" else e * down // up
        worst = max(worst, arrived - returned)
    return worst


class LiveEnhancer:
    """One recording, enhanced as it arrives (module docstring).  ``model``: a HIP-backed ``VFModel`` on ``device`` (default:
    the current one); ``key`` / ``seed``: the keyed noise stream, as ``enhance_long``'s ``noise_key`` / ``noise_seed``;
    ``norm``: a positive float or ``"first"``.  The precision is the model's (``model.dnn.set_precision``).  ``input_rate``:
    the sample rate of what is pushed (default 16000; any ratio ``resample.rational`` admits); ``output_rate``: ``"16000"``
    returns the network's rate, ``"input"`` the input's (module docstring, "Other rates")."""

    def __init__(self, model, *, norm, key, seed=0, chunk_frames=CHUNK_FRAMES, overlap_frames=OVERLAP_FRAMES, N=5, T_rev=1.0,
                 t_eps=0.03, odesolver="euler", device=None, input_rate=RATE, output_rate="16000", hop_frames=None,
                 fade_frames=0):
        _, self.hop, _ = plan_chunks(1, chunk_frames, overlap_frames)
        self.Tc, self.To = int(chunk_frames), int(overlap_frames)
        self.H = self.X = None                              # hop_frames: the trailing schedule (module docstring)
        if hop_frames is not None:
            plan_trailing(1, chunk_frames, hop_frames, fade_frames)
            self.H, self.X = int(hop_frames), int(fade_frames)
        elif fade_frames:
            raise ValueError(f"LiveEnhancer: fade_frames={fade_frames} needs hop_frames (the trailing schedule)")
        self.input_rate = int(input_rate)
        if output_rate not in ("16000", "input"):
            raise ValueError(f"LiveEnhancer: output_rate is '16000' or 'input', got {output_rate!r}")
        self.output_rate = output_rate
        if self.input_rate != RATE:
            from flowmse_amd.resample import rational
            rational(self.input_rate, RATE)                       # an unsupported ratio is refused here, by name
        if key is None:
            raise ValueError("LiveEnhancer: key is required (keyed noise only; util.noise.utterance_key makes one)")
        if isinstance(norm, str):
            if norm != "first":
                raise ValueError(f"LiveEnhancer: norm is a positive float or 'first', got {norm!r}")
        elif not (float(norm) > 0.0 and np.isfinite(float(norm))):
            raise ValueError(f"LiveEnhancer: norm is a positive float or 'first', got {norm!r}")
        dm = getattr(model, "data_module", None)
        dnn = getattr(model, "dnn", None)
        if not (torch.cuda.is_available() and callable(getattr(model, "rk_sample_", None)) and hasattr(dnn, "reserve")):
            raise RuntimeError("flowmse_amd.live runs on the MI355X HIP kernels only: a HIP-backed VFModel on a 'cuda' device "
                               "(there is no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"flowmse_amd.live runs on the MI355X HIP kernels only, got device {self.device} (there is no "
                               "CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not (hasattr(dm, "fused_ok") and dm.fused_ok(torch.empty(0, device=self.device))):
            raise RuntimeError("flowmse_amd.live needs the HIP spectrogram kernels: the released STFT configuration (n_fft 510, "
                               "hop 128, hann, 'exponent')")
        self.model, self._dm = model, dm
        self._norm_arg = norm if isinstance(norm, str) else float(norm)
        self._solver = dict(N=int(N), T_rev=T_rev, t_eps=t_eps)
        self._odesolver, self._seed = odesolver, int(seed)
        self._keep_two = self.Tc - 2 * self.To < 3          # To = Tc / 2: the emitted range reaches a blended frame of chunk k-1
        if self.H is not None:
            self._keep_two = self.H - self.X < 3
        with torch.cuda.device(self.device):
            dnn.reserve(1, 256, self.Tc)
        self._buf = torch.empty(0, dtype=torch.float32, device=self.device)
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
        return latency_samples(self.Tc, self.input_rate, self.output_rate, self.To, self.H, self.X or 0)

    def state_bytes(self):
        """Device bytes this object holds between pushes: the sample buffer (its capacity), the previous chunks and the
        buffers of the resamplers, if any.  No output is pending between calls.  The model's workspace is the model's
        (``reserve(1, 256, Tc)``)."""
        kept = [c for c in (self._prev, self._prev2) if c is not None]
        rs = sum(r.state_bytes() for r in (self._rs_in, self._rs_out) if r is not None)
        return self._buf.numel() * 4 + sum(c.numel() * 8 for c in kept) + rs

    def reset(self, key=None):
        """Forget the recording (the buffer keeps its capacity); ``key``: the next recording's, default the same one."""
        if key is not None:
            self.key = int(key)
        self.samples_in = self.samples_out = 0              # at the caller's rates
        self._in16 = self._out16 = 0                        # at 16 kHz: what the chunk schedule counts
        for r in (self._rs_in, self._rs_out):
            if r is not None:
                r.reset()
        self._s0 = self._n = 0                              # the buffer holds samples [s0, s0 + n) of the recording
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
            if self.H is not None:
                while self._in16 >= _ready_trailing(self._k, self.H):
                    out.append(self._chunk_trailing(self._k, None))
            while self.H is None and self._in16 >= _ready_at(self._k, self.Tc, self.hop):
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
        if self.H is not None:
            K = plan_trailing(L // HOP + 1, self.Tc, self.H, self.X)[0]
        else:
            K = plan_chunks(L // HOP + 1, self.Tc, self.To)[0]
        out = []
        with torch.cuda.device(self.device):
            if self.H is not None:                          # no K = 1 case: a short recording is one right-aligned chunk
                while self._k < K:
                    out.append(self._chunk_trailing(self._k, L, last=self._k == K - 1))
            elif K == 1:                                   # chunk 0 never became ready: enhance_waveform's one padded row
                out.append(self._single(L))
            else:
                while self._k < K:
                    out.append(self._chunk(self._k, L, last=self._k == K - 1))
        self._finished = True
        self._prev = self._prev2 = None
        self._s0 += self._n
        self._n = 0
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
        n = samples.numel()
        if n == 0:
            return
        if self._n + n > self._buf.numel():                 # grow once per new largest push; contents move to the front
            size = self._n + n
            if self.H is not None:                          # before a push at most n_k - 1 - (128 (k H - P) - 256) samples are held,
                size = max(size, HOP * self.Tc + 382 + n)   # whatever k: the capacity follows the largest push from the first one on
            grown = torch.empty(size, dtype=torch.float32, device=self.device)
            grown[:self._n] = self._buf[:self._n]
            self._buf = grown
        self._buf[self._n:self._n + n] = samples.to(self.device)
        self._n += n
        self._in16 += n

    def _normalised(self, lo, hi):
        """Samples [lo, hi) of the recording divided by ``norm`` as ``enhance_long`` divides them: on the device, one
        elementwise torch division by the Python float."""
        if self.norm is None:                               # norm="first": the peak of [0, n_0), or of all there is
            n0 = _ready_at(0, self.Tc, self.hop) if self.H is None else _ready_trailing(0, self.H)
            n0 = min(n0, self._in16)
            peak = self._buf[:n0].abs().max().item()
            self.norm = peak if peak > 0.0 else 1.0
        return self._buf[lo - self._s0:hi - self._s0] / self.norm

    def _sample(self, Y, frame0):
        from flowmse_amd.sampling import get_white_box_solver
        kw = dict(noise_keys=[self.key], noise_seed=self._seed)
        if frame0 is not None:
            kw["noise_frame0"] = [frame0]
        return get_white_box_solver(self._odesolver, self.model.ode, self.model, Y=Y, Y_prior=Y, **self._solver, **kw)()[0]

    def _stft(self, lo, hi, frame0, Tc, L_total):
        from flowmse_amd import _lib
        win = self._normalised(lo, hi)
        Y = torch.empty(1, 1, 256, Tc, dtype=torch.complex64, device=self.device)
        _lib.check(_lib.lib.flowse_stft_compress_window(_lib.ptr(win), lo, hi - lo, 1.0, frame0, Tc, L_total, _lib.ptr(Y),
                                                        float(self._dm.spec_factor), float(self._dm.spec_abs_exponent),
                                                        _lib.current_stream()))
        return Y

    def _istft(self, prev2, prev, cur, k, Tc, hop, last, L, e0, e1):
        from flowmse_amd import _lib
        out = torch.empty(e1 - e0, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib.flowse_istft_decompress_window(_lib.ptr(prev2), _lib.ptr(prev), _lib.ptr(cur), k, Tc, hop,
                                                           int(last), L, float(self._dm.spec_factor),
                                                           float(self._dm.spec_abs_exponent), _lib.ptr(out), e0, e1 - e0,
                                                           float(self.norm), _lib.current_stream()))
        return out

    def _chunk(self, k, L, last=False):
        """Sample chunk ``k`` (``L`` None: the recording is open) and return the samples that became final with it."""
        Tc, hop = self.Tc, self.hop
        lo = max(HOP * k * hop - PADC, 0)
        hi = _ready_at(k, Tc, hop) if L is None else min(_ready_at(k, Tc, hop), L)
        if L is not None:                                   # the right reflection may read one sample before the first frame
            lo = max(min(lo, L - KEEP), self._s0)
        cur = self._sample(self._stft(lo, hi, k * hop, Tc, -1 if L is None else L), k * hop)
        e0 = self._out16
        e1 = L if last else HOP * (k + 1) * hop - PADC
        out = self._istft(self._prev2, self._prev, cur, k, Tc, hop, last, L if last else 0, e0, e1)
        self._out16 = e1
        self._prev2, self._prev = (self._prev if self._keep_two else None), cur
        self._k = k + 1
        self._drop(max(HOP * (k + 1) * hop - KEEP, 0))
        return out

    def _chunk_trailing(self, k, L, last=False):
        """``_chunk`` on the trailing schedule: chunk ``k`` = frames ``[k H - P, k H + H)``, the keyed stream at ``k H``."""
        from flowmse_amd import _lib
        Tc, H, X = self.Tc, self.H, self.X
        if k * H + Tc > NOISE_FRAME_MAX:
            raise ValueError(f"LiveEnhancer: the noise stream is addressed up to frame {NOISE_FRAME_MAX}; chunk {k} ends at "
                             f"stream frame k hop_frames + chunk_frames = {k * H + Tc}")
        lo = max(HOP * max(k * H - (Tc - H), 0) - PADC, 0)
        hi = _ready_trailing(k, H) if L is None else min(_ready_trailing(k, H), L)
        if L is not None:                                   # the right reflection may read one sample before the first frame
            lo = max(min(lo, L - KEEP), self._s0)
        win = self._normalised(lo, hi)
        Y = torch.empty(1, 1, 256, Tc, dtype=torch.complex64, device=self.device)
        _lib.check(_lib.lib.flowse_stft_compress_trailing_window(_lib.ptr(win), lo, hi - lo, 1.0, k, Tc, H,
                                                                 -1 if L is None else L, _lib.ptr(Y),
                                                                 float(self._dm.spec_factor), float(self._dm.spec_abs_exponent),
                                                                 _lib.current_stream()))
        cur = self._sample(Y, k * H)
        e0 = self._out16
        e1 = L if last else _final_trailing(k, H, X)
        out = torch.empty(e1 - e0, dtype=torch.float32, device=self.device)
        if e1 > e0:                                         # E_0 = 0 when the fade reaches back to the first frames
            _lib.check(_lib.lib.flowse_istft_decompress_trailing_window(
                _lib.ptr(self._prev2), _lib.ptr(self._prev), _lib.ptr(cur), k, Tc, H, X, int(last), L if last else 0,
                float(self._dm.spec_factor), float(self._dm.spec_abs_exponent), _lib.ptr(out), e0, e1 - e0, float(self.norm),
                _lib.current_stream()))
        self._out16 = e1
        self._prev2, self._prev = (self._prev if self._keep_two else None), cur
        self._k = k + 1
        self._drop(max(HOP * ((k + 1) * H - (Tc - H)) - KEEP, 0))
        return out

    def _single(self, L):
        """K = 1: one row of ``T`` padded to a multiple of 64, the keyed stream from frame 0, every padded frame in the
        overlap-add -- ``enhance_waveform``'s computation through the window entries."""
        Tpad = -(-(L // HOP + 1) // 64) * 64
        cur = self._sample(self._stft(0, L, 0, Tpad, L), None)
        out = self._istft(None, None, cur, 0, Tpad, Tpad, True, L, 0, L)
        self._out16 = L
        self._k = 1
        return out

    def _drop(self, upto):
        """Forget the samples before ``upto``: the rest moves to the front of the same buffer."""
        cut = min(upto, self._s0 + self._n) - self._s0
        if cut <= 0:
            return
        rest = self._buf[cut:self._n].clone()
        self._buf[:rest.numel()] = rest
        self._s0 += cut
        self._n -= cut

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
