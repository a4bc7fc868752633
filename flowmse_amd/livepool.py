"""Live pool: many streams, and the channels of a stream, enhanced as they arrive in sampler calls they share.

``live.LiveEnhancer`` enhances ONE mono stream, every chunk a sampler call of batch width 1.  A ``LivePool`` of width ``W``
holds any number of ``LiveSession`` s of one or more channels each; their pushes only append samples, and ``pool.step()``
samples every chunk that is ready -- rows ``(session, chunk, channel)`` cut into sampler calls of EXACTLY ``W`` rows, the
mechanism of ``flowmse_amd.pooled`` on the live side.  At a fixed batch width a row's result depends neither on its
neighbours nor on its position (tests/test_gpu_model.py::test_full_batch_properties), and every call here has width ``W``.

**Contract.**  For every session, the concatenation over all ``step()`` results is, bit for bit, the ``[C, L]`` waveform that
``pooled.enhance_pooled(model, ..., items=[(name, C, L)], batch=W, noise_seed=seed)`` writes for the finished recording
ALONE, when ``keys[c] = pooled.channel_key(name, c)``, ``norm`` equals the recording's peak over all channels, and the
geometry, solver, ``N``, ``T_rev``, ``t_eps`` and precision are the same -- whatever else is in the pool, however the pushes
are cut and whenever ``step()`` is called.  At ``W = 1`` with one channel these are ``LiveEnhancer``'s bytes.

Readiness, the emitted ranges, the kept chunks and the dropping of old samples are ``live.py``'s, per session (its module
docstring: ``n_k``, ``E_k``, the ``K == 1`` row of ``pad_spec`` width at ``finish()``, two previous chunks at ``To = Tc / 2``);
both ask ``flowmse_amd.schedule.OverlapSchedule``.  What is new is the schedule (``plan_step``, a host function of what the sessions
hold):

* sessions come in the order they were opened; a session's rows are chunk-major, so a chunk's channels are emitted together;
* rows of one width make a bucket: ``Tc``, and each ``K == 1`` width (a ``K == 1`` row of width ``Tc`` shares the ``Tc`` bucket);
  buckets run in ascending width;
* a bucket is cut into calls of exactly ``W`` rows; the last call is filled by repeating its own first row (same window, key
  and ``frame0``) and the fillers' results are dropped: at most ``W - 1`` fillers per bucket and step.  A step with ``r < W``
  ready rows therefore costs a full ``W``-row call -- the price of bytes that do not depend on the load.

Per call: one ``flowse_stft_compress_window_rows`` launch, the unchanged ``get_white_box_solver`` with per-row ``noise_keys`` /
``noise_frame0``, one ``flowse_istft_decompress_window_rows`` launch for the ranges that became final.

Channels.  A session of several channels is normalised by ONE factor (the level balance between them is kept) and its
channels are enhanced independently.  ``norm="first"``: the peak over all channels of the samples ``[0, n_0)`` (of everything
if the stream ends earlier; 1.0 if that peak is 0), read back once, in the first ``step()`` that samples the session.  The
buffer holds the samples divided by ``norm`` -- one elementwise torch division by the Python float, as ``enhance_pooled``
divides the file -- so the rows carry ``scale_in = 1``.

State per session: a ``[C, capacity]`` sample buffer, one or two previous chunks per channel and, at another rate, the
``[C, capacity]`` buffers of its resamplers (``state_bytes()``, per session and per pool).  A finished session whose tail was
delivered is closed, leaves the pool and returns its memory.

Other rates.  ``pool.open(keys, norm, input_rate=HZ, output_rate="16000" | "input")``: every session has its own rates, and a
pool may mix them; the defaults are the 16 kHz path above, which makes the calls it made before.  ``push`` takes samples at
``input_rate`` and still only appends, into the session's ``resample.RowsResampler``; ``SessionPlan`` counts what was pushed,
and its 16 kHz ``samples_in`` is ``resample.stream_plan`` of that count (``out_len`` once finished), so readiness stays a host
query.  ``step()`` then has three stages:

(a) one ``resample.flush`` over the in-resamplers of all sessions: ONE ``flowse_resample_poly_window_rows`` launch per distinct
    ratio and 32 rows, whatever the number of sessions and channels.  The new 16 kHz samples are divided by ``norm`` -- after
    the resampling, as the file mode divides, so a float ``norm`` applies to the 16 kHz signal and ``norm="first"`` is the peak
    over all channels of the resampled ``[0, n_0)`` -- and appended to the session buffer;
(b) the schedule and the sampler calls above, unchanged;
(c) one ``flush`` over the out-resamplers of the sessions with ``output_rate="input"`` that got samples, finishing those that
    closed; such a session gets exactly as many samples back as were pushed (the trim of ``live.LiveEnhancer``).

``stats`` / ``last_step`` count the launches of (a) and (c) as ``resample_launches``: eight mono sessions at 48 kHz in and out
make two per step that samples.  **Contract:** a session's concatenated output is, bit for bit, ``resample(y, rate, 16000)``,
then ``enhance_pooled`` as above on that alone (``norm`` the peak of the resampled recording), then with ``"input"``
``resample(x_hat, 16000, rate)[:, :L]`` -- and so the bytes of a ``resample.StreamResampler`` per channel before and behind a
16 kHz session.  ``session.latency_samples`` is ``live.latency_samples(Tc, input_rate, output_rate, To)``; ``samples_in`` and
``samples_out`` of a session count at its own rates, those of its ``plan`` at 16 kHz.

Out of scope: adaptive width, resampling fused into the STFT rows kernel, ``--streams`` lanes, several GPUs.
"""
import collections

import numpy as np
import torch

from flowmse_amd.chunked import CHUNK_FRAMES, OVERLAP_FRAMES
from flowmse_amd.live import SampleBuffer, check_norm, require_hip_model
from flowmse_amd.resample import RowsResampler, flush, out_len, rational, stream_plan
from flowmse_amd.schedule import HOP, PADC, RATE, OverlapSchedule

MAX_WIDTH = 16                      # FLOWSE_MAX_WINDOW_ROWS: the rows one window launch builds

Row = collections.namedtuple("Row", "session chunk channel frame0 filler")
Call = collections.namedtuple("Call", "width rows")


def check_width(width):
    w = int(width)
    if not 1 <= w <= MAX_WIDTH:
        raise ValueError(f"LivePool: width must be 1..{MAX_WIDTH} (the rows of one window launch), got {width}")
    return w


def check_keys(keys):
    """One 64-bit key, or one per channel -> tuple of ints."""
    if keys is None:
        raise ValueError("LivePool.open: keys is required (keyed noise only; pooled.channel_key makes one per channel)")
    try:
        ks = [keys] if isinstance(keys, (int, np.integer)) else list(keys)
    except TypeError:
        ks = []
    if not ks or not all(isinstance(k, (int, np.integer)) and 0 <= int(k) < 1 << 64 for k in ks):
        raise ValueError(f"LivePool.open: keys is one 64-bit key or a non-empty list of them (one per channel), got {keys!r}")
    return tuple(int(k) for k in ks)


def check_rates(input_rate, output_rate):
    """``(input_rate, up, down)`` of a session: ``up / down`` takes it to 16 kHz.  A ratio ``resample.rational`` does not admit
    and an ``output_rate`` other than ``"16000"`` or ``"input"`` are refused by name."""
    if output_rate not in ("16000", "input"):
        raise ValueError(f"LivePool.open: output_rate is '16000' or 'input', got {output_rate!r}")
    try:
        up, down = rational(input_rate, RATE)
    except (TypeError, ValueError) as e:
        raise ValueError(f"LivePool.open: input_rate {input_rate!r}: {e}")
    return int(input_rate), up, down


class SessionPlan:
    """What the schedule knows of one session: host counters only (no device, no samples).  ``samples_in`` / ``samples_out``
    follow ``live.live_plan`` as a ``LiveEnhancer``'s do, with "sampled" in place of "arrived": ``samples_out`` moves when a
    ``step()`` has sampled the chunk.  Both count at 16 kHz.  ``pushed`` counts what was pushed, at ``input_rate``, and
    ``samples_in`` is what of the 16 kHz signal those samples make final: ``stream_plan(pushed)``, after ``finish()``
    ``out_len(pushed)`` -- at 16 kHz ``pushed`` itself."""

    def __init__(self, keys, norm, chunk_frames=CHUNK_FRAMES, overlap_frames=OVERLAP_FRAMES, input_rate=RATE,
                 output_rate="16000"):
        self.sched = OverlapSchedule(chunk_frames, overlap_frames)
        self.Tc, self.To = self.sched.Tc, self.sched.To
        self.keys = check_keys(keys)
        self.channels = len(self.keys)
        self.norm_arg = check_norm(norm, "LivePool.open")
        self.input_rate, self.up, self.down = check_rates(input_rate, output_rate)
        self.output_rate = output_rate
        self.pushed = self.samples_out = 0
        self.k = 0                                          # next chunk to sample
        self.finished = self.closed = False
        self.L = self.K = None

    @property
    def samples_in(self):
        return stream_plan(self.pushed, self.up, self.down, finished=self.finished)

    @property
    def latency_samples(self):
        """Worst algorithmic latency in samples at ``input_rate`` (``live.latency_samples``)."""
        return self.sched.latency(self.input_rate, self.output_rate)

    def accept(self, shape):
        """A push of ``shape`` ([C, n]; 1-D or [1, n] at one channel): counted, and ``n`` returned."""
        if self.finished:
            raise RuntimeError("LiveSession.push after finish(): open another session for another recording")
        shape = tuple(int(d) for d in shape)
        if len(shape) == 1 and self.channels == 1:
            shape = (1,) + shape
        if len(shape) != 2 or shape[0] != self.channels:
            raise ValueError(f"LiveSession.push takes [{self.channels}, n] samples (this session has {self.channels} "
                             f"channel{'s' if self.channels > 1 else ''}), got {list(shape)}")
        self.pushed += shape[1]
        return shape[1]

    def finish(self):
        if self.finished:
            raise RuntimeError("LiveSession.finish called twice")
        L = out_len(self.pushed, self.up, self.down)
        if L <= PADC:
            raise ValueError(f"LiveSession.finish: a recording needs more than {PADC} samples (n_fft // 2 of the centred "
                             f"STFT), got {L}" + (f" at 16 kHz ({self.pushed} at {self.input_rate} Hz)" if self.up != self.down
                                                  else ""))
        self.finished, self.L = True, L
        self.K = self.sched.chunks(L // HOP + 1)

    def pending(self):
        """``[(chunk, width)]`` that can be sampled now, in order."""
        if self.closed:
            return []
        if not self.finished:
            return [(k, self.Tc) for k in range(self.k, self.sched.plan(self.samples_in)[0])]
        if self.K == 1:                                     # enhance_waveform's one row, T padded to a multiple of 64
            return [] if self.k else [(0, self.sched.single_width(self.L // HOP + 1))]
        return [(k, self.Tc) for k in range(self.k, self.K)]

    def final_after(self, k):
        """Output samples that are final once chunk ``k`` is sampled: ``E_k``, or ``L`` after the last chunk."""
        if self.finished and k == self.K - 1:
            return self.L
        return self.sched.final_after(k)

    def sampled(self, k):
        """Chunk ``k`` was sampled: the counters move, and a finished session whose last chunk it was is closed."""
        self.samples_out = self.final_after(k)
        self.k = k + 1
        if self.finished and self.k == self.K:
            self.closed = True


def plan_step(plans, width):
    """The sampler calls of one ``step()`` (module docstring): ``plans`` is the list of the sessions' ``SessionPlan`` in the
    order they were opened, and nothing else is looked at.  Returns a list of ``Call(width, rows)`` with ``rows`` a list of
    exactly ``width`` ``Row(session, chunk, channel, frame0, filler)``, ``session`` the index into ``plans``."""
    W = check_width(width)
    buckets = {}
    for i, p in enumerate(plans):
        for k, tw in p.pending():
            buckets.setdefault(tw, []).extend(Row(i, k, c, p.sched.noise_frame0(k), False) for c in range(p.channels))   # K == 1: k = 0
    calls = []
    for tw in sorted(buckets):
        rows = buckets[tw]
        for r0 in range(0, len(rows), W):
            group = rows[r0:r0 + W]
            group += [group[0]._replace(filler=True)] * (W - len(group))
            calls.append(Call(tw, group))
    return calls


class LiveSession:
    """One stream of ``C`` channels in a ``LivePool`` (``pool.open``).  ``push`` and ``finish`` only record; the samples
    come back from ``pool.step()``."""

    def __init__(self, pool, keys, norm, input_rate=RATE, output_rate="16000"):
        self.pool = pool
        self.plan = SessionPlan(keys, norm, pool.Tc, pool.To, input_rate, output_rate)
        self.norm = None if isinstance(self.plan.norm_arg, str) else self.plan.norm_arg
        self._buf = SampleBuffer(self.channels, pool.device)  # the samples [s0, s0 + n) of every channel, divided by norm
        self._prev = [None] * self.channels                 # chunk k - 1 (and k - 2) per channel
        self._prev2 = [None] * self.channels
        self._rs_in = self._rs_out = None                   # input_rate != 16000: the resamplers around the 16 kHz path
        self._delivered = 0                                 # output_rate="input": samples returned, at the input rate
        self._back = output_rate == "input" and self.plan.up != self.plan.down
        if self.plan.up != self.plan.down:
            self._rs_in = RowsResampler(self.input_rate, RATE, self.channels, pool.device)
            if self._back:
                self._rs_out = RowsResampler(RATE, self.input_rate, self.channels, pool.device)

    channels = property(lambda self: self.plan.channels)
    keys = property(lambda self: self.plan.keys)
    input_rate = property(lambda self: self.plan.input_rate)
    output_rate = property(lambda self: self.plan.output_rate)
    latency_samples = property(lambda self: self.plan.latency_samples)
    finished = property(lambda self: self.plan.finished)
    closed = property(lambda self: self.plan.closed)

    @property
    def samples_in(self):
        """Samples pushed, at ``input_rate``."""
        return self.plan.pushed

    @property
    def samples_out(self):
        """Samples returned, at the session's output rate."""
        return self._delivered if self._back else self.plan.samples_out

    def state_bytes(self):
        """Device bytes held between steps: the sample buffer (its capacity), the previous chunks and the buffers of the
        resamplers, if any."""
        kept = [c for c in self._prev + self._prev2 if c is not None]
        rs = sum(r.state_bytes() for r in (self._rs_in, self._rs_out) if r is not None)
        return self._buf.capacity * self.channels * 4 + sum(c.numel() * 8 for c in kept) + rs

    def push(self, samples):
        """Append ``samples`` at ``input_rate``: float32 ``[C, n]`` (1-D or ``[1, n]`` at one channel), numpy, CPU or device
        tensor.  No sampler or resampler call and no device synchronisation; returns None."""
        if isinstance(samples, np.ndarray):
            samples = torch.from_numpy(np.ascontiguousarray(samples))
        if not torch.is_tensor(samples) or samples.dtype != torch.float32:
            raise TypeError("LiveSession.push takes float32 samples (numpy array or tensor), got "
                            f"{getattr(samples, 'dtype', type(samples).__name__)}")
        n = self.plan.accept(samples.shape)
        if n == 0:
            return
        samples = samples.reshape(self.channels, n).to(self.pool.device)
        if self._rs_in is not None:                         # the 16 kHz samples come from the next step()'s flush
            self._rs_in.append(samples)
            return
        self._take(samples)

    def _take(self, samples):
        """``[C, n]`` samples of the 16 kHz signal on the device, n > 0: divided by ``norm`` (once it is known) into the buffer."""
        self._buf.append(samples if self.norm is None else samples / self.norm)

    def finish(self):
        """The stream has ended (more than 255 samples at 16 kHz, as everywhere): its remaining chunks become ready."""
        self.plan.finish()

    def _trimmed(self, x):
        """``output_rate="input"``: what the out-resampler made of this step's 16 kHz samples, trimmed so that the total is
        the pushed count, as ``enhance_recording`` trims (``live.LiveEnhancer._back``: before the end nothing is cut, an
        output at the input rate is final later than the input sample under it)."""
        x = x[:, :max(self.plan.pushed - self._delivered, 0)]
        self._delivered += x.size(1)
        return x

    # ---- what step() does to a session ----------------------------------------------------------------------------
    def _fix_norm(self):
        """``norm="first"``: read the peak back, once, and divide what is held (pushes divide from now on)."""
        if self.norm is not None:
            return
        n0 = min(self.plan.sched.ready_at(0), self.plan.samples_in)                  # nothing was dropped yet: s0 == 0
        peak = self._buf.view(0, n0).abs().max().item()
        self.norm = peak if peak > 0.0 else 1.0
        held = self._buf.view(0, self._buf.n)
        held[:] = held / self.norm

    def _release(self):
        self._buf = SampleBuffer(self.channels, self.pool.device)
        self._prev = [None] * self.channels
        self._prev2 = [None] * self.channels
        self._rs_in = self._rs_out = None


class LivePool:
    """Sessions that share sampler calls of ``width`` rows (module docstring).  ``model``: a HIP-backed ``VFModel`` on
    ``device`` (default: the current one); ``seed``: the keyed noise seed of every session, as ``enhance_pooled``'s
    ``noise_seed``.  The precision is the model's."""

    def __init__(self, model, *, width, seed=0, chunk_frames=CHUNK_FRAMES, overlap_frames=OVERLAP_FRAMES, N=5, T_rev=1.0,
                 t_eps=0.03, odesolver="euler", device=None):
        self.width = check_width(width)
        self.sched = OverlapSchedule(chunk_frames, overlap_frames)
        self.Tc, self.To = self.sched.Tc, self.sched.To
        self.device, self._dm = require_hip_model(model, device, "flowmse_amd.livepool")
        self.model = model
        self._solver = dict(N=int(N), T_rev=T_rev, t_eps=t_eps)
        self._odesolver, self._seed = odesolver, int(seed)
        with torch.cuda.device(self.device):
            model.dnn.reserve(self.width, 256, self.Tc)
        self.sessions = []                                  # open sessions, in the order they were opened
        self.stats = dict(steps=0, calls=0, rows=0, fillers=0, resample_launches=0)
        self.last_step = dict(calls=0, rows=0, fillers={}, resample_launches=0)     # fillers: per bucket width

    def open(self, keys, norm, input_rate=RATE, output_rate="16000", hop_frames=None, fade_frames=0):
        """A new session: ``keys`` one 64-bit key, or one per channel; ``norm`` a positive float or ``"first"`` (it applies to
        the 16 kHz signal); ``input_rate``: the rate of what is pushed, any ratio to 16 kHz that ``resample.rational`` admits
        (another is refused here, by name); ``output_rate``: ``"16000"``, or ``"input"`` for as many samples back as were
        pushed, at their rate.  ``hop_frames`` / ``fade_frames`` (the trailing chunks of ``LiveEnhancer``) are refused by name:
        the pool runs the two-chunks-over-a-frame geometry only."""
        if hop_frames is not None or fade_frames:
            raise ValueError(f"LivePool.open: hop_frames={hop_frames} fade_frames={fade_frames}: trailing chunks are not pooled "
                             "(one LiveEnhancer(hop_frames=...) per mono stream runs them)")
        s = LiveSession(self, keys, norm, input_rate, output_rate)
        self.sessions.append(s)
        return s

    @property
    def ready(self):
        """Rows waiting: over the sessions, channels x chunks that can be sampled now."""
        return sum(s.channels * len(s.plan.pending()) for s in self.sessions)

    def state_bytes(self):
        return sum(s.state_bytes() for s in self.sessions)

    def step(self, as_tensor=False):
        """Sample everything that is ready.  Returns ``[(session, float32 [C, n]), ...]`` for the sessions that got samples,
        numpy or with ``as_tensor`` device tensors.  A finished session whose tail was delivered is closed and leaves the
        pool."""
        from flowmse_amd import _lib
        from flowmse_amd.sampling import get_white_box_solver
        sessions = list(self.sessions)
        self.last_step = dict(calls=0, rows=0, fillers={}, resample_launches=0)
        # (a) what was pushed at other rates becomes 16 kHz samples: one launch per ratio and 32 rows, over all sessions
        feeds = [s for s in sessions if s._rs_in is not None and not s._rs_in.finished
                 and (s.plan.finished or s._rs_in.pending() > 0)]
        if feeds:
            with torch.cuda.device(self.device):
                new = flush([s._rs_in for s in feeds], finished=[s._rs_in for s in feeds if s.plan.finished],
                            stats=self.last_step)
                for s, x in zip(feeds, new):
                    if x.size(1):
                        s._take(x)
                    assert s._buf.s0 + s._buf.n == s.plan.samples_in
            self.stats["resample_launches"] += self.last_step["resample_launches"]
        # (b) the sampler calls of everything that is ready
        calls = plan_step([s.plan for s in sessions], self.width)
        self.last_step["calls"] = len(calls)
        if not calls:
            return []
        launched = self.last_step["resample_launches"]
        factor, exponent = float(self._dm.spec_factor), float(self._dm.spec_abs_exponent)
        with torch.cuda.device(self.device):
            # per session: the output of this step, and where each of its chunks lies in it
            outs, at = {}, {}
            for i, s in enumerate(sessions):
                todo = s.plan.pending()
                if not todo:
                    continue
                s._fix_norm()
                e = s.plan.samples_out
                for k, _ in todo:
                    at[i, k] = (e, s.plan.final_after(k))
                    e = at[i, k][1]
                outs[i] = torch.empty(s.channels, e - s.plan.samples_out, dtype=torch.float32, device=self.device)
            stream = _lib.current_stream()
            for call in calls:
                W, Tw = self.width, call.width
                table = (_lib.flowse_window_row * W)()
                for j, r in enumerate(call.rows):
                    s = sessions[r.session]
                    table[j].buf = s._buf.data.data_ptr() + 4 * r.channel * s._buf.capacity
                    table[j].s0, table[j].n, table[j].frame0 = s._buf.s0, s._buf.n, r.frame0
                    table[j].L_total, table[j].scale_in = (s.plan.L if s.plan.finished else -1), 1.0
                Y = torch.empty(W, 1, 256, Tw, dtype=torch.complex64, device=self.device)
                _lib.check(_lib.lib.flowse_stft_compress_window_rows(table, W, Tw, _lib.ptr(Y), factor, exponent, stream))
                sample = get_white_box_solver(self._odesolver, self.model.ode, self.model, Y=Y, Y_prior=Y, **self._solver,
                                              noise_keys=[sessions[r.session].keys[r.channel] for r in call.rows],
                                              noise_seed=self._seed, noise_frame0=[r.frame0 for r in call.rows])()[0]
                real = [(j, r) for j, r in enumerate(call.rows) if not r.filler]
                ranges = (_lib.flowse_window_out * len(real))()
                held = []                                   # the table holds addresses: every chunk it names lives until the launch
                for d, (j, r) in zip(ranges, real):
                    s, c = sessions[r.session], r.channel
                    cur = sample[j].clone()                 # kept as the previous chunk: not a view of the whole call
                    held += [cur, s._prev[c], s._prev2[c]]
                    e0, e1 = at[r.session, r.chunk]
                    out = outs[r.session]
                    d.prev2_c64 = None if s._prev2[c] is None else s._prev2[c].data_ptr()
                    d.prev_c64 = None if s._prev[c] is None else s._prev[c].data_ptr()
                    d.cur_c64 = cur.data_ptr()
                    d.out = out.data_ptr() + 4 * (c * out.size(1) + e0 - s.plan.samples_out)
                    last = s.plan.finished and r.chunk == s.plan.K - 1
                    d.k, d.L, d.e0, d.n_out, d.last, d.scale_out = r.chunk, (s.plan.L if last else 0), e0, e1 - e0, int(last), s.norm
                    s._prev2[c], s._prev[c] = (s._prev[c] if self.sched.keep_two else None), cur
                # a K == 1 row of width Tc rides in the Tc bucket: at k = 0 with the last flag no frame reads the hop
                hop = self.sched.hop if Tw == self.Tc else Tw
                _lib.check(_lib.lib.flowse_istft_decompress_window_rows(ranges, len(real), Tw, hop, factor, exponent, stream))
                del held
                self.last_step["rows"] += len(real)
                self.last_step["fillers"][Tw] = self.last_step["fillers"].get(Tw, 0) + W - len(real)
            # the counters move, the samples behind the next chunk are dropped, finished sessions leave
            back = []
            for i in sorted(outs):
                s = sessions[i]
                for k, _ in s.plan.pending():
                    s.plan.sampled(k)
                if not s.plan.closed:
                    s._buf.drop(self.sched.drop_before(s.plan.k - 1))
                if s._rs_out is not None:
                    s._rs_out.append(outs[i])
                    back.append(i)
            # (c) output_rate="input": what came out goes back to the sessions' rates, again one launch per ratio and 32 rows
            if back:
                new = flush([sessions[i]._rs_out for i in back],
                            finished=[sessions[i]._rs_out for i in back if sessions[i].plan.closed], stats=self.last_step)
                for i, x in zip(back, new):
                    outs[i] = sessions[i]._trimmed(x)
            results = []
            for i in sorted(outs):
                s = sessions[i]
                if s.plan.closed:
                    s._release()
                    self.sessions.remove(s)
                results.append((s, outs[i] if as_tensor else outs[i].cpu().numpy()))
        self.stats["resample_launches"] += self.last_step["resample_launches"] - launched
        self.stats["steps"] += 1
        self.stats["calls"] += len(calls)
        self.stats["rows"] += self.last_step["rows"]
        self.stats["fillers"] += sum(self.last_step["fillers"].values())
        return results
