"""Sample-rate conversion on the device: recordings at 8 .. 192 kHz in and out of the 16 kHz network.

An opt-in step (``flowmse_amd.enhance --resample``); the reference reads 16 kHz files only.  Rational-ratio polyphase FIR
resampling, zero phase, DEFINED as what ``scipy.signal.resample_poly(x, up, down)`` computes with its defaults
(``window=("kaiser", 5.0)``, ``padtype="constant"``):

    g = gcd(sr_out, sr_in), up = sr_out / g, down = sr_in / g, R = max(up, down), half = 10 R
    h[k]  = up * firwin(2 half + 1, 1 / R, window=("kaiser", 5.0))[k],  k = 0 .. 2 half
    L_out = ceil(L up / down)
    out[n] = sum over m in [0, L) with |n down - m up| <= half of  x[m] h[half + n down - m up]

``R <= 1024`` after reduction: 8 / 11.025 / 12 / 22.05 / 24 / 32 / 44.1 / 48 / 88.2 / 96 / 176.4 / 192 kHz against 16 kHz,
both ways.  The taps come from the library (``flowse_resample_taps``, host only), the device path is one
``flowse_resample_poly`` launch (csrc/resample.hip), and ``resample_reference`` is the float64 restatement the tests hold
against scipy -- nothing here calls scipy.  ``n down`` passes 2^31 five minutes into a 44.1 kHz recording: every index is
a Python int or an int64.

A signal that is still arriving (``flowmse_amd.live`` at 44.1 or 48 kHz) goes through ``StreamResampler``: the same
outputs from a window of the signal, one ``flowse_resample_poly_window`` launch per push; ``stream_plan`` says how many
outputs are final after ``n`` samples.  Several such signals (the channels and sessions of ``flowmse_amd.livepool``) go
through ``RowsResampler`` s and ``flush``: the rows of all of them at one ratio in one
``flowse_resample_poly_window_rows`` launch, ``plan_flush`` being the host side of that grouping.
"""
import ctypes as C
import math

import numpy as np
import torch

from flowmse_amd import _lib

MAX_RATE = 1024
_ROWS = 1 << 16                  # outputs per pass of resample_reference (bounds its [rows, P] work arrays)


def rational(sr_in, sr_out):
    """``(up, down)``, reduced, for a conversion from ``sr_in`` to ``sr_out`` Hz.  ``ValueError``, naming the two rates,
    for non-positive rates and for ratios beyond ``max(up, down) = 1024``."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample: sample rates must be positive, got {sr_in} Hz -> {sr_out} Hz")
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if max(up, down) > MAX_RATE:
        raise ValueError(f"resample: {sr_in} Hz -> {sr_out} Hz is the ratio {up}/{down}; supported up to "
                         f"max(up, down) = {MAX_RATE}")
    return up, down


def out_len(L, up, down):
    """``ceil(L up / down)``: the samples ``L`` input samples become."""
    return -((-int(L) * int(up)) // int(down))


def design_taps(up, down):
    """The ``2 half + 1`` taps ``h`` of a ratio (reduced or not) in float64, from ``flowse_resample_taps``."""
    n = int(_lib.lib.flowse_resample_num_taps(int(up), int(down)))
    if n < 0:
        _lib.check(-n)
    taps = np.empty(n, dtype=np.float64)
    _lib.check(_lib.lib.flowse_resample_taps(int(up), int(down), taps.ctypes.data_as(C.POINTER(C.c_double)), n))
    return taps


def resample_reference(x, sr_in, sr_out, n0=0, n1=None, m0=0):
    """Outputs ``n0 .. n1 - 1`` (default: all) of the formula above in float64, for a 1-D array ``x``.  The polyphase sum
    ``out[n] = sum_j H[p][j] x[q - j]`` with ``c = half + n down``, ``p = c mod up``, ``q = c div up``, built on
    ``design_taps``.  ``m0``: ``x[0]`` is sample ``m0`` of a longer signal -- a window far into a long recording from the
    slice its outputs touch, ``q(n0) - (P - 1) .. q(n1 - 1)``, or from there to the signal's end; samples outside ``x``
    are taken as zero."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError(f"resample_reference takes a 1-D array, got shape {x.shape}")
    up, down = rational(sr_in, sr_out)
    m0 = int(m0)
    L = m0 + x.shape[0]
    n1 = out_len(L, up, down) if n1 is None else int(n1)
    n0 = int(n0)
    if not 0 <= n0 <= n1 <= out_len(L, up, down):
        raise ValueError(f"resample_reference: outputs [{n0}, {n1}) of {out_len(L, up, down)}")
    if up == down:
        return x[n0 - m0:n1 - m0].copy()
    h = design_taps(up, down)
    half = (h.shape[0] - 1) // 2
    P = -(-h.shape[0] // up)
    H = np.zeros(up * P, dtype=np.float64)
    H[:h.shape[0]] = h
    H = np.ascontiguousarray(H.reshape(P, up).T)                   # H[p][j] = h[p + j up]
    j = np.arange(P, dtype=np.int64)
    out = np.empty(n1 - n0, dtype=np.float64)
    for a in range(n0, n1, _ROWS):
        c = half + np.arange(a, min(a + _ROWS, n1), dtype=np.int64) * down
        m = (c // up)[:, None] - j[None, :] - m0                   # index into x
        ok = (m >= 0) & (m < x.shape[0])
        xg = np.where(ok, x[np.where(ok, m, 0)], 0.0)
        out[a - n0:a - n0 + c.shape[0]] = np.einsum("ij,ij->i", H[c % up], xg)
    return out


def resample(sig, sr_in, sr_out):
    """float32 tensor ``[B, L]`` at ``sr_in`` Hz -> ``[B, ceil(L up / down)]`` at ``sr_out`` Hz, every row on its own.
    A HIP tensor: one ``flowse_resample_poly`` launch on the current stream, no host synchronisation.  A CPU tensor: the
    float64 reference rounded to float32 (the oracle composition).  Equal rates return ``sig`` itself."""
    up, down = rational(sr_in, sr_out)
    if up == down:
        return sig
    if sig.dim() != 2 or sig.dtype != torch.float32:
        raise ValueError(f"resample takes a float32 tensor [B, L], got {sig.dtype} {tuple(sig.shape)}")
    B, L = sig.shape
    if not sig.is_cuda:
        rows = [resample_reference(r.numpy(), sr_in, sr_out) for r in sig]
        return torch.from_numpy(np.stack(rows).astype(np.float32))
    sig = sig.contiguous()
    out = torch.empty(B, out_len(L, up, down), dtype=torch.float32, device=sig.device)
    with torch.cuda.device(sig.device):
        _lib.check(_lib.lib.flowse_resample_poly(_lib.ptr(sig), B, L, up, down, _lib.ptr(out), out.size(1),
                                                 _lib.current_stream()))
    return out


# ---- a signal that is still arriving ---------------------------------------------------------------------------
def _geometry(up, down):
    """``(up, down, half, P)`` of a pair, reduced: ``half = 10 max(up, down)``, ``P = ceil((2 half + 1) / up)``."""
    up, down = rational(int(down), int(up))                        # reduces and checks: rational(sr_in, sr_out)
    half = 10 * max(up, down)
    return up, down, half, (2 * half + up) // up


def stream_plan(n_in, up, down, finished=False):
    """How many outputs are final after ``n_in`` samples of a signal.  Output ``n`` reads the samples up to
    ``q(n) = (half + n down) div up``, so while the signal is open it is final iff ``q(n) <= n_in - 1``: the count is
    ``max(0, (n_in up - 1 - half) div down + 1)``.  ``finished``: the signal has ended at ``n_in`` -- ``out_len(n_in)``.
    Equal rates pass samples through: ``n_in``.  Host arithmetic on Python ints."""
    n_in = int(n_in)
    if n_in < 0:
        raise ValueError(f"stream_plan: n_in must be >= 0, got {n_in}")
    up, down, half, _ = _geometry(up, down)
    if up == down:
        return n_in
    if finished:
        return out_len(n_in, up, down)
    return max(0, (n_in * up - 1 - half) // down + 1)


class StreamResampler:
    """``resample`` for ONE row that arrives in pushes of any sizes (empty ones and single samples included).
    **Contract:** the concatenation of everything ``push`` and ``finish`` returned equals
    ``resample(x[None], sr_in, sr_out)[0]`` for the finished signal ``x``, whatever the push sizes.

    On a HIP device the equality is bit for bit: every push that finalises at least one output (``stream_plan``) makes one
    ``flowse_resample_poly_window`` launch on the current stream, whose outputs are those of ``flowse_resample_poly`` by
    construction, and nothing here waits for the device (``as_tensor=True`` returns device tensors; the default copies the
    outputs to numpy).  On the CPU the outputs are ``resample_reference(..., n0, n1, m0)`` rounded to float32: within one
    float32 ulp of ``resample``'s CPU path (the float64 sums are blocked differently), not bit for bit.

    ``device``: where the state lives and the outputs are made; default: the device of the first pushed samples (numpy
    arrays and CPU tensors: the CPU).  State: one linear float32 tensor.  After a push the samples before
    ``q(next output) - (P - 1)`` are dropped; the next output is not final, ``q(next output) >= samples_in``, so at most
    ``P - 1`` samples stay, and the capacity is ``P - 1`` plus the largest push: ``state_bytes()`` follows the largest
    push and does not grow with the recording.  Equal rates pass the samples through untouched.  The first
    call for a ratio on a device uploads the ratio's table: make it outside stream capture."""

    def __init__(self, sr_in, sr_out, device=None):
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.up, self.down = rational(sr_in, sr_out)
        _, _, self.half, self.P = _geometry(self.up, self.down)
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._buf = None
        self.reset()

    def state_bytes(self):
        """Bytes of samples this object holds between pushes (the buffer's capacity)."""
        return 0 if self._buf is None else self._buf.numel() * 4

    def reset(self):
        """Forget the signal; the buffer keeps its capacity."""
        self.samples_in = self.samples_out = 0
        self._m0 = self._n = 0                                     # the buffer holds samples [m0, m0 + n) of the signal
        self._finished = False

    def push(self, samples, as_tensor=False):
        """Append ``samples`` (float32, 1-D or [1, n], n >= 0: numpy, CPU tensor or device tensor) and return the outputs
        that became final: float32 numpy (possibly empty), or with ``as_tensor`` a 1-D tensor on ``device``."""
        if self._finished:
            raise RuntimeError("StreamResampler.push after finish(): call reset() to start another signal")
        x = self._take(samples)
        if self.up == self.down:
            self.samples_in += x.numel()
            self.samples_out += x.numel()
            return x if as_tensor else x.cpu().numpy()
        self._append(x)
        out = self._emit(stream_plan(self.samples_in, self.up, self.down), -1)
        self._drop(max((self.half + self.samples_out * self.down) // self.up - (self.P - 1), 0))
        return out if as_tensor else out.cpu().numpy()

    def finish(self, as_tensor=False):
        """The signal has ended at ``samples_in``: return the remaining outputs, up to ``out_len(samples_in)``."""
        if self._finished:
            raise RuntimeError("StreamResampler.finish called twice: call reset() to start another signal")
        if self.device is None:
            self.device = torch.device("cpu")
        out = self._emit(stream_plan(self.samples_in, self.up, self.down, finished=True), self.samples_in)
        self._finished = True
        self._m0 += self._n
        self._n = 0
        return out if as_tensor else out.cpu().numpy()

    # ---- internals --------------------------------------------------------------------------------------------
    def _take(self, samples):
        if isinstance(samples, np.ndarray):
            samples = torch.from_numpy(np.ascontiguousarray(samples))
        if not torch.is_tensor(samples) or samples.dtype != torch.float32:
            raise TypeError("StreamResampler.push takes float32 samples (numpy array or tensor), got "
                            f"{getattr(samples, 'dtype', type(samples).__name__)}")
        if samples.dim() == 2 and samples.size(0) == 1:
            samples = samples[0]
        if samples.dim() != 1:
            raise ValueError(f"StreamResampler.push takes one row, 1-D or [1, n], got {tuple(samples.shape)}")
        if self.device is None:
            self.device = samples.device
        return samples.to(self.device)

    def _append(self, x):
        n = x.numel()
        if n == 0:
            return
        if self._buf is None or self._n + n > self._buf.numel():   # grow once per new largest push; contents stay in front
            grown = torch.empty(max(self._n, self.P - 1) + n, dtype=torch.float32, device=self.device)
            if self._n:
                grown[:self._n] = self._buf[:self._n]
            self._buf = grown
        self._buf[self._n:self._n + n] = x
        self._n += n
        self.samples_in += n

    def _emit(self, n1, L_total):
        """The outputs [samples_out, n1) from the buffer; ``L_total``: -1 while the signal is open."""
        n0 = self.samples_out
        if n1 <= n0:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        self.samples_out = n1
        if self.device.type != "cuda":
            ref = resample_reference(self._buf[:self._n].numpy(), self.sr_in, self.sr_out, n0, n1, self._m0)
            return torch.from_numpy(ref.astype(np.float32))
        out = torch.empty(n1 - n0, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.flowse_resample_poly_window(_lib.ptr(self._buf), self._m0, self._n, L_total, self.up, self.down,
                                                            _lib.ptr(out), n0, n1 - n0, _lib.current_stream()))
        return out

    def _drop(self, upto):
        """Forget the samples before ``upto``: the rest moves to the front of the same buffer."""
        cut = min(upto, self._m0 + self._n) - self._m0
        if cut <= 0:
            return
        rest = self._buf[cut:self._n].clone()
        self._buf[:rest.numel()] = rest
        self._m0 += cut
        self._n -= cut


# ---- several signals that are still arriving: one launch per ratio ------------------------------------------------
MAX_ROWS = _lib.FLOWSE_MAX_RESAMPLE_ROWS            # the rows one flowse_resample_poly_window_rows launch takes


class RowsResampler:
    """``resample`` for ``rows`` signals that arrive TOGETHER (the channels of a live session): one ``[rows, capacity]``
    float32 buffer under one set of counters.  ``append`` only copies into the buffer; the outputs are made by
    ``flush``, which serves any number of these objects with one ``flowse_resample_poly_window_rows`` launch per ratio and
    ``MAX_ROWS`` rows.  ``push`` and ``finish`` are ``append`` plus ``flush([self])``.

    **Contract** (``StreamResampler``'s, per row): the concatenation of everything the flushes returned for row ``r``
    equals ``resample(x[None], sr_in, sr_out)[0]`` for the row's finished signal -- on a HIP device bit for bit, whatever
    the push sizes (empty ones and single samples included), whenever the flushes happen and whatever else is flushed with
    it.  On the CPU the outputs are ``StreamResampler``'s: ``resample_reference(..., n0, n1, m0)`` rounded to float32.

    State: after a flush the samples before ``q(next output) - (P - 1)`` are dropped, once for all rows; the capacity is
    ``P - 1`` plus the largest backlog between two flushes, per row.  Equal rates pass the samples through."""

    def __init__(self, sr_in, sr_out, rows, device=None):
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.up, self.down = rational(sr_in, sr_out)
        _, _, self.half, self.P = _geometry(self.up, self.down)
        self.rows = int(rows)
        if self.rows < 1:
            raise ValueError(f"RowsResampler: rows must be >= 1, got {rows}")
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._buf = None
        self.reset()

    def state_bytes(self):
        """Bytes of samples this object holds between flushes (the buffer's capacity, all rows)."""
        return 0 if self._buf is None else self._buf.numel() * 4

    def reset(self):
        """Forget the signals; the buffer keeps its capacity."""
        self.samples_in = self.samples_out = 0
        self._m0 = self._n = 0                                     # the buffer holds samples [m0, m0 + n) of every row
        self._finished = False

    @property
    def finished(self):
        return self._finished

    def pending(self, finished=False):
        """The outputs per row the next flush makes (``finished``: the signals end at ``samples_in``): host arithmetic."""
        if self._finished:
            return 0
        return stream_plan(self.samples_in, self.up, self.down, finished=finished) - self.samples_out

    def append(self, samples):
        """Append ``samples``: float32 ``[rows, n]`` (1-D at one row), n >= 0, numpy, CPU or device tensor.  Copies into the
        buffer and nothing else: no launch of the resampler, no synchronisation."""
        if self._finished:
            raise RuntimeError("RowsResampler.append after the signals were finished: call reset() to start others")
        if isinstance(samples, np.ndarray):
            samples = torch.from_numpy(np.ascontiguousarray(samples))
        if not torch.is_tensor(samples) or samples.dtype != torch.float32:
            raise TypeError("RowsResampler.append takes float32 samples (numpy array or tensor), got "
                            f"{getattr(samples, 'dtype', type(samples).__name__)}")
        if samples.dim() == 1 and self.rows == 1:
            samples = samples[None]
        if samples.dim() != 2 or samples.size(0) != self.rows:
            raise ValueError(f"RowsResampler.append takes [{self.rows}, n] samples, got {tuple(samples.shape)}")
        if self.device is None:
            self.device = samples.device
        n = samples.size(1)
        if n == 0:
            return
        if self._buf is None or self._n + n > self._buf.size(1):   # grow once per new largest backlog; contents stay in front
            keep = self.P - 1 if self.up != self.down else 0
            grown = torch.empty(self.rows, max(self._n, keep) + n, dtype=torch.float32, device=self.device)
            if self._n:
                grown[:, :self._n] = self._buf[:, :self._n]
            self._buf = grown
        self._buf[:, self._n:self._n + n] = samples.to(self.device)
        self._n += n
        self.samples_in += n

    def push(self, samples, as_tensor=False):
        """``append`` and ``flush([self])``: the ``[rows, n_new]`` outputs that became final, numpy or a tensor on ``device``."""
        self.append(samples)
        out = flush([self])[0]
        return out if as_tensor else out.cpu().numpy()

    def finish(self, as_tensor=False):
        """The signals have ended at ``samples_in``: the remaining outputs, up to ``out_len(samples_in)``."""
        if self._finished:
            raise RuntimeError("RowsResampler.finish called twice: call reset() to start other signals")
        out = flush([self], finished=[self])[0]
        return out if as_tensor else out.cpu().numpy()

    # ---- what flush() does to a stream ------------------------------------------------------------------------
    def _flushed(self, n1, finished):
        """The outputs up to ``n1`` were made: the counters move and the samples no later output reads are dropped."""
        self.samples_out = n1
        if finished:
            self._finished = True
            self._m0 += self._n
            self._n = 0
            return
        upto = self.samples_in if self.up == self.down else max((self.half + n1 * self.down) // self.up - (self.P - 1), 0)
        cut = min(upto, self._m0 + self._n) - self._m0
        if cut <= 0:
            return
        if cut < self._n:
            rest = self._buf[:, cut:self._n].clone()
            self._buf[:, :rest.size(1)] = rest
        self._m0 += cut
        self._n -= cut


def plan_flush(entries, max_rows=MAX_ROWS):
    """The launches of one ``flush``.  ``entries``: per stream ``(device, up, down, rows, n_new)``.  The rows of the streams
    with ``n_new > 0`` at unequal rates are grouped by ``(device, up, down)``, groups in the order of their first stream and
    rows in stream order; each group is cut into tables of at most ``max_rows`` rows.  Returns ``[((device, up, down),
    [(stream index, row), ...]), ...]``, one launch each.  Host only."""
    groups = {}
    for i, (device, up, down, rows, n_new) in enumerate(entries):
        if n_new > 0 and up != down:
            groups.setdefault((device, int(up), int(down)), []).extend((i, r) for r in range(int(rows)))
    return [(key, rows[a:a + max_rows]) for key, rows in groups.items() for a in range(0, len(rows), max_rows)]


def flush(streams, finished=(), stats=None):
    """Make the outputs that are final in every ``RowsResampler`` of ``streams``; those also in ``finished`` have ended
    and deliver their last outputs.  Returns one float32 ``[rows, n_new]`` tensor per stream, on the stream's device
    (``n_new`` may be 0).  On HIP devices: one ``flowse_resample_poly_window_rows`` launch per table of ``plan_flush`` on the
    current stream, no synchronisation; ``stats["resample_launches"]``, when a dict is given, grows by their number.  CPU
    streams take ``StreamResampler``'s CPU path row by row."""
    streams, ended = list(streams), {id(s) for s in finished}
    if len({id(s) for s in streams}) != len(streams):
        raise ValueError("resample.flush: a stream is named twice")
    if not ended <= {id(s) for s in streams}:
        raise ValueError("resample.flush: finished names a stream that is not among streams")
    todo, outs = [], []
    for s in streams:
        if s._finished:
            raise RuntimeError("resample.flush: a stream was finished before: call reset() to start other signals")
        if s.device is None:
            s.device = torch.device("cpu")
        n1 = stream_plan(s.samples_in, s.up, s.down, finished=id(s) in ended)
        todo.append((n1, id(s) in ended))
        if s.up == s.down:                                         # the samples themselves
            outs.append(s._buf[:, :s._n].clone() if s._n else torch.empty(s.rows, 0, dtype=torch.float32, device=s.device))
        else:
            outs.append(torch.empty(s.rows, n1 - s.samples_out, dtype=torch.float32, device=s.device))
    plan = plan_flush([(s.device, s.up, s.down, s.rows, out.size(1)) for s, out in zip(streams, outs)])
    launches = 0
    for (device, up, down), rows in plan:
        if device.type != "cuda":
            for i, r in rows:
                s, n1 = streams[i], todo[i][0]
                ref = resample_reference(s._buf[r, :s._n].numpy(), s.sr_in, s.sr_out, s.samples_out, n1, s._m0)
                outs[i][r] = torch.from_numpy(ref.astype(np.float32))
            continue
        table = (_lib.flowse_resample_row * len(rows))()
        for d, (i, r) in zip(table, rows):
            s, out = streams[i], outs[i]
            d.win, d.m0, d.n_win = s._buf.data_ptr() + 4 * r * s._buf.size(1), s._m0, s._n
            d.L_total = s.samples_in if todo[i][1] else -1
            d.out, d.n0, d.n_out = out.data_ptr() + 4 * r * out.size(1), s.samples_out, out.size(1)
        with torch.cuda.device(device):
            _lib.check(_lib.lib.flowse_resample_poly_window_rows(table, len(rows), up, down, _lib.current_stream()))
        launches += 1
    for s, (n1, end) in zip(streams, todo):
        s._flushed(n1, end)
    if stats is not None:
        stats["resample_launches"] = stats.get("resample_launches", 0) + launches
    return outs
