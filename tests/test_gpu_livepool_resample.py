"""GPU: the live pool at other sample rates -- ``flowse_resample_poly_window_rows`` against the single-window entry bit for
bit in every launch form, and its errors; the device ``RowsResampler`` / ``resample.flush`` against ``resample`` of the
finished signals bit for bit; ``LivePool`` sessions at 48, 44.1 and 16 kHz in one pool against the file-mode composition
(``resample`` -> ``enhance_pooled(batch=W)`` -> ``resample`` back, trimmed) and against the arrangement it replaces (a
``StreamResampler`` per channel before and behind a 16 kHz session), bit for bit; bf16; ``norm="first"``; bounded state; the
launch counts; ``--live --live_channels 2 --live_rate 48000 --live_resample`` in one child process under its own time limit.
The full network at Tc = 64, N = 2, as tests/test_gpu_livepool.py.  No test asserts a time."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _cases as C
from flowmse_amd import _lib
from flowmse_amd.chunked import plan_chunks
from flowmse_amd.live import latency_samples, pcm_decode, pcm_deinterleave, pcm_encode, pcm_interleave
from flowmse_amd.livepool import LivePool
from flowmse_amd.pooled import channel_key, enhance_pooled
from flowmse_amd.resample import RowsResampler, StreamResampler, flush, out_len, rational, resample
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
SEED = 0x1F2E3D4C5B6A7988
KW = dict(N=2, T_rev=0.9, t_eps=0.04, odesolver="euler")


# ---------------------------------------------------------------------------------------------------- 1
def _form(up, down):
    """(half, P, run, span staged, table in LDS): csrc/resample.hip's launch_form, restated."""
    half = 10 * max(up, down)
    P = (2 * half + up) // up
    span = lambda run: ((run - 1) * down + up - 1) // up + P
    run = 1024 if span(1024) <= 5120 else 256
    return half, P, run, span(run) <= 5120, up * P <= 10240


def _reads(n0, n1, up, down, length):
    """[lo, hi): the samples the outputs [n0, n1) read -- q(n0) - (P - 1) .. q(n1 - 1), clamped to the signal (``length``
    None: it is open)."""
    half, P = _form(up, down)[:2]
    lo = max((half + n0 * down) // up - (P - 1), 0)
    hi = (half + (n1 - 1) * down) // up + 1
    return lo, hi if length is None else min(hi, length)


def _single(win, m0, Lt, up, down, n0, n_out):
    out = torch.full((n_out,), 7.0, device="cuda")
    _lib.check(L.flowse_resample_poly_window(_lib.ptr(win), m0, win.numel(), Lt, up, down, _lib.ptr(out), n0, n_out,
                                             _lib.current_stream()))
    return out


def _table(rows, outs):
    """rows: (win, m0, L_total, n0, n_out)."""
    table = (_lib.flowse_resample_row * max(len(rows), 1))()
    for d, (win, m0, Lt, n0, n_out), out in zip(table, rows, outs):
        d.win, d.m0, d.n_win, d.L_total, d.out, d.n0, d.n_out = win.data_ptr(), m0, win.numel(), Lt, out.data_ptr(), n0, n_out
    return table


def _rows_call(rows, outs, up, down):
    return L.flowse_resample_poly_window_rows(_table(rows, outs), len(rows), up, down, _lib.current_stream())


FORMS = [(1, 3, True, True), (3, 1, True, True), (160, 441, True, True), (441, 160, True, True), (640, 441, True, False),
         (1, 32, False, True), (1, 600, False, False)]


@pytest.mark.parametrize("up,down,x_lds,h_lds", FORMS, ids=lambda v: str(v))
def test_rows_entry_is_the_single_window_entry(up, down, x_lds, h_lds):
    half, P, run, xs, hs = _form(up, down)
    assert (xs, hs) == (x_lds, h_lds)
    big = 2 * run + 100                                             # more than two runs, beside a row of three outputs
    n = -(-(big + 700) * down // up) + 50
    x = torch.randn(n, generator=torch.Generator().manual_seed(up + down)).cuda()
    total = out_len(n, up, down)
    mid = big + 300
    assert total > mid + 300

    def row(n0, n_out, closed, src=x):
        lo, hi = _reads(n0, n0 + n_out, up, down, n if closed else None)
        assert hi <= n
        return (src[lo:hi].clone(), lo, n if closed else -1, n0, n_out)

    lo_s, hi_s = _reads(mid - 200, mid + 200, up, down, None)
    shared = x[lo_s:hi_s].clone()                                   # two rows name this buffer
    far = 2 ** 33 + 12345                                           # a short window far into an open signal
    lo_f, hi_f = _reads(far, far + 5, up, down, None)
    xf = torch.randn(hi_f - lo_f, generator=torch.Generator().manual_seed(7)).cuda()
    rows = [row(0, big, False),                                                # open, from the signal's start
            row(mid, 3, False),                                                # three outputs, m0 > 0
            row(total - 150, 150, True),                                       # closed: zeros past L_total
            (shared, lo_s, -1, mid - 200, 90),                                 # one buffer ...
            (shared, lo_s, -1, mid + 100, 100),                                # ... twice
            (x[:10].clone(), 0, -1, 10 ** 6, 0),                               # no outputs: legal, skipped
            (xf, lo_f, -1, far, 5),                                            # n0 beyond 2^33
            row(total - 1, 1, True)]
    assert rows[1][1] > 0 and lo_f > 2 ** 31 and rows[2][1] + rows[2][0].numel() == n
    want = [_single(*r[:3], up, down, *r[3:]) if r[4] else torch.empty(0, device="cuda") for r in rows]
    assert all(float(w.abs().max()) > 0 and not bool((w == 7.0).any()) for w in want if w.numel())
    outs = [torch.full((r[4] + 16,), 7.0, device="cuda") for r in rows]
    _lib.check(_rows_call(rows, outs, up, down))
    torch.cuda.synchronize()
    for r, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o[:w.numel()], w) and bool((o[w.numel():] == 7.0).all()), (r, int((o[:w.numel()] != w).sum()))
    # an unreduced pair is the reduced one; R = 1; R = 32
    one = [torch.full((big + 16,), 7.0, device="cuda")]
    _lib.check(_rows_call(rows[:1], one, 3 * up, 3 * down))
    many = [rows[i % len(rows)] for i in range(32)]
    outs32 = [torch.full((r[4] + 16,), 7.0, device="cuda") for r in many]
    _lib.check(_rows_call(many, outs32, up, down))
    torch.cuda.synchronize()
    assert torch.equal(one[0][:big], want[0]) and bool((one[0][big:] == 7.0).all())
    for i, o in enumerate(outs32):
        w = want[i % len(rows)]
        assert torch.equal(o[:w.numel()], w) and bool((o[w.numel():] == 7.0).all()), i
    # refusals: nothing is written anywhere
    for o in outs:
        o.fill_(7.0)
    win, m0, Lt, n0, n_out = rows[1]
    for r, short in ((1, (win[1:].clone(), m0 + 1, Lt, n0, n_out)), (3, (win[:-1].clone(), m0, Lt, n0, n_out))):
        bad = list(rows)
        bad[r] = short
        assert _rows_call(bad, outs, up, down) == ERR_SHAPE
        msg = L.flowse_last_error()
        assert b"flowse_resample_poly_window_rows" in msg and f"row {r}".encode() in msg and str(short[1]).encode() in msg
    s = _lib.current_stream()
    for R in (0, 33):
        assert L.flowse_resample_poly_window_rows(_table(many + many[:1], outs32 + outs32[:1]), R, up, down, s) == ERR_SHAPE
    assert L.flowse_resample_poly_window_rows(None, 3, up, down, s) == ERR_ARG
    table = _table(rows, outs)
    table[2].win = None
    assert L.flowse_resample_poly_window_rows(table, len(rows), up, down, s) == ERR_ARG and b"row 2" in L.flowse_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)


def test_rows_entry_at_equal_rates_copies_per_row():
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1)).cuda()
    rows = [(x[200:700].clone(), 2 ** 40 + 200, -1, 2 ** 40 + 250, 100), (x[:10].clone(), 0, -1, 5, 0), (x[:50].clone(), 0, 50, 40, 10)]
    outs = [torch.full((r[4] + 4,), 7.0, device="cuda") for r in rows]
    _lib.check(_rows_call(rows, outs, 48000, 48000))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:100], x[250:350]) and torch.equal(outs[2][:10], x[40:50])
    assert all(bool((o[r[4]:] == 7.0).all()) for o, r in zip(outs, rows))
    for o in outs:
        o.fill_(7.0)
    bad = list(rows)
    bad[2] = (x[:50].clone(), 0, 50, 45, 10)                        # [45, 55) passes the window's end
    assert _rows_call(bad, outs, 5, 5) == ERR_SHAPE and b"row 2" in L.flowse_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)


# ---------------------------------------------------------------------------------------------------- 2
def _patterns(n, seed, block=2048):
    """Push sizes that sum to n: all at once; blocks; seeded random sizes with empty and single-sample pushes."""
    rng = np.random.default_rng(seed)
    rand, done = [0, 1, 1, 0], 2
    while done < n:
        s = min(int(rng.choice([0, 1, 2, 17, 300, 1000, 5000])), n - done)
        rand.append(s)
        done += s
    rand.append(0)
    return {"whole": [n], "blocks": [min(block, n - i) for i in range(0, n, block)], "random": rand}


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (44100, 16000), (16000, 48000), (16000, 44100)], ids=lambda v: str(v))
def test_rows_resampler_is_resample_bit_for_bit(sr_in, sr_out):
    up, down = rational(sr_in, sr_out)
    n = 20001
    x = torch.randn(2, n, generator=torch.Generator().manual_seed(sr_in + sr_out))
    want = resample(x.cuda(), sr_in, sr_out)
    for how, (name, sizes) in enumerate(_patterns(n, sr_in).items()):
        rs = RowsResampler(sr_in, sr_out, 2, device="cuda")
        parts, done = [], 0
        for i, s in enumerate(sizes):
            piece = x[:, done:done + s]
            parts.append(rs.push((piece.numpy(), piece, piece.cuda())[(how + i) % 3], as_tensor=True))
            done += s
        parts.append(rs.finish(as_tensor=True))
        assert all(p.is_cuda and p.dtype == torch.float32 and p.shape[0] == 2 for p in parts)
        got = torch.cat(parts, dim=1)
        assert rs.samples_out == got.size(1) == out_len(n, up, down) and rs.finished
        assert torch.equal(got, want), (name, int((got != want).sum()))
        assert rs.state_bytes() <= 4 * 2 * (rs.P - 1 + max(sizes))
    assert float(want.abs().max()) > 0
    rs.reset()                                                      # numpy out by default, and the object starts again
    assert np.array_equal(np.concatenate([rs.push(x[:, :9000].numpy()), rs.push(x[:, 9000:]), rs.finish()], axis=1),
                          want.cpu().numpy())


def test_flush_makes_one_launch_per_ratio():
    """Streams of three ratios (two of them share one) flushed together, whatever each has pending."""
    n = 12000
    spec = [(48000, 16000, 2), (44100, 16000, 1), (16000, 48000, 2), (48000, 16000, 1)]
    xs = [torch.randn(c, n, generator=torch.Generator().manual_seed(i)) for i, (_, _, c) in enumerate(spec)]
    want = [resample(x.cuda(), a, b) for x, (a, b, _) in zip(xs, spec)]
    streams = [RowsResampler(a, b, c, device="cuda") for a, b, c in spec]
    parts, done = [[] for _ in spec], [0] * 4
    stats = {}
    first = flush(streams, stats=stats)                             # nothing was pushed: no launch
    assert stats == {"resample_launches": 0} and all(o.shape == (c, 0) for o, (_, _, c) in zip(first, spec))
    sizes = [(1500, 700, 1, 3000), (0, 2500, 900, 1), (4000, 1, 0, 2000)]
    rounds = 0
    while min(done) < n:
        before = stats["resample_launches"]
        for i, s in enumerate(streams):
            k = sizes[rounds % 3][i]
            s.append(xs[i][:, done[i]:done[i] + k].cuda())
            done[i] = min(done[i] + k, n)
        ratios = {(s.up, s.down) for s in streams if s.pending() > 0}
        for p, o in zip(parts, flush(streams, stats=stats)):
            p.append(o)
        assert stats["resample_launches"] - before == len(ratios) <= 3
        rounds += 1
    assert rounds > 5
    for p, o in zip(parts, flush(streams, finished=streams, stats=stats)):
        p.append(o)
    for i, p in enumerate(parts):
        got = torch.cat(p, dim=1)
        assert torch.equal(got, want[i]), (i, got.shape, want[i].shape)
    # 40 rows of one ratio: two tables
    wide = RowsResampler(48000, 16000, 40, device="cuda")
    x = torch.randn(40, 3000, generator=torch.Generator().manual_seed(9))
    wide.append(x)
    stats = {}
    a = flush([wide], stats=stats)[0]
    b = flush([wide], finished=[wide], stats=stats)[0]
    assert stats["resample_launches"] == 4 and torch.equal(torch.cat([a, b], dim=1), resample(x.cuda(), 48000, 16000))


# ---------------------------------------------------------------------------------------------------- 3
def _model(cfg):
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **cfg)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def full():
    assert torch.cuda.is_available()
    return _model(C.FULL)


def _signal(seed, n, channels=1, std=0.1):
    return torch.from_numpy(synth.normal(seed, 9, (channels, n), std))


W, TC, TO = 4, 64, 16
# name -> (signal, rate, output_rate): stereo 48 kHz in and out, mono 44.1 kHz to 16 kHz, mono 16 kHz, a short K == 1 at 48 kHz
RECORDINGS = {"a.wav": (_signal(1, 120000, 2), 48000, "input"), "b.wav": (_signal(2, 100000), 44100, "16000"),
              "c.wav": (_signal(3, 33000), 16000, "16000"), "d.wav": (_signal(4, 15000), 48000, "input")}
_ORACLE = {}


def _composition(model, name, tag="fp32"):
    """The file mode: resample to 16 kHz, ``enhance_pooled(batch=W)`` on the recording alone, resample back and trim.
    Returns (waveform, the peak of the resampled recording); computed once per recording and precision."""
    if (name, tag) not in _ORACLE:
        y, rate, mode = RECORDINGS[name]
        y16 = resample(y.cuda(), rate, 16000)
        got = {}
        enhance_pooled(model, lambda i: y16, [(name, y16.size(0), y16.size(1))], lambda i, x: got.update(x=x.cpu().numpy()),
                       batch=W, chunk_frames=TC, overlap_frames=TO, noise_seed=SEED, **KW)
        x = got["x"]
        if mode == "input" and rate != 16000:
            x = resample(torch.from_numpy(x).cuda(), 16000, rate)[:, :y.size(1)].cpu().numpy()
        _ORACLE[name, tag] = (x, y16.abs().max().item())
    return _ORACLE[name, tag]


def _block(block, rate, rounds):
    if block == "ones":
        return 1 if rounds < 200 else 4097 * rate // 16000
    return block * rate // 16000


def _run_pool(model, norms, block, step_when):
    """Push the recordings round-robin in blocks (counted at 16 kHz, scaled to every session's rate); ``step_when(pool)`` says
    after a round whether to step.  Returns ({name: [C, L]}, pool)."""
    pool = LivePool(model, width=W, seed=SEED, chunk_frames=TC, overlap_frames=TO, **KW)
    sess, parts, done = {}, {}, {}
    for name, (sig, rate, mode) in RECORDINGS.items():
        keys = [channel_key(name, c) for c in range(sig.size(0))]
        s = pool.open(keys, norms[name]) if rate == 16000 else pool.open(keys, norms[name], input_rate=rate, output_rate=mode)
        assert s.latency_samples == latency_samples(TC, rate, mode, TO) and (s.input_rate, s.output_rate) == (rate, mode)
        sess[name], parts[s], done[name] = s, [], 0

    def step():
        for s, x in pool.step():
            assert x.dtype == np.float32 and x.shape[0] == s.channels
            parts[s].append(x)
            assert s.samples_out == sum(p.shape[1] for p in parts[s]) <= (s.samples_in if s.output_rate == "input" else 1 << 40)

    how = rounds = 0
    while any(not s.finished for s in sess.values()):
        for name, (sig, rate, mode) in RECORDINGS.items():
            s = sess[name]
            if s.finished:
                continue
            if done[name] == sig.size(1):
                s.finish()
                continue
            piece = sig[:, done[name]:done[name] + _block(block, rate, rounds)]
            if sig.size(0) == 1 and how % 3 == 0:
                piece = piece[0]
            assert s.push(piece.numpy() if how % 3 < 2 else piece.cuda()) is None
            done[name] += piece.shape[-1]
            assert s.samples_in == done[name]
            how += 1
        rounds += 1
        if step_when(pool):
            step()
    while pool.ready:
        step()
    assert not pool.sessions and pool.state_bytes() == 0
    return {n: np.concatenate(parts[s], axis=1) for n, s in sess.items()}, pool


def _run_parent(model, norms, block):
    """The arrangement this replaces: 16 kHz sessions, a ``StreamResampler`` per channel before and behind them."""
    pool = LivePool(model, width=W, seed=SEED, chunk_frames=TC, overlap_frames=TO, **KW)
    sess, parts, done, front, behind = {}, {}, {}, {}, {}
    for name, (sig, rate, mode) in RECORDINGS.items():
        s = pool.open([channel_key(name, c) for c in range(sig.size(0))], norms[name])
        sess[name], parts[s], done[name] = s, [], 0
        front[s] = [StreamResampler(rate, 16000, "cuda") for _ in range(sig.size(0))] if rate != 16000 else None
        behind[s] = [StreamResampler(16000, rate, "cuda") for _ in range(sig.size(0))] if rate != 16000 and mode == "input" else None

    def step():
        for s, x in pool.step(as_tensor=True):
            if behind[s] is not None:
                rows = [[r.push(x[c], as_tensor=True)] + ([r.finish(as_tensor=True)] if s.closed else []) for c, r in enumerate(behind[s])]
                x = torch.stack([torch.cat(r) for r in rows])
            parts[s].append(x.cpu().numpy())

    while any(not s.finished for s in sess.values()):
        for name, (sig, rate, mode) in RECORDINGS.items():
            s = sess[name]
            if s.finished:
                continue
            if done[name] == sig.size(1):
                if front[s] is not None:
                    s.push(torch.stack([r.finish(as_tensor=True) for r in front[s]]))
                s.finish()
                continue
            piece = sig[:, done[name]:done[name] + _block(block, rate, 0)].cuda()
            done[name] += piece.shape[-1]
            s.push(piece if front[s] is None else torch.stack([r.push(piece[c], as_tensor=True) for c, r in enumerate(front[s])]))
        step()
    while pool.ready:
        step()
    return {n: np.concatenate(parts[s], axis=1)[:, :(RECORDINGS[n][0].size(1) if behind[s] is not None else None)]
            for n, s in sess.items()}


def test_pool_at_mixed_rates_is_the_file_mode_composition(full):
    lens16 = [out_len(sig.size(1), *rational(rate, 16000)) for sig, rate, _ in RECORDINGS.values()]
    assert [plan_chunks(n // 128 + 1, TC, TO)[0] for n in lens16] == [7, 6, 6, 1]
    want = {n: _composition(full, n) for n in RECORDINGS}
    norms = {n: w[1] for n, w in want.items()}
    # blocks of 2048 (at 16 kHz; 6144 at 48 kHz) with a step after every round; blocks of 777 stepping when a full call is
    # ready; 200 rounds of single samples, then blocks of 4097, stepping when a full call is ready
    runs = [(2048, lambda p: True), (777, lambda p: p.ready >= W), ("ones", lambda p: p.ready >= W)]
    for block, when in runs:
        got, pool = _run_pool(full, norms, block, when)
        for n, (sig, rate, mode) in RECORDINGS.items():
            assert got[n].shape == want[n][0].shape == (sig.size(0), sig.size(1) if mode == "input" else out_len(sig.size(1), *rational(rate, 16000)))
            assert np.array_equal(got[n], want[n][0]), (n, block, int((got[n] != want[n][0]).sum()))
        assert pool.stats["rows"] == 14 + 6 + 6 + 1 and pool.stats["resample_launches"] > 0
        if block == 2048:                                           # ... and the bytes of the arrangement it replaces
            parent = _run_parent(full, norms, block)
            for n in RECORDINGS:
                assert np.array_equal(got[n], parent[n]), n
    assert all(np.isfinite(w[0]).all() and float(np.abs(w[0]).max()) > 0 for w in want.values())


def test_pool_at_mixed_rates_in_a_16_bit_precision(full):
    full.dnn.set_precision("bf16")
    try:
        want = {n: _composition(full, n, tag="bf16") for n in RECORDINGS}
        got, _ = _run_pool(full, {n: w[1] for n, w in want.items()}, 2048, lambda p: True)
    finally:
        full.dnn.set_precision("fp32")
    for n in RECORDINGS:
        assert np.array_equal(got[n], want[n][0]), n
        assert not np.array_equal(want[n][0], _composition(full, n)[0])


def test_open_refuses_a_ratio_by_name(full):
    pool = LivePool(full, width=2, seed=SEED, chunk_frames=TC, overlap_frames=TO, N=1)
    with pytest.raises(ValueError, match="16001"):
        pool.open(1, 1.0, input_rate=16001)
    with pytest.raises(ValueError, match="output_rate"):
        pool.open(1, 1.0, input_rate=48000, output_rate="48000")
    assert not pool.sessions
    s = pool.open(1, 1.0, input_rate=16000, output_rate="input")    # at 16 kHz "input" is 16 kHz: no resampler
    assert s._rs_in is None and s._rs_out is None and s.latency_samples == 128 * TC + 382


def test_norm_first_at_48_khz(full):
    n, rate = 60000, 48000
    sig = _signal(13, n, 2)
    sig[1] *= 1.5                                                   # the peak lies in the second channel ...
    sig[0, 45000] = 3.0                                             # ... and a later, larger sample is never seen
    n0 = 128 * (TC - 1) + 255
    peak = resample(sig.cuda(), rate, 16000)[:, :n0].abs().max().item()
    assert peak < 1.0
    outs = []
    for block, norm in ((6144, "first"), (1001, "first"), (n, "first"), (6144, peak)):
        pool = LivePool(full, width=2, seed=SEED, chunk_frames=TC, overlap_frames=TO, N=2)
        s = pool.open([1, 2], norm, input_rate=rate, output_rate="input")
        parts = []
        for i in range(0, n, block):
            s.push(sig[:, i:i + block].numpy())
            parts += [x for _, x in pool.step()]
        s.finish()
        parts += [x for _, x in pool.step()]
        assert s.norm == peak and s.closed and s.state_bytes() == 0 and s.samples_out == s.samples_in == n
        outs.append(np.concatenate(parts, axis=1))
    assert outs[0].shape == (2, n) and all(np.array_equal(o, outs[0]) for o in outs[1:])


def test_state_is_bounded_and_counts(full):
    """One mono session at 48 kHz in and out, blocks of 6144 with a step after each: the state after 20 s is the state after
    10 s, and as many samples come back as went in."""
    rate, block = 48000, 6144
    n = 20 * rate + 3 * block
    sig = _signal(17, n)
    pool = LivePool(full, width=1, seed=SEED, chunk_frames=TC, overlap_frames=TO, N=1)
    s = pool.open(7, 0.5, input_rate=rate, output_rate="input")
    seen, got = {}, 0
    for i in range(0, n, block):
        s.push(sig[0, i:i + block].numpy())
        for _, x in pool.step(as_tensor=True):
            got += x.size(1)
            del x
        for sec in (10, 20):
            if s.samples_in >= sec * rate and sec not in seen:
                seen[sec] = (s.state_bytes(), pool.state_bytes(), torch.cuda.memory_allocated())
        assert got == s.samples_out <= s.samples_in
    print(f"state after 10 s: {seen[10]}, after 20 s: {seen[20]}")
    assert seen[10][0] == seen[20][0] == seen[10][1] > 0 and seen[20][2] <= seen[10][2]
    rs = 4 * (60 + 2 * block) + 4 * (20 + 2 * block)                # P - 1 and two blocks each way, at most
    assert seen[10][0] < 4 * (128 * TC + 382 + 2 * 2048) + 2 * 8 * 256 * TC + rs
    s.finish()
    for _, x in pool.step():
        got += x.shape[1]
    assert got == s.samples_out == s.samples_in == n and s.closed and pool.state_bytes() == 0 and not pool.sessions


def test_eight_sessions_make_two_resampler_launches_per_step(full):
    rate, block = 48000, 6144
    pool = LivePool(full, width=8, seed=SEED, chunk_frames=TC, overlap_frames=TO, N=1)
    sigs = [_signal(30 + i, 9 * block) for i in range(8)]
    sess = [pool.open(100 + i, 0.5, input_rate=rate, output_rate="input") for i in range(8)]
    sampled = total = 0
    for r in range(9):
        for s, sig in zip(sess, sigs):
            s.push(sig[0, r * block:(r + 1) * block].numpy())
        out = pool.step()
        assert len(out) in (0, 8)
        assert pool.last_step["resample_launches"] == (2 if out else 1), (r, pool.last_step)
        sampled += bool(out)
        total += pool.last_step["resample_launches"]
    for s in sess:
        s.finish()
    out = pool.step()
    assert len(out) == 8 and pool.last_step["resample_launches"] == 2 and sampled == 2
    assert pool.stats["resample_launches"] == total + 2 == 9 + 2 + 2 and pool.stats["calls"] == 3 and not pool.sessions
    assert all(s.samples_out == 9 * block for s in sess)


# ---------------------------------------------------------------------------------------------------- 4
def test_live_resample_cli_in_a_child_process():
    """3 s of stereo s16le at 48 kHz through ``enhance --live --live_channels 2 --live_rate 48000 --live_resample --output_rate
    input``: as many bytes come back, the interleaved ``pcm_encode`` of an in-process pool's output for the decoded input."""
    from flowmse_amd.evaluate import _load_model
    Ls = 144000
    t = np.arange(Ls) / 48000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * 220 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)), 0.2 * np.sin(2 * np.pi * 330 * t)])
    x = (x + 0.05 * synth.normal(23, 9, (2, Ls), 1.0)).astype(np.float32)
    raw = pcm_encode(pcm_interleave(x), "s16le")
    assert len(raw) == 4 * Ls
    args = ["--live", "--live_channels", "2", "--live_rate", "48000", "--live_resample", "--output_rate", "input", "--synthetic", "1",
            "--seed", "3", "--live_block", "3000", "--chunk_frames", "64", "--overlap_frames", "16", "--live_norm", "0.5", "--N", "2"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "flowmse_amd.enhance"] + args, cwd=ROOT, input=raw,
                       capture_output=True)
    assert r.returncode == 0, f"exited with {r.returncode}:\n{r.stderr.decode(errors='replace')[-3000:]}"
    assert len(r.stdout) == 4 * Ls and b"live: enhanced 144000 frames of 2 channels" in r.stderr
    assert b"48000 Hz in, 48000 Hz out" in r.stderr
    model, _ = _load_model(types.SimpleNamespace(synthetic=1, ckpt=None, test_dir="stdin", precision="fp32"), None)
    pool = LivePool(model, width=2, seed=3, chunk_frames=64, overlap_frames=16, N=2)
    s = pool.open([channel_key("live", 0), channel_key("live", 1)], 0.5, input_rate=48000, output_rate="input")
    s.push(pcm_deinterleave(pcm_decode(raw, "s16le"), 2))
    s.finish()
    (_, y), = pool.step()
    assert y.shape == (2, Ls) and r.stdout == pcm_encode(pcm_interleave(y), "s16le")
    assert np.abs(np.frombuffer(r.stdout, dtype="<i2")).max() > 0
