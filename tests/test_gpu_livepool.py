"""GPU: the live pool (flowmse_amd.livepool) -- the two row-table window entries against the single-window entries bit for
bit, their errors, and ``LivePool`` against ``enhance_pooled(batch=W)`` on every session's finished recording alone, bit for
bit, under several push and step patterns; ``W = 1`` against ``LiveEnhancer``; bf16; ``norm="first"``, bounded state; the
``--live --live_channels 2`` CLI in one child process under its own time limit.  The full network at Tc = 64 (and 128),
N = 2, as tests/test_gpu_live.py.  No test asserts a time."""
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
from flowmse_amd.live import LiveEnhancer, live_plan, pcm_decode, pcm_deinterleave, pcm_encode, pcm_interleave
from flowmse_amd.livepool import LivePool
from flowmse_amd.pooled import channel_key, enhance_pooled
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
SEED = 0x1F2E3D4C5B6A7988
FACTOR, EXPONENT = 0.15, 0.5
KW = dict(N=2, T_rev=0.9, t_eps=0.04, odesolver="euler")


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


def _ready_at(k, Tc, hop):
    return 128 * (k * hop + Tc - 1) + 255


def _E(k, hop):
    return 128 * (k + 1) * hop - 255 if k >= 0 else 0


# ---------------------------------------------------------------------------------------------------- 1
def _stft_rows(rows, Tw, out):
    """rows: (buf, s0, frame0, L_total, scale)."""
    table = (_lib.flowse_window_row * max(len(rows), 1))()
    for d, (buf, s0, frame0, Ltot, scale) in zip(table, rows):
        d.buf, d.s0, d.n, d.frame0, d.L_total, d.scale_in = buf.data_ptr(), s0, buf.numel(), frame0, Ltot, scale
    return L.flowse_stft_compress_window_rows(table, len(rows), Tw, _lib.ptr(out), FACTOR, EXPONENT, _lib.current_stream())


def _stft_single(row, Tw):
    buf, s0, frame0, Ltot, scale = row
    out = torch.full((1, 1, 256, Tw), 7.0, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_stft_compress_window(_lib.ptr(buf), s0, buf.numel(), scale, frame0, Tw, Ltot, _lib.ptr(out), FACTOR,
                                             EXPONENT, _lib.current_stream()))
    return out[0]


def test_stft_rows_are_the_single_window_entry():
    Ls, Tc, To = 98765, 64, 16
    sig = _signal(5, Ls).cuda().reshape(-1)
    other = _signal(6, 30000).cuda().reshape(-1)
    K, hop, _ = plan_chunks(Ls // 128 + 1, Tc, To)
    assert K == 16
    lo5 = 128 * 5 * hop - 255
    shared = sig[1000:60000].clone()                                # two rows name this buffer
    lo14, lo15 = 128 * 14 * hop - 255, 128 * 15 * hop - 256         # the last chunk's one frame reflects back to L - 256
    rows = [(sig[:_ready_at(0, Tc, hop)].clone(), 0, 0, -1, 0.37),                         # reflects about sample 0
            (shared, 1000, 5 * hop, -1, 0.37),                                             # open, s0 > 0
            (shared, 1000, 5 * hop + 16, -1, 0.37),                                        # the same buffer, another frame0
            (sig[lo14:].clone(), lo14, 14 * hop, Ls, 0.37),                                # closed, the last but one
            (sig[min(lo15, Ls - 256):].clone(), min(lo15, Ls - 256), 15 * hop, Ls, 0.37),  # closed: right reflection, zero frames
            (other[128 * hop - 255:].clone(), 128 * hop - 255, hop, 30000, 1.9)]           # a second signal, another scale
    want = [_stft_single(r, Tc) for r in rows]
    assert lo5 >= 1000 and bool((want[4][..., Ls // 128 + 1 - 15 * hop:] == 0).all()) and not torch.equal(want[1], want[2])
    out = torch.full((6, 1, 256, Tc), 7.0, dtype=torch.complex64, device="cuda")
    _lib.check(_stft_rows(rows, Tc, out))
    torch.cuda.synchronize()
    for r in range(6):
        assert torch.equal(out[r], want[r]), r
    # R = 16
    rows16 = [rows[i % 6] for i in range(16)]
    out16 = torch.full((16, 1, 256, Tc), 7.0, dtype=torch.complex64, device="cuda")
    _lib.check(_stft_rows(rows16, Tc, out16))
    torch.cuda.synchronize()
    for r in range(16):
        assert torch.equal(out16[r], want[r % 6]), r
    # one row a sample short at either end: the whole call is refused, by row
    out.fill_(7.0)
    buf, s0, frame0, Ltot, scale = rows[1]
    lo, hi = lo5, _ready_at(5, Tc, hop)
    for r, short in ((3, (sig[lo:hi - 1].clone(), lo, frame0, Ltot, scale)), (5, (sig[lo + 1:hi].clone(), lo + 1, frame0, Ltot, scale))):
        bad = list(rows)
        bad[r] = short
        assert _stft_rows(bad, Tc, out) == ERR_SHAPE
        msg = L.flowse_last_error()
        assert b"stft window rows" in msg and f"row {r}".encode() in msg and str(short[1]).encode() in msg
    for R in (0, 17):
        table = (_lib.flowse_window_row * 17)()
        assert L.flowse_stft_compress_window_rows(table, R, Tc, _lib.ptr(out), FACTOR, EXPONENT, _lib.current_stream()) == ERR_SHAPE
    assert L.flowse_stft_compress_window_rows(None, 6, Tc, _lib.ptr(out), FACTOR, EXPONENT, _lib.current_stream()) == ERR_ARG
    assert b"flowse_stft_compress_window_rows" in L.flowse_last_error()
    table = (_lib.flowse_window_row * 6)()
    for d, (buf, s0, frame0, Ltot, scale) in zip(table, rows):
        d.buf, d.s0, d.n, d.frame0, d.L_total, d.scale_in = buf.data_ptr(), s0, buf.numel(), frame0, Ltot, scale
    table[2].buf = None
    assert L.flowse_stft_compress_window_rows(table, 6, Tc, _lib.ptr(out), FACTOR, EXPONENT, _lib.current_stream()) == ERR_ARG
    assert b"row 2" in L.flowse_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 2
def _istft_rows(rows, Tc, hop):
    """rows: (prev2, prev, cur, k, last, Ltot, out, e0, n_out, scale)."""
    table = (_lib.flowse_window_out * len(rows))()
    for d, (p2, p1, cur, k, last, Ltot, out, e0, n, scale) in zip(table, rows):
        d.prev2_c64, d.prev_c64 = (None if p2 is None else p2.data_ptr()), (None if p1 is None else p1.data_ptr())
        d.cur_c64, d.out = cur.data_ptr(), out.data_ptr()
        d.k, d.L, d.e0, d.n_out, d.last, d.scale_out = k, Ltot, e0, n, int(last), scale
    return L.flowse_istft_decompress_window_rows(table, len(rows), Tc, hop, FACTOR, EXPONENT, _lib.current_stream())


@pytest.mark.parametrize("Tc,To", [(64, 16), (128, 64)], ids=lambda v: str(v))
def test_istft_rows_are_the_single_window_entry(Tc, To):
    K, hop = 4, Tc - To
    Tg = (K - 1) * hop + Tc
    Ls = 128 * (Tg - 6) + 77
    needs_two = Tc - 2 * To < 3
    a = [c.clone() for c in C.c64(synth.synth_spectrogram(40 + Tc + To, K, 256, Tc)).cuda()]
    b = [c.clone() for c in C.c64(synth.synth_spectrogram(41 + Tc + To, K, 256, Tc)).cuda()]
    # (chunks, k, last, scale): k = 0, 1 and 3 open, and a last chunk -- ranges of three different lengths
    spec = [(a, 0, False, 0.7), (a, 1, False, 0.7), (b, 3, False, 1.3), (b, 3, True, 0.7), (b, 1, False, 0.7)]
    rows, want = [], []
    for ch, k, last, scale in spec:
        e0, e1 = _E(k - 1, hop), (Ls if last else _E(k, hop))
        p1 = ch[k - 1] if k >= 1 else None
        p2 = ch[k - 2] if k >= 2 and needs_two else None
        out = torch.full((e1 - e0 + 1000,), 7.0, device="cuda")
        rows.append((p2, p1, ch[k], k, last, Ls if last else 0, out, e0, e1 - e0, scale))
        w = torch.full((e1 - e0,), 7.0, device="cuda")
        _lib.check(L.flowse_istft_decompress_window(_lib.ptr(p2), _lib.ptr(p1), _lib.ptr(ch[k]), k, Tc, hop, int(last),
                                                    Ls if last else 0, FACTOR, EXPONENT, _lib.ptr(w), e0, e1 - e0, scale,
                                                    _lib.current_stream()))
        want.append(w)
    assert len({r[8] for r in rows}) == 3
    _lib.check(_istft_rows(rows, Tc, hop))
    torch.cuda.synchronize()
    for r, (row, w) in enumerate(zip(rows, want)):
        n = row[8]
        assert torch.equal(row[6][:n], w) and bool((row[6][n:] == 7.0).all()), r
        assert float(w.abs().max()) > 0 and not bool((w == 7.0).any())
    if needs_two:                                                   # a row that needs chunk k - 2 without it: nothing is written
        for row in rows:
            row[6].fill_(7.0)
        bad = list(rows)
        bad[2] = (None,) + rows[2][1:]
        assert _istft_rows(bad, Tc, hop) == ERR_SHAPE
        msg = L.flowse_last_error()
        assert b"istft window rows" in msg and b"row 2" in msg
        torch.cuda.synchronize()
        assert all(bool((row[6] == 7.0).all()) for row in rows)
    for R in (0, 17):
        table = (_lib.flowse_window_out * 17)()
        assert L.flowse_istft_decompress_window_rows(table, R, Tc, hop, FACTOR, EXPONENT, _lib.current_stream()) == ERR_SHAPE
    assert L.flowse_istft_decompress_window_rows(None, 1, Tc, hop, FACTOR, EXPONENT, _lib.current_stream()) == ERR_ARG


# ---------------------------------------------------------------------------------------------------- 3, 4, 6
_ORACLE = {}


def _oracle(model, name, sig, W, Tc, To, seed=SEED, tag="fp32"):
    """``enhance_pooled(batch=W)`` on the recording alone, computed once per (recording, geometry, precision)."""
    key = (name, W, Tc, To, seed, tag)
    if key not in _ORACLE:
        got = {}
        enhance_pooled(model, lambda i: sig.cuda(), [(name, sig.size(0), sig.size(1))], lambda i, x: got.update(x=x.cpu().numpy()),
                       batch=W, chunk_frames=Tc, overlap_frames=To, noise_seed=seed, **KW)
        _ORACLE[key] = got["x"]
    return _ORACLE[key]


def _run_pool(model, recordings, W, Tc, To, block, step_when, seed=SEED):
    """Push the recordings round-robin in blocks of ``block``; ``step_when(pool)`` says after a round whether to step.
    Returns ({name: [C, L]}, pool, the largest filler count of any bucket in any step)."""
    pool = LivePool(model, width=W, seed=seed, chunk_frames=Tc, overlap_frames=To, **KW)
    sess, parts, done, worst = {}, {}, {}, 0
    for name, sig in recordings.items():
        s = pool.open([channel_key(name, c) for c in range(sig.size(0))], sig.abs().max().item())
        sess[name], parts[s], done[name] = s, [], 0

    def step():
        nonlocal worst
        for s, x in pool.step():
            assert x.dtype == np.float32 and x.shape[0] == s.channels
            parts[s].append(x)
        worst = max([worst] + list(pool.last_step["fillers"].values()))

    how = rounds = 0
    while any(done[n] < sig.size(1) or not sess[n].finished for n, sig in recordings.items()):
        for name, sig in recordings.items():
            s = sess[name]
            if s.finished:
                continue
            if done[name] == sig.size(1):
                s.finish()
                continue
            piece = sig[:, done[name]:done[name] + ((1 if rounds < 300 else 4097) if block == "ones" else block)]
            if sig.size(0) == 1 and how % 3 == 0:
                piece = piece[0]
            assert s.push(piece.numpy() if how % 3 < 2 else piece.cuda()) is None
            done[name] += piece.shape[-1]
            how += 1
        rounds += 1
        if step_when(pool):
            step()
    while pool.ready:
        step()
    assert not pool.sessions and pool.state_bytes() == 0
    return {n: np.concatenate(parts[s], axis=1) for n, s in sess.items()}, pool, worst


def _recordings_3():
    return {"a.wav": _signal(1, 20000), "b.wav": _signal(2, 30000, 2), "c.wav": _signal(3, 5000), "d.wav": _signal(4, 8200)}


def test_pool_is_enhance_pooled_on_every_session_alone(full):
    W, Tc, To = 4, 64, 16
    rec = _recordings_3()
    assert [plan_chunks(s.size(1) // 128 + 1, Tc, To)[0] for s in rec.values()] == [3, 5, 1, 2]
    want = {n: _oracle(full, n, s, W, Tc, To) for n, s in rec.items()}
    # blocks of 2048 with a step after every round; blocks of 777, then 300 rounds of single samples followed by blocks of
    # 4097, stepping only when a full call is ready (and at the end)
    runs = [(2048, lambda p: True), (777, lambda p: p.ready >= W), ("ones", lambda p: p.ready >= W)]
    for block, when in runs:
        got, pool, worst = _run_pool(full, rec, W, Tc, To, block, when)
        for n in rec:
            assert got[n].shape == want[n].shape and np.array_equal(got[n], want[n]), (n, block)
        assert worst <= W - 1 and pool.stats["rows"] == 3 + 10 + 1 + 2
    # B alone
    got, _, _ = _run_pool(full, {"b.wav": rec["b.wav"]}, W, Tc, To, 2048, lambda p: True)
    assert np.array_equal(got["b.wav"], want["b.wav"])
    # another seed is another output
    got, _, _ = _run_pool(full, {"b.wav": rec["b.wav"]}, W, Tc, To, 2048, lambda p: p.ready >= W, seed=SEED + 1)
    assert got["b.wav"].shape == want["b.wav"].shape and not np.array_equal(got["b.wav"], want["b.wav"])
    assert all(np.isfinite(w).all() and float(np.abs(w).max()) > 0 for w in want.values())


def test_pool_keeps_two_chunks_and_a_second_bucket(full):
    W, Tc, To = 4, 128, 64
    rec = {"e.wav": _signal(5, 5000), "f.wav": _signal(6, 8200), "g.wav": _signal(7, 40000)}
    assert [plan_chunks(s.size(1) // 128 + 1, Tc, To)[0] for s in rec.values()] == [1, 1, 4]
    want = {n: _oracle(full, n, s, W, Tc, To) for n, s in rec.items()}
    for block, when in ((2048, lambda p: True), (777, lambda p: p.ready >= 2)):
        got, pool, worst = _run_pool(full, rec, W, Tc, To, block, when)
        for n in rec:
            assert np.array_equal(got[n], want[n]), (n, block)
        assert worst <= W - 1


def test_pool_of_width_one_is_the_live_enhancer(full):
    Ls, Tc, To = 40000, 64, 16
    sig = _signal(19, Ls)
    key, norm = channel_key("h.wav", 0), sig.abs().max().item()
    live = LiveEnhancer(full, norm=norm, key=key, seed=SEED, chunk_frames=Tc, overlap_frames=To, **KW)
    want = np.concatenate([live.push(sig[0, i:i + 2048].numpy()) for i in range(0, Ls, 2048)] + [live.finish()])
    got, pool, worst = _run_pool(full, {"h.wav": sig}, 1, Tc, To, 2048, lambda p: True)
    assert got["h.wav"].shape == (1, Ls) and np.array_equal(got["h.wav"][0], want) and worst == 0


def test_pool_in_a_16_bit_precision(full):
    W, Tc, To = 4, 64, 16
    rec = {n: s for n, s in _recordings_3().items() if n in ("a.wav", "b.wav")}
    full.dnn.set_precision("bf16")
    try:
        want = {n: _oracle(full, n, s, W, Tc, To, tag="bf16") for n, s in rec.items()}
        got, _, _ = _run_pool(full, rec, W, Tc, To, 2048, lambda p: True)
    finally:
        full.dnn.set_precision("fp32")
    for n in rec:
        assert np.array_equal(got[n], want[n]), n
        assert not np.array_equal(want[n], _oracle(full, n, rec[n], W, Tc, To))


# ---------------------------------------------------------------------------------------------------- 7
def test_norm_first_and_state(full):
    Ls, Tc, To = 20000, 64, 16
    hop = Tc - To
    sig = _signal(13, Ls, 2)
    sig[1] *= 1.5                                                   # the peak lies in the second channel ...
    sig[0, 15000] = 3.0                                             # ... and a later, larger sample is never seen
    n0 = _ready_at(0, Tc, hop)
    peak = sig[:, :n0].abs().max().item()
    assert peak == sig[1, :n0].abs().max().item() > sig[0, :n0].abs().max().item()
    kw = dict(width=2, seed=SEED, chunk_frames=Tc, overlap_frames=To, N=2)
    outs = []
    for block, norm in ((2048, "first"), (777, "first"), (Ls, "first"), (2048, peak)):
        pool = LivePool(full, **kw)
        s = pool.open([1, 2], norm)
        parts = []
        for i in range(0, Ls, block):
            s.push(sig[:, i:i + block].numpy())
            parts += [x for _, x in pool.step()]
        s.finish()
        parts += [x for _, x in pool.step()]
        assert s.norm == peak and s.closed and s.state_bytes() == 0
        outs.append(np.concatenate(parts, axis=1))
    assert outs[0].shape == (2, Ls) and all(np.array_equal(o, outs[0]) for o in outs[1:])
    # an all-zero stream that ends before chunk 0: norm 1.0
    pool = LivePool(full, **kw)
    s = pool.open([1, 2], "first")
    s.push(np.zeros((2, 3000), dtype=np.float32))
    s.finish()
    (_, x), = pool.step()
    assert s.norm == 1.0 and x.shape == (2, 3000) and np.isfinite(x).all()
    # state: equal after chunk 3 and after chunk 39, and returned when the session closes
    n = _ready_at(39, Tc, hop) + 100
    sig = _signal(17, n)
    pool = LivePool(full, width=1, seed=SEED, chunk_frames=Tc, overlap_frames=To, N=1)
    s = pool.open(7, 0.5)
    seen = {}
    for i in range(0, n, 2048):
        s.push(sig[0, i:i + 2048].numpy())
        out = pool.step()
        ready = live_plan(s.samples_in, Tc, To)[0]
        assert s.samples_out == live_plan(s.samples_in, Tc, To)[1]
        if ready in (4, 40) and ready not in seen:
            del out
            seen[ready] = (s.state_bytes(), pool.state_bytes(), torch.cuda.memory_allocated())
    assert set(seen) == {4, 40} and seen[4][0] == seen[40][0] == seen[4][1] > 0 and seen[40][2] <= seen[4][2]
    assert seen[4][0] < 4 * (128 * Tc + 382 + 2 * 2048) + 2 * 8 * 256 * Tc
    s.finish()
    (_, tail), = pool.step()
    assert s.samples_out == n and s.closed and s.state_bytes() == 0 and pool.state_bytes() == 0 and not pool.sessions
    assert np.isfinite(tail).all()
    del tail
    assert torch.cuda.memory_allocated() < seen[40][2]


# ---------------------------------------------------------------------------------------------------- 8
def test_live_channels_cli_in_a_child_process():
    """3 s of stereo s16le through ``enhance --live --live_channels 2``: the interleaved ``pcm_encode`` of an in-process
    pool's output for the decoded input.  ``--synthetic 1`` names the weights, as in the other CLI tests."""
    from flowmse_amd.evaluate import _load_model
    Ls = 48000
    t = np.arange(Ls) / 16000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * 220 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)), 0.2 * np.sin(2 * np.pi * 330 * t)])
    x = (x + 0.05 * synth.normal(23, 9, (2, Ls), 1.0)).astype(np.float32)
    raw = pcm_encode(pcm_interleave(x), "s16le")
    assert len(raw) == 4 * Ls
    args = ["--live", "--live_channels", "2", "--synthetic", "1", "--seed", "3", "--live_block", "1000", "--chunk_frames", "64",
            "--overlap_frames", "16", "--live_norm", "0.5", "--N", "2"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "flowmse_amd.enhance"] + args, cwd=ROOT, input=raw,
                       capture_output=True)
    assert r.returncode == 0, f"exited with {r.returncode}:\n{r.stderr.decode(errors='replace')[-3000:]}"
    assert len(r.stdout) == 4 * Ls and b"live: enhanced 48000 frames of 2 channels" in r.stderr
    model, _ = _load_model(types.SimpleNamespace(synthetic=1, ckpt=None, test_dir="stdin", precision="fp32"), None)
    pool = LivePool(model, width=2, seed=3, chunk_frames=64, overlap_frames=16, N=2)
    s = pool.open([channel_key("live", 0), channel_key("live", 1)], 0.5)
    s.push(pcm_deinterleave(pcm_decode(raw, "s16le"), 2))
    s.finish()
    (_, y), = pool.step()
    assert y.shape == (2, Ls) and r.stdout == pcm_encode(pcm_interleave(y), "s16le")
    assert np.abs(np.frombuffer(r.stdout, dtype="<i2")).max() > 0
