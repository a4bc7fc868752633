"""GPU: live enhancement (flowmse_amd.live) -- the window STFT against rows of the chunk call, the window iSTFT against
slices of the chunk call, the shape errors of both, and ``LiveEnhancer`` against ``enhance_long(batch=1)`` bit for bit under
every push pattern; ``norm="first"``, bounded state, the counters, the life cycle and the ``--live`` CLI in one child
process under its own time limit.  No test asserts a time."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _cases as C
from flowmse_amd import _lib
from flowmse_amd.chunked import enhance_long, plan_chunks
from flowmse_amd.live import LiveEnhancer, live_plan, pcm_decode, pcm_encode
from flowmse_amd.util import synth
from flowmse_amd.util.noise import utterance_key

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
KEY, SEED = 0x912975D344AF26C6, 0x1F2E3D4C5B6A7988
FACTOR, EXPONENT = 0.15, 0.5


def _model(cfg):
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **cfg)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def full():
    assert torch.cuda.is_available()
    return _model(C.FULL)


def _signal(seed, n, std=0.1):
    return torch.from_numpy(synth.normal(seed, 9, (1, n), std))


def _ready_at(k, Tc, hop):
    return 128 * (k * hop + Tc - 1) + 255


def _E(k, hop):
    """Output samples final once chunk k is sampled (E_{-1} = 0)."""
    return 128 * (k + 1) * hop - 255 if k >= 0 else 0


def _stft_window(buf, s0, frame0, Tc, L_total, out, scale=1.0):
    return L.flowse_stft_compress_window(_lib.ptr(buf), s0, buf.numel(), scale, frame0, Tc, L_total, _lib.ptr(out), FACTOR,
                                         EXPONENT, _lib.current_stream())


def _istft_window(prev2, prev, cur, k, Tc, hop, last, Ltot, out, e0, n_out, scale=0.7):
    return L.flowse_istft_decompress_window(_lib.ptr(prev2), _lib.ptr(prev), _lib.ptr(cur), k, Tc, hop, int(last), Ltot, FACTOR,
                                            EXPONENT, _lib.ptr(out), e0, n_out, scale, _lib.current_stream())


def _samples_read(frame0, Tc, Ls, closed):
    """[lo, hi): the sample indices the frames [frame0, frame0 + Tc) read, from the STFT's definition (centre padding of
    255, reflection at both ends, frames >= Ls // 128 + 1 of a closed recording zero) -- not from the library's closed form."""
    t = np.arange(frame0, min(frame0 + Tc, Ls // 128 + 1) if closed else frame0 + Tc)
    j = np.abs(128 * t[:, None] + np.arange(510)[None, :] - 255)
    if closed:
        j = np.where(j >= Ls, 2 * (Ls - 1) - j, j)
    return int(j.min()), int(j.max()) + 1


# ---------------------------------------------------------------------------------------------------- 1
def test_window_stft_is_rows_of_the_chunk_call():
    """L = 98765 at (64, 16): 772 frames, 16 chunks.  Every chunk from the smallest window that holds what its frames read
    (s0 > 0 from chunk 1 on), open where the recording has that many samples, closed for the last two (right reflection and
    zero frames); chunk 0 reflects about sample 0.  A window one sample short at either end is refused."""
    Ls, Tc, To = 98765, 64, 16
    sig = _signal(5, Ls).cuda().reshape(-1)
    K, hop, _ = plan_chunks(Ls // 128 + 1, Tc, To)
    assert K == 16
    whole = torch.empty(K, 1, 256, Tc, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_stft_compress_chunks(_lib.ptr(sig), Ls, 0.37, _lib.ptr(whole), K, Tc, hop, FACTOR, EXPONENT,
                                             _lib.current_stream()))
    done = []
    for k in range(K):
        for closed in (False, True):
            if (not closed and _ready_at(k, Tc, hop) > Ls) or (closed and k < K - 2):
                continue
            lo, hi = _samples_read(k * hop, Tc, Ls, closed)
            assert (lo == 0) == (k == 0) and (closed or hi == _ready_at(k, Tc, hop))
            row = torch.full((1, 1, 256, Tc), 7.0, dtype=torch.complex64, device="cuda")
            _lib.check(_stft_window(sig[lo:hi].clone(), lo, k * hop, Tc, Ls if closed else -1, row, 0.37))
            torch.cuda.synchronize()
            assert torch.equal(row[0], whole[k]), (k, closed)
            done.append((k, closed))
            # one sample short, at the end and (past chunk 0) at the start
            assert _stft_window(sig[lo:hi - 1].clone(), lo, k * hop, Tc, Ls if closed else -1, row, 0.37) == ERR_SHAPE
            if k:
                assert _stft_window(sig[lo + 1:hi].clone(), lo + 1, k * hop, Tc, Ls if closed else -1, row, 0.37) == ERR_SHAPE
            torch.cuda.synchronize()
            assert torch.equal(row[0], whole[k])
    assert (K - 1, True) in done and (K - 2, True) in done and (0, False) in done and (K - 1, False) not in done
    assert bool((whole[-1][..., Ls // 128 + 1 - (K - 1) * hop:] == 0).all())      # the zero frames were compared too
    # a window that holds more than the frames read gives the same row; frame0 need not be a chunk start
    row = torch.empty(1, 1, 256, Tc, dtype=torch.complex64, device="cuda")
    _lib.check(_stft_window(sig[1000:60000].clone(), 1000, 5 * hop, Tc, -1, row, 0.37))
    assert torch.equal(row[0], whole[5])
    _lib.check(_stft_window(sig[1000:60000].clone(), 1000, 5 * hop + 16, Tc, -1, row, 0.37))
    assert torch.equal(row[0, :, :, :32], whole[5][:, :, 16:48]) and torch.equal(row[0, :, :, 32:], whole[6][:, :, :32])


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("Tc,To", [(64, 16), (128, 64), (64, 0)], ids=lambda v: str(v))
def test_window_istft_is_slices_of_the_chunk_call(Tc, To):
    """Independent random chunks, K = 4.  The ranges [E_{k-1}, E_k) per chunk and the tail with the last flag concatenate to
    the chunk call's output; so do the same ranges cut at an odd sample.  At To = Tc / 2 the range of chunk k lies under
    blended frames of chunk k - 1, whose other half is chunk k - 2: without that chunk the call refuses."""
    K, hop = 4, Tc - To
    Tg = (K - 1) * hop + Tc
    Ls = 128 * (Tg - 6) + 77
    assert plan_chunks(Ls // 128 + 1, Tc, To)[0] == K
    chunks = C.c64(synth.synth_spectrogram(40 + Tc + To, K, 256, Tc)).cuda()
    want = torch.empty(1, Ls, device="cuda")
    _lib.check(L.flowse_istft_decompress_chunks(_lib.ptr(chunks), K, Tc, hop, FACTOR, EXPONENT, _lib.ptr(want), Ls, 0.7,
                                                _lib.current_stream()))
    rows = [chunks[k].clone() for k in range(K)]                   # separate allocations, as a live session holds them
    needs_two = Tc - 2 * To < 3
    for cut in (None, 1001):
        parts = []
        for k in range(K):
            last = k == K - 1
            e0, e1 = _E(k - 1, hop), (Ls if last else _E(k, hop))
            prev = rows[k - 1] if k >= 1 else None
            prev2 = rows[k - 2] if k >= 2 and needs_two else None
            for a, b in ([(e0, e1)] if cut is None else [(e0, e0 + cut), (e0 + cut, e1)]):
                out = torch.full((b - a,), 7.0, device="cuda")
                _lib.check(_istft_window(prev2, prev, rows[k], k, Tc, hop, last, Ls if last else 0, out, a, b - a))
                parts.append(out)
            if k >= 2 and needs_two:
                out = torch.full((e1 - e0,), 7.0, device="cuda")
                assert _istft_window(None, prev, rows[k], k, Tc, hop, last, Ls if last else 0, out, e0, e1 - e0) == ERR_SHAPE
                assert b"istft window" in L.flowse_last_error()
                torch.cuda.synchronize()
                assert bool((out == 7.0).all())
        got = torch.cat(parts)
        torch.cuda.synchronize()
        assert got.shape == (Ls,) and torch.equal(got, want[0]), (Tc, To, cut)
    assert float(want.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 3
def test_window_shape_errors_return_a_status_and_launch_nothing():
    Ls, Tc, hop = 40000, 64, 48
    sig = _signal(2, Ls).cuda().reshape(-1)
    row = torch.full((1, 1, 256, Tc), 7.0, dtype=torch.complex64, device="cuda")
    lo, hi = _samples_read(2 * hop, Tc, Ls, False)
    bad = [(sig[lo:hi - 1], lo, 2 * hop, Tc, -1),                  # the last frame's last sample has not arrived
           (sig[lo + 1:hi], lo + 1, 2 * hop, Tc, -1),              # the first frame's first sample was dropped
           (sig[1:hi], 1, 0, Tc, -1),                              # left reflection with s0 > 0
           (sig[1:hi], 1, 1, Tc, -1),                              # frame 1 reflects too (128 - 255 < 0)
           (sig[lo:hi], lo, 2 * hop, Tc, 200),                     # L_total <= 255
           (sig[lo:hi], lo, 2 * hop, Tc, hi - 1),                  # the window reaches past the end of the recording
           (sig[lo:hi], lo, 2 * hop, 0, -1), (sig[lo:hi], lo, -2, Tc, -1), (sig[lo:hi], -1, 2 * hop, Tc, -1),
           (sig[lo:hi], lo, 2 * hop, Tc, -2)]
    for buf, s0, frame0, tc, Ltot in bad:
        assert _stft_window(buf.clone(), s0, frame0, tc, Ltot, row) == ERR_SHAPE, (s0, frame0, tc, Ltot)
        assert b"stft window" in L.flowse_last_error()
    assert _stft_window(sig[1:hi].clone(), 1, 0, Tc, -1, row) == ERR_SHAPE
    msg = L.flowse_last_error()
    assert b"s0=1" in msg and b"sample 0" in msg                   # the values are in the message
    assert _stft_window(sig[lo:hi - 1].clone(), lo, 2 * hop, Tc, -1, row) == ERR_SHAPE
    assert str(hi - 1).encode() in L.flowse_last_error() and str(lo).encode() in L.flowse_last_error()
    s = _lib.current_stream()
    assert L.flowse_stft_compress_window(None, lo, hi - lo, 1.0, 2 * hop, Tc, -1, _lib.ptr(row), FACTOR, EXPONENT, s) == ERR_ARG
    assert L.flowse_stft_compress_window(_lib.ptr(sig), lo, hi - lo, 1.0, 2 * hop, Tc, -1, None, FACTOR, EXPONENT, s) == ERR_ARG
    assert b"flowse_stft_compress_window" in L.flowse_last_error()
    torch.cuda.synchronize()
    assert bool((row == 7.0).all())
    _lib.check(_stft_window(sig[lo:hi].clone(), lo, 2 * hop, Tc, -1, row))
    torch.cuda.synchronize()
    assert not bool((row == 7.0).any())

    # the inverse: chunks 1, 2, 3 of a stack at (64, 16); chunk 3 is current
    ch = [C.c64(synth.synth_spectrogram(50 + i, 1, 256, Tc)).cuda()[0] for i in range(3)]
    k, To = 3, Tc - hop
    e0, e1 = _E(k - 1, hop), _E(k, hop)
    out = torch.full((e1 - e0 + 1000,), 7.0, device="cuda")
    first_plain = 128 * ((k - 1) * hop + To) + 127                 # the first sample under no blended frame of chunk k-1
    bad = [(None, ch[1], ch[2], k, Tc, hop, 0, 0, e0, e1 - e0 + 1, 0.15),          # one sample into the frames of chunk k+1
           (None, None, ch[2], k, Tc, hop, 0, 0, e0, e1 - e0, 0.15),               # chunk k-1 is needed and not given
           (None, ch[1], ch[2], k, Tc, hop, 0, 0, first_plain - 1, 500, 0.15),     # a blended frame of chunk k-1: needs k-2
           (ch[0], ch[1], ch[2], k, Tc, hop, 0, 0, 128 * (k - 2) * hop + 127, 500, 0.15),   # a blended frame of chunk k-2: a 4th chunk
           (None, ch[1], ch[2], k, Tc, hop, 1, e1 - 1, e0, e1 - e0, 0.15),         # past L with the last flag
           (None, ch[1], ch[2], k, Tc, hop, 1, 128 * (k * hop + Tc - 1) + 256, e0, 500, 0.15),   # L past the frames
           (None, ch[1], ch[2], k, Tc, 30, 0, 0, e0, 500, 0.15), (None, ch[1], ch[2], k, Tc, 65, 0, 0, e0, 500, 0.15),
           (None, ch[1], ch[2], -1, Tc, hop, 0, 0, e0, 500, 0.15), (None, ch[1], ch[2], k, Tc, hop, 0, 0, e0, 0, 0.15),
           (None, ch[1], ch[2], k, Tc, hop, 0, 0, -1, 500, 0.15), (None, ch[1], ch[2], k, Tc, hop, 0, 0, e0, 500, 0.0)]
    s = _lib.current_stream()
    for p2, p1, cur, kk, tc, hp, last, Ltot, a, n, factor in bad:
        rc = L.flowse_istft_decompress_window(_lib.ptr(p2), _lib.ptr(p1), _lib.ptr(cur), kk, tc, hp, last, Ltot, factor, EXPONENT,
                                              _lib.ptr(out), a, n, 1.0, s)
        assert rc == ERR_SHAPE, (kk, tc, hp, last, Ltot, a, n, factor)
        assert b"istft window" in L.flowse_last_error()
    assert _istft_window(None, ch[1], ch[2], k, Tc, hop, 0, 0, out, e0, e1 - e0 + 1) == ERR_SHAPE
    msg = L.flowse_last_error()
    assert f"[{e0}, {e1 + 1})".encode() in msg and b"k+1" in msg
    assert _istft_window(None, ch[1], None, k, Tc, hop, 0, 0, out, e0, 500) == ERR_ARG
    assert L.flowse_istft_decompress_window(None, _lib.ptr(ch[1]), _lib.ptr(ch[2]), k, Tc, hop, 0, 0, FACTOR, EXPONENT, None, e0,
                                            500, 1.0, s) == ERR_ARG
    assert b"flowse_istft_decompress_window" in L.flowse_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the range that needed chunk k-2 is served once it is given, and equals the chunk call on the three chunks
    stack = torch.stack(ch)[:, None].contiguous()
    Lw = 128 * (2 * hop + Tc - 1)
    want = torch.empty(1, Lw, device="cuda")
    _lib.check(L.flowse_istft_decompress_chunks(_lib.ptr(stack), 3, Tc, hop, FACTOR, EXPONENT, _lib.ptr(want), Lw, 0.7, s))
    off = 128 * (k - 2) * hop                                      # the three chunks as chunks 0..2 of a recording of their own
    _lib.check(_istft_window(ch[0], ch[1], ch[2], k, Tc, hop, 0, 0, out, first_plain - 1, 500))
    torch.cuda.synchronize()
    assert torch.equal(out[:500], want[0, first_plain - 1 - off:first_plain - 1 - off + 500])
    assert bool((out[500:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 4
def _patterns(n):
    """Push sizes that sum to n: all at once; blocks of 2048; 300 single samples, then blocks of 4097; with empty pushes."""
    def blocks(sizes, start=0):
        out, done, i = [], start, 0
        while done < n:
            s = min(sizes[i % len(sizes)], n - done)
            out.append(s)
            done += s
            i += 1
        return out
    return {"whole": [n], "2048": blocks([2048]), "ones": [1] * 300 + blocks([4097], 300),
            "empties": [0] + blocks([0, 777, 0, 0, 3001, 5]) + [0]}


def _as_input(chunk, how):
    if how == 0:
        return chunk.numpy()
    if how == 1:
        return chunk[None]                                          # a CPU tensor [1, n]
    return chunk.cuda()


def _run_live(live, y, sizes, how=0, check=None):
    """Push ``y`` (a CPU tensor [n]) in ``sizes`` and finish; returns the concatenated output."""
    parts, done = [], 0
    for i, s in enumerate(sizes):
        parts.append(live.push(_as_input(y[done:done + s], (how + i) % 3 if how < 0 else how)))
        done += s
        if check:
            check(live)
    parts.append(live.finish())
    assert all(p.dtype == np.float32 and p.ndim == 1 for p in parts)
    return np.concatenate(parts)


CONTRACT = [(20000, 64, 16), (255 * 128, 64, 16), (40000, 64, 16), (98765, 64, 16), (40000, 128, 64),
            (20000, 256, 32),          # K = 1, T = 157 padded to 192 < Tc
            (255 * 128, 256, 32),      # K = 1, T = 256 = Tc exactly
            (5000, 64, 16),            # K = 1 at the small geometry
            (8200, 64, 16),            # K = 2 and chunk 0 never became ready: both sampled by finish()
            (16384, 64, 0)]            # T = 129 = 2 Tc + 1: the last chunk's one frame reflects back to sample L - 256


@pytest.mark.parametrize("Ls,Tc,To", CONTRACT, ids=lambda v: str(v))
def test_live_is_enhance_long_bit_for_bit(full, Ls, Tc, To):
    """The contract: concat(push..., finish) == enhance_long(batch=1, same key and seed, norm = max|y|) for every push
    pattern, with ``samples_out`` following ``live_plan`` after every push."""
    sig = _signal(Ls % 89, Ls)
    kw = dict(N=2, T_rev=0.9, t_eps=0.04, odesolver="euler")
    want = enhance_long(full, sig.cuda(), Tc, To, batch=1, noise_key=KEY, noise_seed=SEED, **kw)
    live = LiveEnhancer(full, norm=sig.abs().max().item(), key=KEY, seed=SEED, chunk_frames=Tc, overlap_frames=To, **kw)
    assert live.latency_samples == 128 * Tc + 382

    def counters(lv):
        assert lv.samples_out == live_plan(lv.samples_in, Tc, To)[1]

    for how, (name, sizes) in enumerate(_patterns(Ls).items()):
        got = _run_live(live, sig[0], sizes, how=-1 - how if name == "empties" else how % 3, check=counters)
        assert live.samples_in == live.samples_out == Ls == got.shape[0]
        assert np.array_equal(got, want), (name, int((got != want).sum()), int(np.flatnonzero(got != want)[0]))
        with pytest.raises(RuntimeError):
            live.push(np.zeros(4, dtype=np.float32))
        live.reset()
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    # another key or seed is another recording
    live.reset(KEY + 1)
    assert not np.array_equal(_run_live(live, sig[0], [Ls]), want)


@pytest.mark.parametrize("precision", ["bf16"])
def test_live_is_enhance_long_in_a_16_bit_precision(full, precision):
    Ls, Tc, To = 40000, 64, 16
    sig = _signal(11, Ls)
    full.dnn.set_precision(precision)
    try:
        want = enhance_long(full, sig.cuda(), Tc, To, batch=1, N=2, noise_key=KEY, noise_seed=SEED)
        live = LiveEnhancer(full, norm=sig.abs().max().item(), key=KEY, seed=SEED, chunk_frames=Tc, overlap_frames=To, N=2)
        for sizes in (_patterns(Ls)["2048"], _patterns(Ls)["ones"]):
            assert np.array_equal(_run_live(live, sig[0], sizes), want)
            live.reset()
    finally:
        full.dnn.set_precision("fp32")
    assert not np.array_equal(want, enhance_long(full, sig.cuda(), Tc, To, batch=1, N=2, noise_key=KEY, noise_seed=SEED))


# ---------------------------------------------------------------------------------------------------- 5
def test_norm_first_depends_on_the_signal_alone(full):
    Ls, Tc, To = 30000, 64, 16
    sig = _signal(13, Ls)
    sig[0, 20000] = 3.0                                             # a later peak that "first" never sees
    n0 = _ready_at(0, Tc, Tc - To)
    kw = dict(key=KEY, seed=SEED, chunk_frames=Tc, overlap_frames=To, N=2)
    live = LiveEnhancer(full, norm="first", **kw)
    outs = []
    for sizes in _patterns(Ls).values():
        outs.append(_run_live(live, sig[0], sizes))
        assert live.norm == sig[0, :n0].abs().max().item()
        live.reset()
        assert live.norm is None
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    fixed = LiveEnhancer(full, norm=sig[0, :n0].abs().max().item(), **kw)
    assert np.array_equal(_run_live(fixed, sig[0], [Ls]), outs[0])
    assert not np.array_equal(_run_live(LiveEnhancer(full, norm=3.0, **kw), sig[0], [Ls]), outs[0])
    # a recording that ends before chunk 0 is ready: the peak of all of it
    short = sig[:, :5000]
    assert np.array_equal(_run_live(live, short[0], [1000] * 5),
                          _run_live(LiveEnhancer(full, norm=short.abs().max().item(), **kw), short[0], [5000]))
    # an all-zero prefix: norm 1.0, finite output
    quiet = torch.cat([torch.zeros(1, n0), sig[:, :12000]], dim=1)
    live.reset()
    out = _run_live(live, quiet[0], _patterns(quiet.size(1))["2048"])
    assert live.norm == 1.0 and np.isfinite(out).all() and out.shape == (quiet.size(1),)


# ---------------------------------------------------------------------------------------------------- 6
def test_state_is_bounded(full):
    """40 chunks' worth in blocks of 2048 at (64, 16), N = 1: after chunk 3 and after chunk 39 the object reports the same
    state and the allocator holds no more."""
    Tc, To = 64, 16
    hop = Tc - To
    n = _ready_at(39, Tc, hop) + 100
    sig = _signal(17, n)
    live = LiveEnhancer(full, norm=0.5, key=KEY, seed=SEED, chunk_frames=Tc, overlap_frames=To, N=1)
    seen, done = {}, 0
    while done < n:
        out = live.push(sig[0, done:done + 2048].numpy())
        done += min(2048, n - done)
        ready = live_plan(live.samples_in, Tc, To)[0]
        if ready in (4, 40) and ready not in seen:
            del out
            seen[ready] = (live.state_bytes(), torch.cuda.memory_allocated())
    assert set(seen) == {4, 40}
    print(f"live state after chunk 3: {seen[4]}, after chunk 39: {seen[40]}")
    assert seen[4][0] == seen[40][0] > 0 and seen[40][1] <= seen[4][1]
    assert seen[4][0] < 4 * (128 * Tc + 382 + 2 * 2048) + 2 * 8 * 256 * Tc      # buffer of a window and a block, one chunk
    tail = live.finish()
    assert live.samples_out == n and np.isfinite(tail).all()
    # the geometry that keeps two chunks says so
    two = LiveEnhancer(full, norm=0.5, key=KEY, chunk_frames=128, overlap_frames=64, N=1)
    two.push(sig[0, :_ready_at(2, 128, 64)].numpy())
    assert two.state_bytes() >= 2 * 8 * 256 * 128


# ---------------------------------------------------------------------------------------------------- 7
def test_life_cycle_and_device_output(full):
    Ls, Tc, To = 40000, 64, 16
    sig = _signal(19, Ls)
    live = LiveEnhancer(full, norm=0.4, key=KEY, seed=SEED, chunk_frames=Tc, overlap_frames=To, N=2)
    with pytest.raises(ValueError, match="255"):
        live.finish()                                               # nothing pushed
    live.reset()
    live.push(np.zeros(255, dtype=np.float32))
    with pytest.raises(ValueError, match="255"):
        live.finish()
    live.reset()
    a = _run_live(live, sig[0], _patterns(Ls)["2048"])
    for call in (lambda: live.push(np.zeros(1, dtype=np.float32)), live.finish):
        with pytest.raises(RuntimeError, match="reset"):
            call()
    live.reset()
    assert (live.samples_in, live.samples_out) == (0, 0)
    assert np.array_equal(_run_live(live, sig[0], _patterns(Ls)["ones"]), a)
    # device tensors in, device tensors out
    live.reset()
    d = sig[0].cuda()
    parts = [live.push(d[i:i + 3000], as_tensor=True) for i in range(0, Ls, 3000)] + [live.finish(as_tensor=True)]
    assert all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 1 for p in parts)
    assert np.array_equal(torch.cat(parts).cpu().numpy(), a)
    for bad in (np.zeros(4, dtype=np.float64), np.zeros((2, 4), dtype=np.float32), [0.0, 1.0]):
        live.reset()
        with pytest.raises((TypeError, ValueError)):
            live.push(bad)


# ---------------------------------------------------------------------------------------------------- 8
def test_live_cli_in_a_child_process():
    """3 s of s16le through ``enhance --live``: 2 L bytes come back, the bytes of an in-process ``LiveEnhancer`` with the
    same settings through the same quantiser.  ``--synthetic 1`` names the weights, as in the other CLI tests: the committed
    checkpoint (tests/golden/tiny_ckpt.ckpt) is a 32-bin network (image_size 32), and the library refuses the STFT's 256 bins
    on it by name (``F=256 must equal image_size=32``), so no recording can go through it."""
    from flowmse_amd.evaluate import _load_model
    Ls = 48000
    t = np.arange(Ls) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * 220 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.05 * synth.normal(23, 9, (Ls,), 1.0)
    raw = pcm_encode(x.astype(np.float32), "s16le")
    assert len(raw) == 2 * Ls
    args = ["--live", "--synthetic", "1", "--seed", "3", "--live_block", "1000", "--chunk_frames", "64", "--overlap_frames", "16",
            "--live_norm", "0.5", "--N", "2"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "flowmse_amd.enhance"] + args, cwd=ROOT, input=raw,
                       capture_output=True)
    assert r.returncode == 0, f"exited with {r.returncode}:\n{r.stderr.decode(errors='replace')[-3000:]}"
    assert len(r.stdout) == 2 * Ls and b"live: enhanced 48000 samples" in r.stderr
    model, _ = _load_model(types.SimpleNamespace(synthetic=1, ckpt=None, test_dir="stdin", precision="fp32"), None)
    live = LiveEnhancer(model, norm=0.5, key=utterance_key("live"), seed=3, chunk_frames=64, overlap_frames=16, N=2)
    want = b"".join(pcm_encode(live.push(pcm_decode(raw[i:i + 2000], "s16le")), "s16le") for i in range(0, len(raw), 2000))
    want += pcm_encode(live.finish(), "s16le")
    assert r.stdout == want
    assert np.abs(np.frombuffer(want, dtype="<i2")).max() > 0
