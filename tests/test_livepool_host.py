"""Host side of the live pool (flowmse_amd.livepool; no GPU): ``plan_step`` against a brute-force restatement of its rules,
the session counters against ``live.live_plan``, the argument errors by name, the interleave helpers, the C ABI surface of
the two row-table window entries and the ``--live_channels`` refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from flowmse_amd import _lib, enhance
from flowmse_amd.chunked import plan_chunks
from flowmse_amd.live import live_plan, pcm_decode, pcm_deinterleave, pcm_encode, pcm_interleave
from flowmse_amd.livepool import MAX_WIDTH, LivePool, SessionPlan, check_width, plan_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n(k, Tc, hop):
    """Samples at which chunk k is ready: its last frame k hop + Tc - 1 needs 128 t + 255 samples."""
    return 128 * (k * hop + Tc - 1) + 255


def _sessions(Tc, To):
    """(channels, samples pushed, chunks already sampled, finished): several sessions at different chunk indices, one
    finished with chunks waiting, one finished with K == 1 (a width of its own at Tc = 128), one with nothing ready."""
    hop = Tc - To
    return [(1, _n(0, Tc, hop), 0, False),                          # chunk 0 just became ready
            (2, _n(4, Tc, hop) + 99, 3, False),                     # chunks 3 and 4 wait, two channels
            (1, _n(2, Tc, hop) + 5000, 1, True),                    # finished: every remaining chunk is ready
            (3, 5000, 0, True),                                     # finished, K == 1: one row per channel, T = 40 -> width 64
            (1, _n(0, Tc, hop) - 1, 0, False),                      # one sample short of chunk 0
            (1, _n(7, Tc, hop), 8, False)]                          # everything sampled


def _plans(Tc, To):
    plans = []
    for channels, n, done, finished in _sessions(Tc, To):
        p = SessionPlan(list(range(10, 10 + channels)), 1.0, Tc, To)
        p.accept((channels, n))
        for k in range(done):
            p.sampled(k)
        if finished:
            p.finish()
        plans.append(p)
    return plans


def _brute_rows(Tc, To):
    """{width: [(session, chunk, channel, frame0)]} from the rules, written out sample by sample and chunk by chunk."""
    hop = Tc - To
    buckets = {}
    for i, (channels, n, done, finished) in enumerate(_sessions(Tc, To)):
        T = n // 128 + 1
        if finished and T <= Tc:                                    # one chunk: the pad_spec width
            todo, width = ([0] if done == 0 else []), 64 * ((T + 63) // 64)
        elif finished:
            K = 1
            while (K - 1) * hop + Tc < T:
                K += 1
            todo, width = list(range(done, K)), Tc
        else:
            todo, width = [k for k in range(done, 1000) if n >= _n(k, Tc, hop)], Tc
            assert todo == list(range(done, done + len(todo)))
        for k in todo:
            for c in range(channels):
                buckets.setdefault(width, []).append((i, k, c, k * hop))
    return buckets


@pytest.mark.parametrize("W", [1, 3, 4])
@pytest.mark.parametrize("Tc,To", [(64, 16), (128, 64)], ids=lambda v: str(v))
def test_plan_step_against_the_rules(Tc, To, W):
    want = _brute_rows(Tc, To)
    assert (sorted(want) == [64]) if Tc == 64 else (sorted(want) == [64, 128])    # the K == 1 rows share or own a bucket
    calls = plan_step(_plans(Tc, To), W)
    assert all(len(c.rows) == W for c in calls)                     # exactly W rows, always
    widths = [c.width for c in calls]
    assert widths == sorted(widths) and set(widths) == set(want)    # buckets in ascending width
    for width, rows in want.items():
        mine = [c for c in calls if c.width == width]
        real = [tuple(r[:4]) for c in mine for r in c.rows if not r.filler]
        assert real == rows                                         # sessions in order, chunk-major, channels together
        fillers = [r for c in mine for r in c.rows if r.filler]
        assert len(fillers) == -len(rows) % W <= W - 1
        for c in mine[:-1]:
            assert not any(r.filler for r in c.rows)                # only the bucket's last call is filled ...
        last = mine[-1].rows
        assert not last[0].filler and all(r == last[0]._replace(filler=True) for r in last if r.filler)    # ... by its first row
        assert [r.filler for r in last] == sorted(r.filler for r in last)
    # sessions with nothing ready contribute nothing, and an empty pool plans nothing
    assert not any(r.session in (4, 5) for c in calls for r in c.rows)
    assert plan_step([], W) == [] and plan_step(_plans(Tc, To)[4:], W) == []


@pytest.mark.parametrize("Tc,To", [(64, 16), (128, 64), (64, 0)], ids=lambda v: str(v))
def test_session_counters_follow_live_plan(Tc, To):
    """After every push, the chunks a session offers are those ``live_plan`` counts, and once they are sampled its counters
    are ``live_plan``'s -- for every push pattern."""
    n = 60000
    patterns = {"whole": [n], "2048": [2048] * 30, "ones": [1] * 300 + [4097] * 15, "empties": [0, 777, 0, 3001, 5] * 16}
    for sizes in patterns.values():
        p = SessionPlan(5, "first", Tc, To)
        for s in sizes:
            assert p.accept((s,)) == s
            ready, final = live_plan(p.samples_in, Tc, To)
            assert [k for k, _ in p.pending()] == list(range(p.k, ready)) and all(w == Tc for _, w in p.pending())
            if s % 2:                                               # a step now, or later: the counters catch up either way
                for k, _ in p.pending():
                    p.sampled(k)
                assert (p.k, p.samples_out) == (ready, final)
        p.finish()
        K = live_plan(p.samples_in, Tc, To, finished=True)[0]
        assert (p.L, p.K) == (p.samples_in, K) == (sum(sizes), plan_chunks(sum(sizes) // 128 + 1, Tc, To)[0])
        assert [k for k, _ in p.pending()] == list(range(p.k, K)) and not p.closed
        for k, _ in p.pending():
            p.sampled(k)
        assert p.samples_out == p.samples_in and p.closed and p.pending() == []
    # K == 1: one row of the pad_spec width, and the whole recording with it
    p = SessionPlan([1, 2], 0.5, Tc, To)
    p.accept((2, 5000))
    assert p.pending() == []
    p.finish()
    assert p.K == 1 and p.pending() == [(0, 64)]
    p.sampled(0)
    assert p.samples_out == 5000 and p.closed


def test_argument_errors_by_name():
    for bad in (0, MAX_WIDTH + 1, -3):
        with pytest.raises(ValueError, match="width"):
            check_width(bad)
        with pytest.raises(ValueError, match="width"):
            LivePool(None, width=bad)                               # before the model is looked at
        with pytest.raises(ValueError, match="width"):
            plan_step([], bad)
    assert MAX_WIDTH == _lib.FLOWSE_MAX_WINDOW_ROWS and check_width(MAX_WIDTH) == MAX_WIDTH
    with pytest.raises(ValueError, match="chunk_frames"):
        LivePool(None, width=2, chunk_frames=100)
    with pytest.raises(RuntimeError, match="HIP"):
        LivePool(None, width=2)                                     # no CPU fallback
    for bad in (None, [], [1, "a"], [1, -1], 1 << 64, 1.5):
        with pytest.raises((ValueError, TypeError), match="keys"):
            SessionPlan(bad, 1.0, 64, 16)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "peak"):
        with pytest.raises(ValueError, match="norm"):
            SessionPlan(1, bad, 64, 16)
    assert SessionPlan(np.uint64(7), "first", 64, 16).keys == (7,) and SessionPlan([1, 2, 3], 2, 64, 16).channels == 3
    p = SessionPlan([1, 2], 1.0, 64, 16)
    for shape in ((100,), (1, 100), (3, 100), (2, 3, 4), ()):
        with pytest.raises(ValueError, match="2 channels"):
            p.accept(shape)
    assert p.samples_in == 0 and p.accept((2, 100)) == 100
    with pytest.raises(ValueError, match="255"):
        p.finish()
    mono = SessionPlan(1, 1.0, 64, 16)
    assert mono.accept((300,)) == 300 and mono.accept((1, 10)) == 10
    with pytest.raises(ValueError, match="1 channel"):
        mono.accept((2, 10))
    mono.finish()
    with pytest.raises(RuntimeError, match="after finish"):
        mono.accept((10,))
    with pytest.raises(RuntimeError, match="twice"):
        mono.finish()


@pytest.mark.parametrize("fmt", ["s16le", "f32le"])
def test_interleave_round_trip(fmt):
    rng = np.random.default_rng(3)
    for channels in (1, 2, 5):
        x = (rng.integers(-32768, 32768, size=(channels, 1001)) / 32768.0).astype(np.float32)
        flat = pcm_interleave(x)
        assert flat.shape == (channels * 1001,) and flat.flags.c_contiguous
        assert flat[channels:2 * channels].tolist() == x[:, 1].tolist()               # frame after frame
        back = pcm_deinterleave(flat, channels)
        assert back.flags.c_contiguous and np.array_equal(back, x)
        raw = pcm_encode(flat, fmt)
        assert pcm_encode(pcm_interleave(pcm_deinterleave(pcm_decode(raw, fmt), channels)), fmt) == raw
        # samples past the last whole frame are ignored
        assert np.array_equal(pcm_deinterleave(np.concatenate([flat, flat[:channels - 1]]), channels), x)
    with pytest.raises(ValueError):
        pcm_deinterleave(np.zeros(4, dtype=np.float32), 0)
    with pytest.raises(ValueError):
        pcm_interleave(np.zeros(4, dtype=np.float32))


SIZES = {"int64_t": 8, "int32_t": 4, "float": 4}


def _header_layout(header, name):
    """[(field, offset)], size of ``struct name`` in the header under the natural alignment of the C ABI."""
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", header, flags=re.S).group(1)
    fields, off, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(?:const\s+)?(\w+)\s*(.*)$", decl, flags=re.S)
        base, names = m.group(1), [s.strip() for s in m.group(2).split(",")]
        for field in names:
            size = 8 if field.startswith("*") or base.endswith("*") else SIZES[base]
            off = -(-off // size) * size
            fields.append((field.lstrip("* "), off))
            off += size
            align = max(align, size)
    return fields, -(-off // align) * align


def test_cabi_declares_and_exports_the_window_rows_calls():
    text = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("flowse_stft_compress_window_rows", "flowse_istft_decompress_window_rows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.flowse_abi_version() == 3 and re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)
    assert re.search(r"#define\s+FLOWSE_MAX_WINDOW_ROWS\s+16\b", header) and _lib.FLOWSE_MAX_WINDOW_ROWS == 16
    for name, size in (("flowse_window_row", 48), ("flowse_window_out", 72)):
        fields, total = _header_layout(header, name)
        struct = getattr(_lib, name)
        assert [f for f, _ in fields] == [f for f, _ in struct._fields_], name
        assert [(f, getattr(struct, f).offset) for f, _ in struct._fields_] == fields, name
        assert ctypes.sizeof(struct) == total == size               # 16 by value: 768 and 1152 bytes of the argument block
    # argument errors are answered before any device call
    out = ctypes.create_string_buffer(8)
    rows = (_lib.flowse_window_row * 17)()
    assert _lib.lib.flowse_stft_compress_window_rows(None, 1, 64, out, 0.15, 0.5, None) == 1
    assert _lib.lib.flowse_stft_compress_window_rows(rows, 1, 64, None, 0.15, 0.5, None) == 1
    assert _lib.lib.flowse_stft_compress_window_rows(rows, 0, 64, out, 0.15, 0.5, None) == 4
    assert _lib.lib.flowse_stft_compress_window_rows(rows, 17, 64, out, 0.15, 0.5, None) == 4
    assert _lib.lib.flowse_stft_compress_window_rows(rows, 2, 64, out, 0.15, 0.5, None) == 1          # null buf
    assert b"row 0" in _lib.lib.flowse_last_error()
    rows[0].buf, rows[0].n, rows[0].L_total = ctypes.addressof(out), 8, -1
    assert _lib.lib.flowse_stft_compress_window_rows(rows, 1, 64, out, 0.15, 0.5, None) == 4          # frames past the window
    assert b"stft window rows: row 0" in _lib.lib.flowse_last_error()
    outs = (_lib.flowse_window_out * 17)()
    assert _lib.lib.flowse_istft_decompress_window_rows(None, 1, 64, 48, 0.15, 0.5, None) == 1
    assert _lib.lib.flowse_istft_decompress_window_rows(outs, 0, 64, 48, 0.15, 0.5, None) == 4
    assert _lib.lib.flowse_istft_decompress_window_rows(outs, 17, 64, 48, 0.15, 0.5, None) == 4
    assert _lib.lib.flowse_istft_decompress_window_rows(outs, 1, 64, 48, 0.15, 0.5, None) == 1        # null cur_c64 / out
    outs[0].cur_c64 = outs[0].out = ctypes.addressof(out)
    outs[0].n_out = 0
    assert _lib.lib.flowse_istft_decompress_window_rows(outs, 1, 64, 48, 0.15, 0.5, None) == 4
    assert b"istft window rows: row 0" in _lib.lib.flowse_last_error()


def test_live_channels_command_line(capsys):
    a = enhance.parse_args(["--live", "--ckpt", "m.ckpt"])
    assert a.live_channels == 1
    a = enhance.parse_args(["--live", "--synthetic", "1", "--live_channels", "2"])
    assert a.live_channels == 2
    for argv, word in ((["--live", "--synthetic", "1", "--live_channels", "0"], "--live_channels"),
                       (["--live", "--synthetic", "1", "--live_channels", "17"], "--live_channels"),
                       (["--live", "--synthetic", "1", "--live_channels", "2", "--live_rate", "48000"], "--live_rate 48000"),
                       (["--output", "o", "--synthetic", "1", "--live_channels", "2"], "needs --live")):
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and word in err and "--live_channels" in err, argv
    # one channel at another rate is today's path
    assert enhance.parse_args(["--live", "--synthetic", "1", "--live_rate", "48000"]).live_channels == 1
