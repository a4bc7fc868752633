"""Host side of the live pool at other sample rates (no GPU): the C ABI surface of ``flowse_resample_poly_window_rows``,
``resample.plan_flush``, ``RowsResampler`` on the CPU against ``StreamResampler`` on the CPU row by row, the
``SessionPlan`` counters at 48 and 44.1 kHz against ``stream_plan`` / ``live_plan`` / ``latency_samples``, and the
``--live_resample`` command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from flowmse_amd import _lib, enhance
from flowmse_amd.live import latency_samples, live_plan
from flowmse_amd.livepool import SessionPlan, plan_step
from flowmse_amd.resample import (MAX_ROWS, RowsResampler, StreamResampler, flush, out_len, plan_flush, rational,
                                  stream_plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_rows_entry_surface():
    with open(os.path.join(ROOT, "include", "flowse_hip.h")) as f:
        header = f.read()
    assert hasattr(_lib.lib, "flowse_resample_poly_window_rows")
    assert re.search(r"int\s+flowse_resample_poly_window_rows\(const flowse_resample_row\* rows, int R, int up, int down, "
                     r"void\* stream\);", header)
    cap = int(re.search(r"#define\s+FLOWSE_MAX_RESAMPLE_ROWS\s+(\d+)", header).group(1))
    assert cap == _lib.FLOWSE_MAX_RESAMPLE_ROWS == MAX_ROWS == 32
    assert ctypes.sizeof(_lib.flowse_resample_row) == 56
    assert [n for n, _ in _lib.flowse_resample_row._fields_] == ["win", "m0", "n_win", "L_total", "out", "n0", "n_out"]
    assert _lib.lib.flowse_abi_version() == 3                       # an additive entry: the version stays
    # the argument errors are answered on the host, before any device call
    rows = (_lib.flowse_resample_row * (cap + 1))()
    fn = _lib.lib.flowse_resample_poly_window_rows
    assert fn(None, 1, 1, 3, None) == ERR_ARG and b"flowse_resample_poly_window_rows" in _lib.lib.flowse_last_error()
    assert fn(rows, 0, 1, 3, None) == ERR_SHAPE and fn(rows, cap + 1, 1, 3, None) == ERR_SHAPE
    assert str(cap).encode() in _lib.lib.flowse_last_error()
    assert fn(rows, 2, 1, 3, None) == ERR_ARG and b"row 0" in _lib.lib.flowse_last_error()          # null win and out
    mem = (ctypes.c_float * 64)()
    for r in range(3):
        rows[r].win = rows[r].out = ctypes.addressof(mem)
        rows[r].m0, rows[r].n_win, rows[r].L_total, rows[r].n0, rows[r].n_out = 0, 64, -1, 0, 0
    assert fn(rows, 3, 1, 3, None) == 0                             # no outputs anywhere: nothing is launched
    rows[2].win = None
    assert fn(rows, 3, 1, 3, None) == ERR_ARG and b"row 2" in _lib.lib.flowse_last_error()
    rows[2].win = ctypes.addressof(mem)
    rows[1].n_out = 30                                              # q(29) = (30 + 87) // 1 = 117: not in the window
    assert fn(rows, 3, 1, 3, None) == ERR_SHAPE
    msg = _lib.lib.flowse_last_error()
    assert b"row 1" in msg and b"117" in msg
    rows[1].n_out, rows[1].L_total = 8, 10                          # closed: the window passes the signal's end
    assert fn(rows, 3, 1, 3, None) == ERR_SHAPE and b"row 1" in _lib.lib.flowse_last_error()
    assert fn(rows, 3, 1, 3000, None) == ERR_SHAPE and b"1024" in _lib.lib.flowse_last_error()
    assert fn(rows, 3, 0, 3, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------------- plan_flush
def test_plan_flush_groups_by_ratio_and_cuts_at_32():
    a, b = torch.device("cuda", 0), torch.device("cuda", 1)
    entries = [(a, 1, 3, 2, 100),            # 0: stereo, 48 kHz in
               (a, 160, 441, 1, 7),          # 1: 44.1 kHz in
               (a, 1, 3, 1, 0),              # 2: nothing new: no row
               (a, 3, 1, 2, 50),             # 3: the way back is another ratio
               (a, 1, 1, 4, 99),             # 4: equal rates pass through: no row
               (b, 1, 3, 1, 5),              # 5: another device is another group
               (a, 1, 3, 3, 1)]              # 6: joins the first group
    plan = plan_flush(entries)
    assert plan == [((a, 1, 3), [(0, 0), (0, 1), (6, 0), (6, 1), (6, 2)]), ((a, 160, 441), [(1, 0)]),
                    ((a, 3, 1), [(3, 0), (3, 1)]), ((b, 1, 3), [(5, 0)])]
    assert plan_flush([]) == [] and plan_flush([(a, 1, 3, 5, 0)]) == []
    # 69 rows of one ratio in streams of 1, 2 and 3 rows: tables of 32, 32 and 5, in stream and row order
    many = [(a, 1, 3, 1 + i % 3, 10) for i in range(35)]
    rows = [(i, r) for i in range(35) for r in range(1 + i % 3)]
    assert len(rows) == 69
    plan = plan_flush(many)
    assert [len(t) for _, t in plan] == [32, 32, 5] and [k for k, _ in plan] == [(a, 1, 3)] * 3
    assert [x for _, t in plan for x in t] == rows
    assert [len(t) for _, t in plan_flush(many, max_rows=64)] == [64, 5]
    # exactly 32 rows make one table, 33 make two
    assert [len(t) for _, t in plan_flush([(a, 1, 3, 32, 1)])] == [32]
    assert [len(t) for _, t in plan_flush([(a, 1, 3, 32, 1), (a, 2, 6, 1, 1)])] == [32, 1]


# ---------------------------------------------------------------------------------------------------- RowsResampler, CPU
def _sizes(n, seed):
    """Push sizes that sum to n, with empty and single-sample pushes."""
    rng = np.random.default_rng(seed)
    sizes, done = [0, 1, 1, 0], 2
    while done < n:
        s = min(int(rng.choice([0, 1, 2, 17, 300, 1000])), n - done)
        sizes.append(s)
        done += s
    return sizes + [0]


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (44100, 16000), (16000, 48000), (16000, 44100)], ids=lambda v: str(v))
def test_rows_resampler_on_the_cpu_is_the_stream_resampler_row_by_row(sr_in, sr_out):
    up, down = rational(sr_in, sr_out)
    n, C = 2600, 3
    x = torch.randn(C, n, generator=torch.Generator().manual_seed(sr_in + sr_out))
    for pattern in ([n], _sizes(n, 1), _sizes(n, 2)):
        rows = RowsResampler(sr_in, sr_out, C)
        single = [StreamResampler(sr_in, sr_out) for _ in range(C)]
        got, want, done = [], [[] for _ in range(C)], 0
        for i, s in enumerate(pattern):
            piece = x[:, done:done + s]
            assert rows.pending() == 0
            rows.append(piece.numpy() if i % 2 else piece)
            assert rows.pending() == stream_plan(done + s, up, down) - rows.samples_out
            got.append(rows.push(np.zeros((C, 0), dtype=np.float32), as_tensor=True))
            for c in range(C):
                want[c].append(single[c].push(piece[c], as_tensor=True))
            done += s
            assert (rows.samples_in, rows.samples_out) == (done, stream_plan(done, up, down)) == (single[0].samples_in, single[0].samples_out)
            assert rows._n == single[0]._n and rows._m0 == single[0]._m0          # the same samples are kept
        assert rows.pending(finished=True) == out_len(n, up, down) - rows.samples_out
        got.append(rows.finish(as_tensor=True))
        got = torch.cat(got, dim=1)
        assert got.shape == (C, out_len(n, up, down)) and got.dtype == torch.float32 and rows.finished
        for c in range(C):
            want[c].append(single[c].finish(as_tensor=True))
            assert torch.equal(got[c], torch.cat(want[c])), (c, pattern[:6])
        assert float(got.abs().max()) > 0
        assert rows.state_bytes() == 4 * C * rows._buf.size(1) <= 4 * C * (rows.P - 1 + max(pattern))
        with pytest.raises(RuntimeError, match="finish"):
            rows.finish()
        with pytest.raises(RuntimeError, match="reset"):
            rows.append(x[:, :1])


def test_flush_of_several_cpu_streams_and_equal_rates():
    x = torch.randn(2, 1500, generator=torch.Generator().manual_seed(5))
    a, b, same = RowsResampler(48000, 16000, 2), RowsResampler(44100, 16000, 1), RowsResampler(16000, 16000, 2)
    ref_a = [StreamResampler(48000, 16000) for _ in range(2)]
    ref_b = StreamResampler(44100, 16000)
    a.append(x[:, :700])
    b.append(x[0, :900])                                            # 1-D at one row
    same.append(x[:, :10])
    stats = {}
    oa, ob, os_ = flush([a, b, same], stats=stats)
    assert stats == {"resample_launches": 0}                        # the CPU path launches nothing
    assert torch.equal(os_, x[:, :10]) and same.samples_out == 10 and same._n == 0
    assert all(torch.equal(oa[c], ref_a[c].push(x[c, :700], as_tensor=True)) for c in range(2)) and oa.size(1) > 200
    assert torch.equal(ob[0], ref_b.push(x[0, :900], as_tensor=True))
    a.append(x[:, 700:])
    oa2, ob2 = flush([a, b], finished=[b])
    assert b.finished and not a.finished and torch.equal(ob2[0], ref_b.finish(as_tensor=True))
    assert all(torch.equal(oa2[c], ref_a[c].push(x[c, 700:], as_tensor=True)) for c in range(2))
    with pytest.raises(ValueError, match="twice"):
        flush([a, a])
    with pytest.raises(ValueError, match="finished"):
        flush([a], finished=[same])
    with pytest.raises(RuntimeError, match="finished before"):
        flush([a, b])
    with pytest.raises(ValueError, match=r"\[2, n\]"):
        a.append(x[0])
    with pytest.raises(TypeError, match="float32"):
        a.append(x.double())
    with pytest.raises(ValueError, match="rows"):
        RowsResampler(48000, 16000, 0)
    with pytest.raises(ValueError, match="16000 Hz -> 16001 Hz"):
        RowsResampler(16000, 16001, 1)


# ---------------------------------------------------------------------------------------------------- SessionPlan
@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("mode", ["16000", "input"])
def test_session_plan_counts_at_its_rate(rate, mode):
    Tc, To = 64, 16
    up, down = rational(rate, 16000)
    p = SessionPlan([1, 2], "first", Tc, To, input_rate=rate, output_rate=mode)
    assert (p.input_rate, p.output_rate, p.up, p.down) == (rate, mode, up, down)
    assert p.latency_samples == latency_samples(Tc, rate, mode, To) > 128 * Tc + 382
    pushed, sampled = 0, 0
    rng = np.random.default_rng(rate)
    for _ in range(60):
        n = int(rng.choice([0, 1, 999, 6144, 20000]))
        assert p.accept((2, n)) == n
        pushed += n
        assert p.pushed == pushed and p.samples_in == stream_plan(pushed, up, down)
        ready, final = live_plan(p.samples_in, Tc, To)
        todo = p.pending()
        assert todo == [(k, Tc) for k in range(sampled, ready)]
        assert len(plan_step([p], 4)) == -(-2 * len(todo) // 4)
        for k, _ in todo:
            p.sampled(k)
        sampled = ready
        assert p.samples_out == final
    assert sampled > 3
    p.finish()
    L = out_len(pushed, up, down)
    assert p.samples_in == L == p.L and p.K == live_plan(L, Tc, To, finished=True)[0]
    for k, _ in p.pending():
        p.sampled(k)
    assert p.closed and p.samples_out == L
    # the 16 kHz default is the plan as it was: pushed samples are the 16 kHz samples
    q = SessionPlan(7, 1.0, Tc, To)
    q.accept((12345,))
    assert (q.input_rate, q.output_rate, q.pushed, q.samples_in) == (16000, "16000", 12345, 12345)
    assert q.latency_samples == 128 * Tc + 382


def test_session_plan_refusals_at_other_rates():
    # finish() counts at 16 kHz: 600 samples at 48 kHz are 200
    p = SessionPlan(1, 1.0, 64, 16, input_rate=48000)
    p.accept((600,))
    with pytest.raises(ValueError, match="255.*got 200"):
        p.finish()
    p.accept((168,))                                                # 768 / 3 = 256
    p.finish()
    assert p.L == 256 and p.K == 1
    with pytest.raises(ValueError, match="16001"):                  # a ratio beyond the resampler, by name
        SessionPlan(1, 1.0, 64, 16, input_rate=16001)
    with pytest.raises(ValueError, match="input_rate"):
        SessionPlan(1, 1.0, 64, 16, input_rate=0)
    with pytest.raises(ValueError, match="output_rate"):
        SessionPlan(1, 1.0, 64, 16, input_rate=48000, output_rate="48000")


# ---------------------------------------------------------------------------------------------------- command line
def test_live_resample_command_line(capsys):
    base = ["--live", "--synthetic", "1"]
    a = enhance.parse_args(base + ["--live_channels", "2", "--live_rate", "48000", "--live_resample"])
    assert a.live_resample and a.live_channels == 2 and a.live_rate == 48000 and a.output_rate == "16000"
    a = enhance.parse_args(base + ["--live_channels", "2", "--live_rate", "44100", "--live_resample", "--output_rate", "input"])
    assert a.live_resample and a.output_rate == "input"
    assert not enhance.parse_args(base).live_resample
    for argv, words in ((["--output", "o", "--synthetic", "1", "--live_resample"], ("--live_resample", "needs --live")),
                        (base + ["--live_channels", "2", "--live_resample"], ("--live_resample", "--live_rate", "16000")),
                        (base + ["--live_rate", "48000", "--live_resample"], ("--live_resample", "--live_channels")),
                        (base + ["--live_channels", "2", "--live_rate", "16001", "--live_resample"], ("--live_rate", "16001")),
                        (base + ["--live_channels", "2", "--live_rate", "48000"], ("--live_rate 48000", "--live_resample"))):
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (argv, err)
