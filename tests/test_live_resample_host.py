"""CPU: the streaming resampler's schedule (``stream_plan``) against plain enumeration of its definition, the CPU
``StreamResampler`` against the CPU ``resample`` under every push pattern, the live latency at other rates against a
brute-force count, the ``--live_rate`` command line, and the C-ABI surface and host-side argument checks of
``flowse_resample_poly_window`` (no GPU call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
PLAN_RATIOS = [(1, 3), (3, 1), (160, 441), (441, 160), (320, 441), (1, 2)]            # (up, down)
STREAM_RATES = [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000), (8000, 16000)]


def _q(n_outputs, up, down):
    """q(n) = (half + n down) div up for n < n_outputs: the last sample output n reads (the header's definition)."""
    half = 10 * max(up, down)
    return (half + np.arange(n_outputs, dtype=np.int64) * down) // up


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("up,down", PLAN_RATIOS, ids=lambda v: str(v))
def test_stream_plan_against_plain_enumeration(up, down):
    from flowmse_amd.resample import out_len, stream_plan
    n_max = 3000
    n_outputs = n_max * up // down + 2
    q = _q(n_outputs, up, down)
    assert (np.diff(q) >= 0).all()
    last_open = last_fin = 0
    seen_positive = False
    for n_in in range(n_max + 1):
        final = int(np.count_nonzero(q <= n_in - 1))                # outputs whose every sample has arrived
        exist = int(np.count_nonzero(np.arange(n_outputs, dtype=np.int64) * down < n_in * up))   # n < L up / down
        got, fin = stream_plan(n_in, up, down), stream_plan(n_in, up, down, finished=True)
        assert got == final and fin == exist == out_len(n_in, up, down), (n_in, got, final, fin, exist)
        assert isinstance(got, int) and last_open <= got <= fin and last_fin <= fin
        last_open, last_fin = got, fin
        seen_positive |= got > 0
    assert seen_positive and stream_plan(0, up, down) == 0 == stream_plan(0, up, down, finished=True)
    # an unreduced pair is the reduced one; equal rates pass every sample through; Python ints far past 2^31
    assert stream_plan(1000, 7 * up, 7 * down) == stream_plan(1000, up, down)
    assert stream_plan(123, 5, 5) == 123 == stream_plan(123, 5, 5, finished=True)
    big = 3 * 2 ** 40
    assert stream_plan(big, up, down) == (big * up - 1 - 10 * max(up, down)) // down + 1
    with pytest.raises(ValueError):
        stream_plan(-1, up, down)
    with pytest.raises(ValueError):
        stream_plan(10, 1, 1025)


# ---------------------------------------------------------------------------------------------------- 2
def _patterns(n, seed):
    """Push sizes that sum to n: all at once; single samples (n <= 2000 only); blocks of 2048; random sizes with zeros."""
    rng = np.random.default_rng(seed)
    rand, done = [0], 0
    while done < n:
        s = int(rng.choice([0, 1, 2, 17, 300, 1000, 5000]))
        s = min(s, n - done)
        rand.append(s)
        done += s
    rand.append(0)
    pats = {"whole": [n], "2048": [min(2048, n - i) for i in range(0, n, 2048)], "random": rand}
    if n <= 2000:
        pats["ones"] = [1] * n
    return pats


def _within_one_ulp(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((np.abs(a.astype(np.float64) - b.astype(np.float64))
                                        <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


@pytest.mark.parametrize("sr_in,sr_out", STREAM_RATES, ids=lambda v: str(v))
def test_cpu_stream_resampler_is_cpu_resample(sr_in, sr_out):
    from flowmse_amd.resample import StreamResampler, out_len, rational, resample, stream_plan
    up, down = rational(sr_in, sr_out)
    rs = StreamResampler(sr_in, sr_out)
    assert rs.state_bytes() == 0
    for n in (1, 9, 1200, 9000):                                    # 9 < P for every ratio here
        x = torch.randn(n, generator=torch.Generator().manual_seed(n + sr_in))
        want = resample(x[None], sr_in, sr_out)[0].numpy()
        for how, (name, sizes) in enumerate(_patterns(n, n + sr_out).items()):
            assert sum(sizes) == n
            parts, done = [], 0
            for i, s in enumerate(sizes):
                block = x[done:done + s]
                parts.append(rs.push((block.numpy(), block, block[None])[(how + i) % 3]))
                done += s
                assert rs.samples_in == done and rs.samples_out == stream_plan(done, up, down)
                assert parts[-1].dtype == np.float32 and parts[-1].ndim == 1
            parts.append(rs.finish())
            got = np.concatenate(parts)
            assert rs.samples_out == out_len(n, up, down) == got.shape[0]
            assert _within_one_ulp(got, want), (n, name, float(np.abs(got - want).max()))
            with pytest.raises(RuntimeError, match="reset"):
                rs.push(np.zeros(1, dtype=np.float32))
            with pytest.raises(RuntimeError, match="reset"):
                rs.finish()
            rs.reset()
        assert np.abs(want).max() > 0
    # the state follows the largest push and the filter, not the signal: 40 blocks of 500 hold what 4 blocks held
    rs, sizes = StreamResampler(sr_in, sr_out), []                  # a fresh one: reset() keeps the capacity
    for i in range(40):
        rs.push(np.zeros(500, dtype=np.float32))
        sizes.append(rs.state_bytes())
    P = (20 * max(up, down) + up) // up
    assert sizes[3] == sizes[39] <= 4 * (500 + P + down // up + 1)
    for bad in (np.zeros(4), np.zeros((2, 4), dtype=np.float32), [0.0]):
        with pytest.raises((TypeError, ValueError)):
            rs.push(bad)


def test_equal_rates_pass_samples_through_and_empty_signals_end():
    from flowmse_amd.resample import StreamResampler
    rs = StreamResampler(48000, 48000)
    x = np.arange(5, dtype=np.float32)
    assert rs.push(x).tobytes() == x.tobytes() and rs.push(x[:0]).shape == (0,) and rs.finish().shape == (0,)
    assert (rs.samples_in, rs.samples_out, rs.state_bytes()) == (5, 5, 0)
    t = torch.arange(3, dtype=torch.float32)
    rs.reset()
    assert rs.push(t, as_tensor=True) is t
    rs = StreamResampler(44100, 16000)
    assert rs.finish().shape == (0,)                                # nothing pushed: nothing comes out
    rs.reset()
    assert rs.push(np.zeros(0, dtype=np.float32)).shape == (0,) and rs.finish(as_tensor=True).shape == (0,)
    with pytest.raises(ValueError, match="16001"):
        StreamResampler(16001, 16000)


# ---------------------------------------------------------------------------------------------------- 3
def _ready_at(k, Tc, hop):
    """n_k from the frame definition: the last frame of chunk k, k hop + Tc - 1, reads samples up to 128 t + 254."""
    return 128 * (k * hop + Tc - 1) + 254 + 1


@pytest.mark.parametrize("Tc,To", [(64, 16), (64, 0)], ids=lambda v: str(v))
@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_latency_at_other_rates_is_the_worst_wait_of_the_three_schedules(rate, Tc, To):
    """For every chunk k of a long recording: the input samples that have arrived when it runs (the first count at which
    the 16 kHz sample n_k - 1 is final, by enumeration of q) minus the input samples already returned (the outputs of the
    back resampler final on the E_{k-1} samples returned at 16 kHz, by enumeration; at 16 kHz output, the input samples
    those cover).  Twice the horizon the formula walks gives the same worst case."""
    from flowmse_amd.live import latency_samples, live_plan
    from flowmse_amd.resample import rational
    hop = Tc - To
    up, down = rational(rate, 16000)
    chunks = 2 * up + 2
    n16 = _ready_at(chunks - 1, Tc, hop)
    q_in = _q(n16, up, down)                                        # 16 kHz sample m is final once input sample q_in[m] is in
    q_back = _q(n16 * down // up + 2, down, up)                     # input-rate output n reads 16 kHz samples up to q_back[n]
    for mode in ("16000", "input"):
        waits = []
        for k in range(chunks):
            n_k = _ready_at(k, Tc, hop)
            arrived = int(q_in[n_k - 1]) + 1
            assert live_plan(n_k - 1, Tc, To)[0] == k
            e = live_plan(n_k - 1, Tc, To)[1]                       # 16 kHz samples returned before chunk k runs
            returned = int(np.searchsorted(q_back, e - 1, side="right")) if mode == "input" else e * rate // 16000
            assert returned <= arrived
            waits.append(arrived - returned)
        got = latency_samples(Tc, rate, mode, To)
        assert got == max(waits) == max(waits[:up + 1]), (rate, mode, got, max(waits))
        assert got >= (128 * Tc + 382) * rate // 16000
    if rate == 48000:                                               # integer ratio: the closed form of the docstring
        assert latency_samples(Tc, rate, "input", To) == 3 * (128 * Tc + 382) + 58
        assert latency_samples(Tc, rate, "16000", To) == 3 * (128 * Tc + 382) + 28
    assert latency_samples(Tc) == latency_samples(Tc, 16000, "input", To) == 128 * Tc + 382


# ---------------------------------------------------------------------------------------------------- 4
def test_live_rate_command_line(capsys):
    from flowmse_amd import enhance
    a = enhance.parse_args(["--live", "--ckpt", "m.ckpt"])
    assert (a.live_rate, a.output_rate) == (16000, "16000")
    a = enhance.parse_args(["--live", "--synthetic", "1", "--live_rate", "48000", "--output_rate", "input"])
    assert (a.live, a.live_rate, a.output_rate, a.resample) == (True, 48000, "input", False)
    a = enhance.parse_args(["--live", "--ckpt", "m.ckpt", "--live_rate", "44100"])
    assert (a.live_rate, a.output_rate) == (44100, "16000")
    a = enhance.parse_args(["--live", "--ckpt", "m.ckpt", "--output_rate", "input"])       # at 16 kHz: a no-op, as before
    assert (a.live_rate, a.output_rate) == (16000, "input")
    for argv, words in [(["--output", "o", "--synthetic", "1", "--live_rate", "48000"], ["--live_rate 48000", "needs --live"]),
                        (["--live", "--ckpt", "m.ckpt", "--live_rate", "16001"], ["--live_rate", "16001 Hz", "1024"]),
                        (["--live", "--ckpt", "m.ckpt", "--live_rate", "0"], ["--live_rate", "positive"]),
                        (["--live", "--ckpt", "m.ckpt", "--live_rate", "48000", "--resample"],
                         ["--live does not take --resample"]),
                        (["--live", "--ckpt", "m.ckpt", "--resample"], ["--live does not take --resample"])]:
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (argv, err)


def test_live_enhancer_checks_its_rates_first():
    import types
    from flowmse_amd.data_module import SpecTransform
    from flowmse_amd.live import LiveEnhancer
    model = types.SimpleNamespace(data_module=SpecTransform(), dnn=torch.nn.Identity())
    with pytest.raises(ValueError, match="output_rate"):
        LiveEnhancer(model, norm=1.0, key=1, output_rate="48000")
    with pytest.raises(ValueError, match="16001"):
        LiveEnhancer(model, norm=1.0, key=1, input_rate=16001)
    with pytest.raises(RuntimeError, match="HIP"):                  # and then, as at 16 kHz, there is no CPU path
        LiveEnhancer(model, norm=1.0, key=1, input_rate=48000, output_rate="input")


# ---------------------------------------------------------------------------------------------------- 5
def test_cabi_declares_and_exports_the_window_resampler():
    from flowmse_amd import _lib
    name = "flowse_resample_poly_window"
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    assert "stream capture" in header[header.index(name):header.index("int flowse_resample_num_taps")]
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(decl.split(",")) == 10 and getattr(_lib.lib, name).argtypes == args
    kinds = [C.c_int64 if "int64_t" in a else C.c_int if re.search(r"\bint\b", a) else C.c_void_p for a in decl.split(",")]
    assert kinds == args
    assert _lib.lib.flowse_abi_version() == 3
    assert re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)


def test_window_entry_refuses_bad_arguments_before_any_device_call():
    from flowmse_amd import _lib
    L, p = _lib.lib, C.c_void_p(256)

    def call(win=p, m0=0, n_win=100, L_total=-1, up=1, down=3, out=p, n0=0, n_out=1):
        return L.flowse_resample_poly_window(win, m0, n_win, L_total, up, down, out, n0, n_out, None)

    for kw in (dict(win=None), dict(out=None), dict(m0=-1), dict(n_win=-1), dict(n0=-1), dict(n_out=-1), dict(L_total=-2),
               dict(up=0), dict(down=-3)):
        assert call(**kw) == ERR_ARG, kw
        assert b"flowse_resample_poly_window" in L.flowse_last_error()
    assert call(up=1, down=1025) == ERR_SHAPE and b"1024" in L.flowse_last_error()
    assert call(up=16000, down=16001) == ERR_SHAPE
    assert call(m0=2 ** 51) == ERR_SHAPE and call(n_out=2 ** 31) == ERR_SHAPE
    # 1 / 3: half = 30, P = 61, q(n) = 30 + 3 n.  Open: output 23 reads sample 99, output 24 sample 102
    assert call(n_out=25) == ERR_SHAPE
    msg = L.flowse_last_error()
    assert b"open" in msg and b"102" in msg and b"[0, 100)" in msg
    # a window that starts after the first sample read: output 20 reads [90 - 60, 90]
    assert call(m0=31, n_win=69, n0=20, n_out=1) == ERR_SHAPE
    msg = L.flowse_last_error()
    assert b"[30, 90]" in msg and b"[31, 100)" in msg
    # closed: the window or the outputs past the end (100 samples have 34 outputs)
    assert call(L_total=99) == ERR_SHAPE and b"99" in L.flowse_last_error()
    assert call(L_total=100, n0=30, n_out=5) == ERR_SHAPE and b"34" in L.flowse_last_error()
    # closed: output 33 reads [69, 129], clamped to [69, 99]; a window from 70 is one sample short
    assert call(L_total=100, m0=70, n_win=30, n0=33, n_out=1) == ERR_SHAPE
    assert b"[69, 99]" in L.flowse_last_error()
    # equal rates: the outputs are the samples themselves and must lie in the window
    assert call(up=5, down=5, m0=10, n_win=20, n0=9, n_out=3) == ERR_SHAPE
    assert call(up=5, down=5, m0=10, n_win=20, n0=28, n_out=3) == ERR_SHAPE
    # nothing to write: OK, and nothing is launched (there is no device here to launch on)
    assert call(n_out=0) == 0 and call(L_total=100, n0=34, n_out=0) == 0
