"""GPU: live enhancement at other sample rates -- ``flowse_resample_poly_window`` against the whole-signal kernel bit for
bit from the smallest legal windows, its outputs far past 2^31 against float64 under the derived bound, the device
``StreamResampler`` against ``resample`` bit for bit under every push pattern with bounded state, ``LiveEnhancer(input_rate,
output_rate)`` against ``enhance_recording`` bit for bit, and ``--live --live_rate`` in one child process under its own time
limit.  No test asserts a time.

The bound of the far-index test is the one of tests/test_gpu_resample.py: an output is a P-term fp32 fmaf chain of
fp32-rounded taps times fp32 samples, so |out[n] - ref[n]| <= (P + 2) 2^-24 S[n], S[n] = sum_j |H[p][j]| |x[q - j]|."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from flowmse_amd import _lib
from flowmse_amd.live import LiveEnhancer, latency_samples, pcm_decode, pcm_encode
from flowmse_amd.resample import (StreamResampler, design_taps, out_len, rational, resample, resample_reference,
                                  stream_plan)
from flowmse_amd.util import synth
from flowmse_amd.util.noise import utterance_key

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
U = 2.0 ** -24
KEY, SEED = 0x912975D344AF26C6, 0x1F2E3D4C5B6A7988
# the ratios of RATE_CASES and PATH_CASES in tests/test_gpu_resample.py (the four launch forms: a run of 256 outputs, the
# table through L2, the input from global memory, both), at lengths that give a window of more than one block
WINDOW_CASES = [(48000, 16000, 9001), (44100, 16000, 8000), (22050, 16000, 4000), (8000, 16000, 1500), (16000, 48000, 1100),
                (16000, 44100, 1200), (192000, 16000, 20000), (16384, 16368, 3000), (384000, 16000, 30000),
                (1024000, 1000, 300000)]


def _geometry(up, down):
    half = 10 * max(up, down)
    return half, -(-(2 * half + 1) // up)


def _samples_read(n0, n1, up, down, length):
    """[lo, hi): the samples of the signal the outputs [n0, n1) read, by enumerating q(n) - j over all P taps of every
    output and keeping what lies in the signal (``length`` None: it is open and has no end)."""
    half, P = _geometry(up, down)
    q = (half + np.arange(n0, n1, dtype=np.int64) * down) // up
    m = (q[:, None] - np.arange(P, dtype=np.int64)[None, :]).reshape(-1)
    m = m[(m >= 0) & ((m < length) if length is not None else True)]
    return int(m.min()), int(m.max()) + 1


def _window(win, m0, L_total, up, down, out, n0):
    return L.flowse_resample_poly_window(_lib.ptr(win), m0, win.numel(), L_total, up, down, _lib.ptr(out), n0, out.numel(),
                                         _lib.current_stream())


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("sr_in,sr_out,n", WINDOW_CASES, ids=lambda v: str(v))
def test_window_entry_is_the_whole_signal_kernel_bit_for_bit(sr_in, sr_out, n):
    """Windows over one signal: its start, its end with L_total given, the interior (open, and closed), one output.  Each
    from the smallest window that holds what its outputs read; one sample fewer at either end is refused and writes
    nothing."""
    up, down = rational(sr_in, sr_out)
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
    whole = resample(x[None], sr_in, sr_out)[0]
    n_out = whole.numel()
    assert n_out == out_len(n, up, down)
    a = min(1500, n_out // 3)
    mid = n_out // 2
    ranges = [(0, a, False), (0, a, True), (n_out - a, n_out, True), (mid - a // 2, mid + a, False), (mid - a // 2, mid + a, True),
              (mid + 1, mid + 2, False), (n_out - 1, n_out, True), (0, n_out, True)]
    done = 0
    for n0, n1, closed in ranges:
        lo, hi = _samples_read(n0, n1, up, down, n if closed else None)
        if hi > n:                                                  # open, and the outputs reach past what exists
            continue
        out = torch.full((n1 - n0,), 7.0, device="cuda")
        Lt = n if closed else -1
        for win, m0 in ((x[lo + 1:hi], lo + 1), (x[lo:hi - 1], lo)):
            assert _window(win.clone(), m0, Lt, up, down, out, n0) == ERR_SHAPE, (n0, n1, closed, lo, hi, m0)
            assert b"flowse_resample_poly_window" in L.flowse_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
        _lib.check(_window(x[lo:hi].clone(), lo, Lt, up, down, out, n0))
        torch.cuda.synchronize()
        assert torch.equal(out, whole[n0:n1]), (n0, n1, closed, int((out != whole[n0:n1]).sum()))
        done += 1
    assert done >= 6 and float(whole.abs().max()) > 0
    # a larger window gives the same outputs; an unreduced pair is the reduced one; no outputs, no launch
    out = torch.full((a,), 7.0, device="cuda")
    _lib.check(_window(x, 0, n, 3 * up, 3 * down, out, mid))
    assert torch.equal(out, whole[mid:mid + a])
    out.fill_(7.0)
    s, p = _lib.current_stream(), _lib.ptr
    assert L.flowse_resample_poly_window(p(x), 0, n, n, up, down, p(out), n_out, 0, s) == 0
    assert L.flowse_resample_poly_window(p(x), 0, n, -1, up, down, p(out), 10 ** 9, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_window_entry_at_equal_rates_copies_the_slice():
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1)).cuda()
    out = torch.full((100,), 7.0, device="cuda")
    _lib.check(_window(x[200:700].clone(), 2 ** 40 + 200, -1, 48000, 48000, out, 2 ** 40 + 250))
    torch.cuda.synchronize()
    assert torch.equal(out, x[250:350])
    out.fill_(7.0)
    assert _window(x[200:700].clone(), 200, 1000, 5, 5, out, 601) == ERR_SHAPE      # [601, 701) passes the window's end
    assert _window(x[200:700].clone(), 200, 650, 5, 5, out, 300) == ERR_SHAPE       # the window passes the signal's end
    assert L.flowse_resample_poly_window(None, 0, 10, -1, 1, 3, _lib.ptr(out), 0, 1, _lib.current_stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 2
FAR_CASES = [(44100, 16000, 4_869_000),            # c = half + n down passes 2^31 inside the range
             (44100, 16000, 2 ** 33 + 7),          # n down near 2^42, m0 past 2^34
             (16000, 48000, 3 * 2 ** 31 + 1011),   # an upsampler: n and m0 past 2^31
             (16000, 44100, 2 ** 34 + 5)]


@pytest.mark.parametrize("sr_in,sr_out,n0", FAR_CASES, ids=lambda v: str(v))
def test_far_outputs_from_a_slice(sr_in, sr_out, n0):
    """3000 outputs far into an open signal from the slice they read, against float64 under (P + 2) 2^-24 S[n]."""
    up, down = rational(sr_in, sr_out)
    half, P = _geometry(up, down)
    n1 = n0 + 3000
    lo, hi = _samples_read(n0, n1, up, down, None)
    assert (n1 - 1) * down > 2 ** 31 and lo == (half + n0 * down) // up - (P - 1)
    if n0 > 2 ** 31:
        assert lo > 2 ** 31
    else:
        assert half + n0 * down < 2 ** 31 < half + (n1 - 1) * down
    xs = torch.randn(hi - lo, generator=torch.Generator().manual_seed(n0 % 1000))
    out = torch.full((n1 - n0,), 7.0, device="cuda")
    _lib.check(_window(xs.cuda(), lo, -1, up, down, out, n0))
    torch.cuda.synchronize()
    x64 = xs.numpy().astype(np.float64)
    ref = resample_reference(x64, sr_in, sr_out, n0, n1, m0=lo)
    h = np.zeros(up * P)
    h[:2 * half + 1] = np.abs(design_taps(up, down))
    H = h.reshape(P, up).T                                          # |H[p][j]| = |h[p + j up]|
    c = half + np.arange(n0, n1, dtype=np.int64) * down
    m = (c // up)[:, None] - np.arange(P)[None, :] - lo
    assert m.min() == 0 and m.max() == x64.shape[0] - 1
    bound = (P + 2) * U * np.einsum("ij,ij->i", H[c % up], np.abs(x64)[m])
    d = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print(f"{sr_in} -> {sr_out}, outputs [{n0}, {n1}): max |kernel - float64| / bound = {(d / bound).max():.3f}")
    assert (bound > 0).all() and np.abs(ref).max() > 0.5
    bad = np.nonzero(d > bound)[0]
    assert bad.size == 0, (bad[:5], d[bad[:5]], bound[bad[:5]])
    # the same outputs with the window one sample short at either end: refused, with the numbers
    assert _window(xs[1:].cuda(), lo + 1, -1, up, down, out, n0) == ERR_SHAPE and str(lo).encode() in L.flowse_last_error()
    assert _window(xs[:-1].cuda(), lo, -1, up, down, out, n0) == ERR_SHAPE and str(hi - 1).encode() in L.flowse_last_error()


# ---------------------------------------------------------------------------------------------------- 3
def _patterns(n, seed, block=2048):
    """Push sizes that sum to n: all at once; single samples (n <= 2000 only); blocks; seeded random sizes with zeros."""
    rng = np.random.default_rng(seed)
    rand, done = [0], 0
    while done < n:
        s = min(int(rng.choice([0, 1, 2, 17, 300, 1000, 5000])), n - done)
        rand.append(s)
        done += s
    rand.append(0)
    pats = {"whole": [n], "blocks": [min(block, n - i) for i in range(0, n, block)], "random": rand}
    if n <= 2000:
        pats["ones"] = [1] * n
    return pats


def _as_input(chunk, how):
    return (chunk.numpy(), chunk[None], chunk.cuda())[how % 3]


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000), (8000, 16000)],
                         ids=lambda v: str(v))
def test_stream_resampler_is_resample_bit_for_bit(sr_in, sr_out):
    up, down = rational(sr_in, sr_out)
    rs = StreamResampler(sr_in, sr_out, device="cuda")
    for n in (1, 9, 1500, 40001):                                   # 9 < P for every ratio here
        x = torch.randn(n, generator=torch.Generator().manual_seed(n + sr_in))
        want = resample(x[None].cuda(), sr_in, sr_out)[0]
        for how, (name, sizes) in enumerate(_patterns(n, n + sr_out).items()):
            parts, done = [], 0
            for i, s in enumerate(sizes):
                parts.append(rs.push(_as_input(x[done:done + s], how + i), as_tensor=True))
                done += s
                assert (rs.samples_in, rs.samples_out) == (done, stream_plan(done, up, down))
            parts.append(rs.finish(as_tensor=True))
            assert all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 1 for p in parts)
            got = torch.cat(parts)
            assert rs.samples_out == got.numel() == out_len(n, up, down)
            assert torch.equal(got, want), (n, name, int((got != want).sum()))
            rs.reset()
        assert float(want.abs().max()) > 0
    # numpy out by default, the same values
    assert np.array_equal(np.concatenate([rs.push(x[:20000].numpy()), rs.push(x[20000:].numpy()), rs.finish()]),
                          want.cpu().numpy())
    # the device follows the first push when none is named
    free = StreamResampler(sr_in, sr_out)
    assert torch.equal(torch.cat([free.push(x.cuda(), as_tensor=True), free.finish(as_tensor=True)]), want)


def test_stream_resampler_state_is_bounded():
    """60 blocks of 2048 at 44.1 -> 16 kHz: after block 4 and after block 59 the object reports the same state and the
    allocator holds no more."""
    x = torch.randn(60 * 2048, generator=torch.Generator().manual_seed(3)).cuda()
    rs = StreamResampler(44100, 16000, device="cuda")
    seen = {}
    for i in range(60):
        out = rs.push(x[2048 * i:2048 * (i + 1)], as_tensor=True)
        del out
        if i in (4, 59):
            seen[i] = (rs.state_bytes(), torch.cuda.memory_allocated())
    print(f"stream resampler state after block 4: {seen[4]}, after block 59: {seen[59]}")
    assert seen[4] == seen[59] and 0 < seen[4][0] <= 4 * (2048 + 56 + 3)     # a block, and P - 1 + ceil(down / up) kept


# ---------------------------------------------------------------------------------------------------- 4
@pytest.fixture(scope="module")
def model():
    from flowmse_amd.evaluate import _load_model
    assert torch.cuda.is_available()
    return _load_model(types.SimpleNamespace(synthetic=1, ckpt=None, test_dir="stdin", precision="fp32"), None)[0]


GEOMETRY = dict(chunk_frames=64, overlap_frames=16)
SOLVER = dict(N=2, T_rev=0.9, t_eps=0.04, odesolver="euler")
# 16 kHz lengths: one chunk (T <= 64 frames), two chunks (T <= 112), about 3 s
RECORDINGS = {48000: [15001, 36002, 144001], 44100: [13801, 33077, 132297]}


def _signal(seed, n, std=0.1):
    return torch.from_numpy(synth.normal(seed, 9, (1, n), std))


def _run_live(live, y, sizes):
    parts, done = [], 0
    for i, s in enumerate(sizes):
        parts.append(live.push(_as_input(y[done:done + s], i)))
        done += s
        assert live.samples_in == done and (live.output_rate != "input" or live.samples_out <= done)
    parts.append(live.finish())
    assert all(p.dtype == np.float32 and p.ndim == 1 for p in parts)
    return np.concatenate(parts)


def _reference(model, y, rate, mode):
    from flowmse_amd.enhance import enhance_recording
    want, sr, _ = enhance_recording(model, y.cuda(), rate, mode, batch=1, noise_key=KEY, noise_seed=SEED, **GEOMETRY, **SOLVER)
    assert sr == (rate if mode == "input" else 16000)
    return want


@pytest.mark.parametrize("mode", ["16000", "input"])
@pytest.mark.parametrize("rate,which", [(r, i) for r in RECORDINGS for i in range(3)], ids=lambda v: str(v))
def test_live_at_other_rates_is_enhance_recording_bit_for_bit(model, rate, which, mode):
    """The contract: concat(push..., finish) == enhance_recording(batch=1, same key and seed) when norm = max|y16|."""
    n = RECORDINGS[rate][which]
    y = _signal(n % 97, n)
    want = _reference(model, y, rate, mode)
    norm = resample(y.cuda(), rate, 16000).abs().max().item()
    live = LiveEnhancer(model, norm=norm, key=KEY, seed=SEED, input_rate=rate, output_rate=mode, **GEOMETRY, **SOLVER)
    assert live.latency_samples == latency_samples(64, rate, mode, 16) > 128 * 64 + 382
    pats = _patterns(n, n, block=2048 * rate // 16000)
    for name in ("whole", "blocks", "random"):
        got = _run_live(live, y[0], pats[name])
        assert live.samples_in == n and live.samples_out == got.shape[0] == want.shape[0]
        assert got.shape[0] == (n if mode == "input" else out_len(n, *rational(rate, 16000)))
        assert np.array_equal(got, want), (name, int((got != want).sum()), int(np.flatnonzero(got != want)[0]))
        live.reset()
        assert (live.samples_in, live.samples_out) == (0, 0)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0


def test_live_at_another_rate_in_a_16_bit_precision(model):
    rate, n = 48000, 36002
    y = _signal(11, n)
    model.dnn.set_precision("bf16")
    try:
        want = _reference(model, y, rate, "input")
        norm = resample(y.cuda(), rate, 16000).abs().max().item()
        live = LiveEnhancer(model, norm=norm, key=KEY, seed=SEED, input_rate=rate, output_rate="input", **GEOMETRY, **SOLVER)
        assert np.array_equal(_run_live(live, y[0], _patterns(n, 5, block=6144)["blocks"]), want)
    finally:
        model.dnn.set_precision("fp32")
    assert not np.array_equal(want, _reference(model, y, rate, "input"))


def test_norm_first_and_the_default_rate(model):
    """``norm="first"`` is the peak of the 16 kHz samples [0, n_0) whatever the push sizes; the object without the new
    arguments, and with them at their defaults' meaning, returns what ``enhance_long(batch=1)`` returns."""
    from flowmse_amd.chunked import enhance_long
    rate, n = 44100, 60000
    y = _signal(13, n)
    y[0, 50000] = 3.0                                               # a later peak that "first" never sees
    n_0 = 128 * 63 + 255
    y16 = resample(y.cuda(), rate, 16000)
    kw = dict(key=KEY, seed=SEED, **GEOMETRY, **SOLVER)
    live = LiveEnhancer(model, norm="first", input_rate=rate, output_rate="input", **kw)
    pats = _patterns(n, 1, block=5000)
    a = _run_live(live, y[0], pats["blocks"])
    assert live.norm == y16[0, :n_0].abs().max().item() < 1.0
    live.reset()
    assert live.norm is None
    b = _run_live(live, y[0], pats["random"])
    assert np.array_equal(a, b) and a.shape == (n,)
    fixed = LiveEnhancer(model, norm=y16[0, :n_0].abs().max().item(), input_rate=rate, output_rate="input", **kw)
    assert np.array_equal(_run_live(fixed, y[0], [n]), a)
    # 16 kHz: nothing moved
    z = _signal(17, 30000)
    want = enhance_long(model, z.cuda(), 64, 16, batch=1, noise_key=KEY, noise_seed=SEED, **SOLVER)
    for extra in ({}, dict(input_rate=16000, output_rate="input")):
        plain = LiveEnhancer(model, norm=z.abs().max().item(), **kw, **extra)
        assert plain._rs_in is None and plain._rs_out is None and plain.latency_samples == 128 * 64 + 382
        assert np.array_equal(_run_live(plain, z[0], _patterns(30000, 2)["blocks"]), want)
        assert plain.samples_in == plain.samples_out == 30000
    # a recording too short for the STFT is refused at the 16 kHz count, and the object can go on
    live.reset()
    live.push(np.zeros(600, dtype=np.float32))                      # 218 samples at 16 kHz
    with pytest.raises(ValueError, match="255"):
        live.finish()


# ---------------------------------------------------------------------------------------------------- 5
def test_live_rate_cli_in_a_child_process(model):
    """1.5 s of 48 kHz s16le through ``enhance --live --live_rate 48000 --output_rate input``: as many bytes come back, the
    bytes of an in-process ``LiveEnhancer`` with the same settings through the same quantiser."""
    n = 72000
    t = np.arange(n) / 48000.0
    x = 0.3 * np.sin(2 * np.pi * 220 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.05 * synth.normal(23, 9, (n,), 1.0)
    raw = pcm_encode(x.astype(np.float32), "s16le")
    args = ["--live", "--live_rate", "48000", "--output_rate", "input", "--synthetic", "1", "--seed", "3", "--live_block", "3000",
            "--chunk_frames", "64", "--overlap_frames", "16", "--live_norm", "0.5", "--N", "2"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "flowmse_amd.enhance"] + args, cwd=ROOT, input=raw,
                       capture_output=True)
    assert r.returncode == 0, f"exited with {r.returncode}:\n{r.stderr.decode(errors='replace')[-3000:]}"
    assert len(r.stdout) == 2 * n and b"live: enhanced 72000 samples" in r.stderr and b"48000 Hz in, 48000 Hz out" in r.stderr
    live = LiveEnhancer(model, norm=0.5, key=utterance_key("live"), seed=3, chunk_frames=64, overlap_frames=16, N=2,
                        input_rate=48000, output_rate="input")
    want = b"".join(pcm_encode(live.push(pcm_decode(raw[i:i + 5000], "s16le")), "s16le") for i in range(0, len(raw), 5000))
    want += pcm_encode(live.finish(), "s16le")
    assert r.stdout == want
    assert np.abs(np.frombuffer(want, dtype="<i2")).max() > 0
