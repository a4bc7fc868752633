"""GPU: the polyphase resampler (csrc/resample.hip) -- the kernel against float64 scipy under a derived per-sample bound,
the far end of a 14 M-sample signal (``n down`` past 2^31), row independence and repeatability, the C call's argument checks,
and ``enhance --resample`` end to end: in process against the same steps around a float64 CPU resampler, then as child
processes, one after the other, each under its own time limit.  No test asserts a time.

The bound.  An output is a P-term fp32 fmaf chain of fp32-rounded taps times fp32 samples: with u = 2^-24 every product
carries (1 + u) from its tap and the chain at most (1 + u)^P more, so |out[n] - ref[n]| <= (P + 2) u S[n] to first order,
S[n] = sum |h| |x| over the terms of out[n].  S comes from scipy.signal.resample_poly(|x|, up, down, window=|firwin taps|)
(scipy multiplies an array window by ``up`` itself).  An fp32 restatement of the sum on the CPU stays below 0.2 of the
bound; an indexing error is a wrong sample of order |x|, thousands of times the bound.
"""
import filecmp
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from flowmse_amd import _lib
from flowmse_amd.resample import out_len, rational, resample, resample_reference

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
U = 2.0 ** -24
RATE_CASES = [(48000, 16000, 1000), (44100, 16000, 1327), (22050, 16000, 700), (8000, 16000, 333), (16000, 48000, 257),
              (16000, 44100, 320)]
# ratios at which the launch takes its other forms (csrc/resample.hip): a run of 256 outputs instead of 1024 (192 kHz),
# the table read through L2 (1023/1024: 21483 entries), the input read from global memory with the table in LDS (1/24:
# a run's span exceeds the staging buffer) and both from global memory (1/1024); lengths that give more than one block
PATH_CASES = [(192000, 16000, 20000), (16384, 16368, 3000), (384000, 16000, 30000), (1024000, 1000, 300000)]


def _taps_P(up, down):
    from scipy.signal import firwin
    R = max(up, down)
    return firwin(20 * R + 1, 1.0 / R, window=("kaiser", 5.0)), -(-(20 * R + 1) // up)


def _bound(x64, up, down):
    """(P + 2) 2^-24 S[n] for every output of the float64 signal ``x64`` (module docstring)."""
    from scipy.signal import resample_poly
    taps, P = _taps_P(up, down)
    return (P + 2) * U * resample_poly(np.abs(x64), up, down, window=np.abs(taps))


def _signal(seed, B, n):
    return torch.randn(B, n, generator=torch.Generator().manual_seed(seed))


def _check_rows(sr_in, sr_out, sig):
    """Every sample of every row of the kernel's output against float64 scipy, under the bound; returns the largest
    |difference| / bound."""
    from scipy.signal import resample_poly
    up, down = rational(sr_in, sr_out)
    got = resample(sig.cuda(), sr_in, sr_out)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (sig.size(0), out_len(sig.size(1), up, down))
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    worst = 0.0
    for b in range(sig.size(0)):
        x = sig[b].numpy().astype(np.float64)
        ref, bound = resample_poly(x, up, down), _bound(x, up, down)
        d = np.abs(got[b] - ref)
        assert bound.shape == d.shape and (bound > 0).all()
        worst = max(worst, float((d / bound).max()))
        bad = np.nonzero(d > bound)[0]
        assert bad.size == 0, (sr_in, sr_out, b, bad[:5], d[bad[:5]], bound[bad[:5]])
    return worst


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("sr_in,sr_out,n", RATE_CASES, ids=lambda v: str(v))
def test_kernel_matches_float64_scipy(sr_in, sr_out, n):
    """B = 3 rows of different content at the case's length, at 5 samples and at 1 (every tap hangs over an edge)."""
    for length in (n, 5, 1):
        w = _check_rows(sr_in, sr_out, _signal(sr_in + length, 3, length))
        print(f"{sr_in} -> {sr_out}, [3, {length}]: max |kernel - float64| / bound = {w:.3f}")


@pytest.mark.parametrize("sr_in,sr_out,n", PATH_CASES, ids=lambda v: str(v))
def test_kernel_forms_for_large_ratios(sr_in, sr_out, n):
    w = _check_rows(sr_in, sr_out, _signal(n, 2, n))
    print(f"{sr_in} -> {sr_out}, [2, {n}]: max |kernel - float64| / bound = {w:.3f}")


# ---------------------------------------------------------------------------------------------------- 2
def test_far_end_of_a_long_signal():
    """44100 -> 16000 on 14 000 000 samples generated on the device (56 MB): c = half + n down passes 2^31 at output
    4 869 568.  The last 4096 outputs and 4096 straddling output 4 869 000 against ``resample_reference`` on the input
    slice they touch, copied back; a slice starts on a multiple of 441 samples = 160 outputs, so that scipy's S of the
    slice lines up with the signal's (one 441-sample block of margin covers the P - 1 = 55 samples an output reaches back)."""
    n, (up, down) = 14_000_000, rational(44100, 16000)
    x = torch.randn(1, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(14))
    got = resample(x, 44100, 16000)
    torch.cuda.synchronize()
    n_out = out_len(n, up, down)
    assert got.shape == (1, n_out) and n_out == 5_079_366 and (n_out - 1) * down > 2 ** 31
    half, P = 10 * down, _taps_P(up, down)[1]
    for n0, n1 in ((4_869_000 - 2048, 4_869_000 + 2048), (n_out - 4096, n_out)):
        q_lo, q_hi = (half + n0 * down) // up - (P - 1), (half + (n1 - 1) * down) // up
        blk = q_lo // down - 1                                     # the slice starts at sample blk * 441 = output blk * 160
        m0, m1 = blk * down, min(q_hi + 1, n)
        assert 0 < m0 <= q_lo - (P - 1) and blk * up < n0                 # S of output n0 has all its terms inside the slice
        xs = x[0, m0:m1].cpu().numpy().astype(np.float64)
        ref = resample_reference(xs, 44100, 16000, n0, n1, m0=m0)
        bound = _bound(xs, up, down)[n0 - blk * up:n1 - blk * up]
        d = np.abs(got[0, n0:n1].cpu().numpy().astype(np.float64) - ref)
        assert d.shape == bound.shape == (4096,) and (bound > 0).all()
        print(f"outputs [{n0}, {n1}): max |kernel - float64| / bound = {(d / bound).max():.3f}, max |ref| = {np.abs(ref).max():.3f}")
        bad = np.nonzero(d > bound)[0]
        assert bad.size == 0, (n0, bad[:5], d[bad[:5]], bound[bad[:5]])
        assert np.abs(ref).max() > 0.5                             # a real signal there, not the zeros past an edge
    assert (half + (4_869_000 - 2048) * down) < 2 ** 31 < (half + (4_869_000 + 2048) * down)


# ---------------------------------------------------------------------------------------------------- 3
def test_rows_are_independent_and_calls_repeat():
    sig = _signal(3, 3, 5000).cuda()
    for sr_in, sr_out in ((44100, 16000), (16000, 44100), (48000, 16000)):
        a = resample(sig, sr_in, sr_out)
        one = resample(sig[1:2].contiguous(), sr_in, sr_out)
        b = resample(sig, sr_in, sr_out)
        torch.cuda.synchronize()
        assert torch.equal(a[1], one[0]) and torch.equal(a, b)
        assert not torch.equal(a[0], a[1])
    assert resample(sig, 16000, 16000) is sig
    # up == down through the C entry is a device copy (the pair is reduced first)
    out = torch.zeros_like(sig)
    _lib.check(L.flowse_resample_poly(_lib.ptr(sig), 3, 5000, 48000, 48000, _lib.ptr(out), 5000, _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, sig)


# ---------------------------------------------------------------------------------------------------- 4
def test_bad_arguments_return_a_status_and_launch_nothing():
    sig = _signal(4, 2, 1000).cuda()
    out = torch.full((2, 400), 7.0, device="cuda")
    s, p = _lib.current_stream(), _lib.ptr
    assert out_len(1000, 1, 3) == 334
    for L_out in (333, 335, 0, -1):
        assert L.flowse_resample_poly(p(sig), 2, 1000, 1, 3, p(out), L_out, s) == ERR_SHAPE, L_out
        assert b"flowse_resample_poly" in L.flowse_last_error() and b"334" in L.flowse_last_error()
    assert L.flowse_resample_poly(p(sig), 2, 1000, 1, 1025, p(out), 1, s) == ERR_SHAPE           # R > 1024
    assert L.flowse_resample_poly(p(sig), 2, 1000, 16000, 16001, p(out), 1000, s) == ERR_SHAPE
    assert b"1024" in L.flowse_last_error()
    assert L.flowse_resample_poly(p(sig), 65536, 1000, 1, 3, p(out), 334, s) == ERR_SHAPE         # right L_out, too many rows
    assert b"65535 rows" in L.flowse_last_error()
    assert L.flowse_resample_poly(p(sig), 2, 1000, 0, 3, p(out), 334, s) == ERR_ARG
    assert L.flowse_resample_poly(None, 2, 1000, 1, 3, p(out), 334, s) == ERR_ARG
    assert L.flowse_resample_poly(p(sig), 2, 1000, 1, 3, None, 334, s) == ERR_ARG
    assert L.flowse_resample_poly(p(sig), 0, 1000, 1, 3, p(out), 334, s) == ERR_ARG
    with pytest.raises(ValueError):
        resample(sig, 16001, 16000)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _lib.check(L.flowse_resample_poly(p(sig), 2, 1000, 1, 3, p(out), 334, s))                     # rows of 334 in the buffer
    torch.cuda.synchronize()
    assert not bool((out.reshape(-1)[:668] == 7.0).any()) and bool((out.reshape(-1)[668:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 5
# End to end, measured on an MI355X (gfx950), full net, synthetic weights, N = 1, one second of 44.1 kHz synthetic signal,
# keyed noise of "synthetic_00.wav" under seed 3.  GPU resampler against the float64 CPU resampler (rounded to fp32) around
# the same GPU enhance_long, relative to the largest sample of the reference:
#   16 kHz input of the network:  max |difference| = E2E_IN_MEASURED x max|y16|   (what the resampler bound above allows)
#   written 44.1 kHz waveform:    max |difference| = E2E_MEASURED x max|x_hat|
# Their quotient is the sensitivity of the sampler to its input on these weights.  Asserted: 4 x each
# measured figure, the convention of tests/test_gpu_keyed_noise.py; a wrong phase or an off-by-one sample in either
# direction is a difference of order 1e-1.
# Measured: 4.825e-07 at the network's input, 1.102e-06 in the written waveform (max |x_hat| = 1.298), a sensitivity of
# 2.28: the one-step sampler roughly doubles a relative input error of the order of fp32 rounding and no more.
E2E_IN_MEASURED = 4.825e-07
E2E_MEASURED = 1.102e-06
E2E_BOUND = 4 * E2E_MEASURED
CLI = ["--synthetic", "1", "--synthetic_seconds", "1", "--resample", "--N", "1", "--seed", "3"]


def _enhance(out, extra, limit=400):
    return subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "flowmse_amd.enhance", "--output", str(out)]
                          + CLI + extra, cwd=ROOT, capture_output=True, text=True)


@pytest.mark.timeout(1200)
def test_enhance_resample_end_to_end(tmp_path):
    """In process against the float64-resampler composition, then the command in two child processes.  The bound is
    4 x the figure measured once on an MI355X (E2E_MEASURED, the comment above); the test prints what it measures."""
    from scipy.io import wavfile
    from flowmse_amd.chunked import enhance_long
    from flowmse_amd.enhance import enhance_recording
    from flowmse_amd.evaluate import _load_model, _synthetic_pairs, _write_wav
    from flowmse_amd.util.noise import utterance_key
    assert torch.cuda.is_available()
    model, _ = _load_model(types.SimpleNamespace(synthetic=1, ckpt=None, test_dir=None, precision="fp32"), None)
    name, _, noisy = _synthetic_pairs(1, seconds=[1.0], sr=44100)[0]
    y = torch.from_numpy(noisy)[None]
    assert name == "synthetic_00.wav" and y.shape == (1, 44100)
    kw = dict(chunk_frames=256, overlap_frames=32, batch=8, N=1, T_rev=1.0, t_eps=0.03, odesolver="euler",
              noise_key=utterance_key(name), noise_seed=3)
    got, sr, frames = enhance_recording(model, y.cuda(), 44100, "input", **kw)
    assert sr == 44100 and frames == 126 and got.shape == (44100,) and got.dtype == np.float32 and np.isfinite(got).all()
    # the same steps with the float64 CPU resampler (rounded to fp32) around the unchanged GPU enhance_long
    y16 = resample(y, 44100, 16000)
    assert y16.shape == (1, 16000) and not y16.is_cuda
    x16 = enhance_long(model, y16.cuda(), as_tensor=True, **kw)
    want = resample(x16.cpu()[None], 16000, 44100)[0, :44100].numpy()
    y16_gpu = resample(y.cuda(), 44100, 16000).cpu()
    e_in = float((y16_gpu - y16).abs().max() / y16.abs().max())
    e_out = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
    print(f"enhance --resample 44.1 kHz: 16 kHz input max |gpu - float64| / max = {e_in:.3e}, written waveform "
          f"{e_out:.3e}, sensitivity {e_out / max(e_in, 1e-30):.2f}, max |x_hat| = {np.abs(want).max():.3f}")
    assert e_in <= 4 * E2E_IN_MEASURED, (e_in, 4 * E2E_IN_MEASURED)
    assert e_out <= E2E_BOUND, (e_out, E2E_BOUND)
    # at 16 kHz output the composition is the resampler and enhance_long, nothing after
    x16k, sr16, _ = enhance_recording(model, y.cuda(), 44100, "16000", **kw)
    assert sr16 == 16000 and x16k.shape == (16000,)
    assert x16k.tobytes() == enhance_long(model, resample(y.cuda(), 44100, 16000), **kw).tobytes()

    # the command, in child processes one after the other; the second only if the first exited 0
    r = _enhance(tmp_path / "a", ["--synthetic_rate", "44100", "--output_rate", "input"])
    assert r.returncode == 0, f"exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    sr, data = wavfile.read(tmp_path / "a" / name)
    assert sr == 44100 and data.shape == (44100,) and data.dtype == np.int16 and np.abs(data).max() > 0
    _write_wav(str(tmp_path / "want.wav"), got, 44100)
    assert filecmp.cmp(tmp_path / "a" / name, tmp_path / "want.wav", shallow=False)
    settings = (tmp_path / "a" / "_settings.txt").read_text()
    assert "resample: True\noutput_rate: input\nresampled synthetic_00.wav: 44100 Hz\n" in settings
    assert "(126 frames)" in r.stdout
    r = _enhance(tmp_path / "b", ["--synthetic_rate", "44100", "--output_rate", "16000"])
    assert r.returncode == 0, f"exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    sr, data = wavfile.read(tmp_path / "b" / name)
    assert sr == 16000 and data.shape == (16000,) and data.dtype == np.int16 and np.abs(data).max() > 0
    _write_wav(str(tmp_path / "want16.wav"), x16k, 16000)
    assert filecmp.cmp(tmp_path / "b" / name, tmp_path / "want16.wav", shallow=False)
