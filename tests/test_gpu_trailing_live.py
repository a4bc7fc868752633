"""GPU, end to end: trailing chunks.  ``enhance_trailing`` against the oracle composition; ``LiveEnhancer(hop_frames=...)``
against ``enhance_trailing(batch=1)`` bit for bit under every push pattern, in fp32 and bf16, with the counts ``live_plan``
predicts and a state that does not grow; one 48 kHz stream against the file-mode composition; and the object without the new
keywords, which makes the calls and returns the bytes it always did.  Tc = 64 everywhere; no test asserts a time."""
import numpy as np
import pytest
import torch

import _cases as C
from flowmse_amd import _lib
from flowmse_amd.chunked import enhance_long, enhance_trailing, plan_trailing
from flowmse_amd.live import LiveEnhancer, latency_samples, live_plan
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
KEY, SEED = 0x912975D344AF26C6, 0x1F2E3D4C5B6A7988
TC = 64
SOLVER = dict(N=2, T_rev=0.9, t_eps=0.04, odesolver="euler")


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


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.timeout(900)
def test_enhance_trailing_vs_oracle_composition(full):
    """Full net, synthetic weights, 20000 samples as ten trailing chunks of 64 frames at (H, X) = (16, 4), N = 2, explicit
    global z [1,1,256,208]: the HIP path against the oracle field per chunk driven through the same host code and the float64
    blend on the CPU.  Bound: 1e-3 waveform rel-L2, that of test_enhance_long_vs_oracle_composition.  Measured on an MI355X:
    5.1e-7."""
    from oracle import ncsnpp_oracle as O
    tb = C.param_tables()["full"]
    w = C.synth_weights(tb["names"], tb["shapes"])
    sig = _signal(3, 20000)
    K, P, Tg = plan_trailing(20000 // 128 + 1, TC, 16, 4)
    assert (K, P, Tg) == (10, 48, 160)
    z = C.c64(synth.synth_noise(2, 1, 256, P + Tg))
    kw = dict(chunk_frames=TC, hop_frames=16, fade_frames=4, N=2)
    ref = enhance_trailing(full, sig, z=z, VF_fn=lambda x, t, y: O.vf_forward(w, O.make_cfg(), x, t, y), device="cpu", **kw)
    got = enhance_trailing(full, sig.cuda(), z=z.cuda(), **kw)
    err = _rel(got, ref)
    print("trailing end-to-end waveform rel-L2 vs oracle composition", err)
    assert got.shape == ref.shape == (20000,) and np.isfinite(got).all() and float(np.abs(ref).max()) > 0
    assert err < 1e-3
    with pytest.raises(ValueError, match="P \\+ Tg"):
        enhance_trailing(full, sig.cuda(), z=z[..., :Tg].cuda(), **kw)


# ---------------------------------------------------------------------------------------------------- 2
def _patterns(n, H):
    """Push sizes that sum to n: one sample short of each n_k, then that sample; blocks of 2048; all at once; ragged primes."""
    def blocks(sizes):
        out, done, i = [], 0, 0
        while done < n:
            s = min(sizes[i % len(sizes)], n - done)
            out.append(s)
            done += s
            i += 1
        return out
    short, done, k = [], 0, 0
    while True:
        n_k = 128 * (k * H + H - 1) + 255
        if n_k > n:
            break
        short += [n_k - 1 - done, 1]
        done, k = n_k, k + 1
    short.append(n - done)
    assert sum(short) == n and min(short) >= 0
    return {"short": short, "2048": blocks([2048]), "whole": [n], "primes": blocks([997, 1, 4099, 13, 2, 251, 7919, 3])}


def _run_live(live, y, sizes, check=None):
    parts, done = [], 0
    for s in sizes:
        parts.append(live.push(y[done:done + s].numpy()))
        done += s
        if check:
            check(live, sum(p.shape[0] for p in parts))
    parts.append(live.finish())
    assert all(p.dtype == np.float32 and p.ndim == 1 for p in parts)
    return np.concatenate(parts)


@pytest.mark.parametrize("H,X", [(16, 4), (8, 8), (4, 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("Ls", [300, 128 * 16 * 4, 20000, 33333])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_live_is_enhance_trailing_bit_for_bit(full, precision, Ls, H, X):
    """The contract: concat(push..., finish) == enhance_trailing(batch=1, same key and seed, norm = max|y|) for every push
    pattern, every push returning exactly the count ``live_plan`` predicts.  300 samples: one right-aligned chunk, sampled by
    finish(); 8192: T = 65 = 4 H + 1 at H = 16, a last chunk of one real frame; (8, 8) and (4, 2) keep two previous chunks."""
    sig = _signal(Ls % 89 + H, Ls)
    geo = dict(chunk_frames=TC, hop_frames=H, fade_frames=X)
    full.dnn.set_precision(precision)
    try:
        want = enhance_trailing(full, sig.cuda(), batch=1, noise_key=KEY, noise_seed=SEED, **geo, **SOLVER)
        live = LiveEnhancer(full, norm=sig.abs().max().item(), key=KEY, seed=SEED, **geo, **SOLVER)
        assert live.latency_samples == 128 * (H + X) + 382 == latency_samples(TC, hop_frames=H, fade_frames=X)

        def counters(lv, returned):
            assert lv.samples_out == returned == live_plan(lv.samples_in, TC, hop_frames=H, fade_frames=X)[1]

        for name, sizes in _patterns(Ls, H).items():
            got = _run_live(live, sig[0], sizes, check=counters)
            assert live.samples_in == live.samples_out == Ls == got.shape[0]
            assert live._k == live_plan(Ls, TC, finished=True, hop_frames=H, fade_frames=X)[0]
            assert np.array_equal(got, want), (name, int((got != want).sum()), int(np.flatnonzero(got != want)[0]))
            live.reset()
        assert want.shape == (Ls,) and np.isfinite(want).all() and float(np.abs(want).max()) > 0
        if Ls == 20000 and (H, X) == (16, 4):                   # another seed is another recording; so is the other geometry
            other = enhance_trailing(full, sig.cuda(), batch=1, noise_key=KEY, noise_seed=SEED + 1, **geo, **SOLVER)
            assert not np.array_equal(other, want)
            assert not np.array_equal(enhance_long(full, sig.cuda(), TC, 16, batch=1, noise_key=KEY, noise_seed=SEED, **SOLVER), want)
    finally:
        full.dnn.set_precision("fp32")


def test_state_is_bounded(full):
    """32 chunks' worth in blocks of 2048 at (16, 4), N = 1: after chunk 3 and after chunk 30 the object reports the same
    state and the allocator holds no more."""
    H, X = 16, 4
    n = 128 * (31 * H + H - 1) + 255 + 100
    sig = _signal(17, n)
    live = LiveEnhancer(full, norm=0.5, key=KEY, seed=SEED, chunk_frames=TC, hop_frames=H, fade_frames=X, N=1)
    seen, done = {}, 0
    while done < n:
        out = live.push(sig[0, done:done + 2048].numpy())
        done += min(2048, n - done)
        ready = live_plan(live.samples_in, TC, hop_frames=H, fade_frames=X)[0]
        for mark in (4, 31):
            if ready >= mark and mark not in seen:
                out = None                                      # the returned samples are the caller's, not state
                seen[mark] = (live.state_bytes(), torch.cuda.memory_allocated())
    assert set(seen) == {4, 31}
    print(f"trailing live state after chunk 3: {seen[4]}, after chunk 30: {seen[31]}")
    assert seen[4][0] == seen[31][0] > 0 and seen[31][1] <= seen[4][1]
    assert seen[4][0] < 4 * (128 * TC + 382 + 2 * 2048) + 2 * 8 * 256 * TC      # buffer of a window and a block, one chunk
    tail = live.finish()
    assert live.samples_out == n and np.isfinite(tail).all()
    two = LiveEnhancer(full, norm=0.5, key=KEY, chunk_frames=TC, hop_frames=8, fade_frames=8, N=1)
    two.push(sig[0, :128 * (3 * 8 - 1) + 255].numpy())
    assert two.state_bytes() >= 2 * 8 * 256 * TC                                # the geometry that keeps two chunks says so


# ---------------------------------------------------------------------------------------------------- 3
def test_live_at_48_khz_is_the_file_mode_composition(full):
    """48 kHz in and out at (16, 4): resample -> enhance_trailing(batch=1) -> resample back, bit for bit, when norm is the peak
    of the resampled recording."""
    from flowmse_amd.enhance import enhance_recording
    from flowmse_amd.resample import resample
    rate, n, H, X = 48000, 50001, 16, 4
    y = _signal(31, n)
    geo = dict(chunk_frames=TC, hop_frames=H, fade_frames=X)
    want, sr, _ = enhance_recording(full, y.cuda(), rate, "input", batch=1, noise_key=KEY, noise_seed=SEED, **geo, **SOLVER)
    assert sr == rate and want.shape == (n,)
    norm = resample(y.cuda(), rate, 16000).abs().max().item()
    live = LiveEnhancer(full, norm=norm, key=KEY, seed=SEED, input_rate=rate, output_rate="input", **geo, **SOLVER)
    assert live.latency_samples == latency_samples(TC, rate, "input", hop_frames=H, fade_frames=X) >= 3 * (128 * (H + X) + 382)
    assert live.latency_samples < latency_samples(TC, rate, "input", 16)
    for sizes in ([n], [6144] * (n // 6144) + [n % 6144]):
        got = _run_live(live, y[0], sizes)
        assert live.samples_in == live.samples_out == n
        assert np.array_equal(got, want), (int((got != want).sum()), int(np.flatnonzero(got != want)[0]))
        live.reset()
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0


# ---------------------------------------------------------------------------------------------------- 4
def test_without_the_keywords_nothing_changed(full, monkeypatch):
    """``LiveEnhancer`` without ``hop_frames`` returns the bytes of ``enhance_long(batch=1)`` and never calls a trailing entry:
    the four new bindings are patched to raise."""
    def boom(*a, **k):
        raise AssertionError("a trailing entry was called without hop_frames")
    for name in ("flowse_stft_compress_trailing", "flowse_istft_decompress_trailing", "flowse_stft_compress_trailing_window",
                 "flowse_istft_decompress_trailing_window"):
        assert callable(getattr(_lib.lib, name))
        monkeypatch.setattr(_lib.lib, name, boom)
    Ls, To = 20000, 16
    sig = _signal(41, Ls)
    want = enhance_long(full, sig.cuda(), TC, To, batch=1, noise_key=KEY, noise_seed=SEED, **SOLVER)
    live = LiveEnhancer(full, norm=sig.abs().max().item(), key=KEY, seed=SEED, chunk_frames=TC, overlap_frames=To, **SOLVER)
    assert live.H is None and live.latency_samples == 128 * TC + 382
    got = _run_live(live, sig[0], [2048] * (Ls // 2048) + [Ls % 2048])
    assert np.array_equal(got, want) and float(np.abs(want).max()) > 0
    with pytest.raises(AssertionError, match="trailing entry"):
        LiveEnhancer(full, norm=0.5, key=KEY, chunk_frames=TC, hop_frames=16, N=1).push(np.zeros(128 * 15 + 255, dtype=np.float32))
    with pytest.raises(ValueError, match="hop_frames"):
        LiveEnhancer(full, norm=0.5, key=KEY, chunk_frames=TC, fade_frames=4)
