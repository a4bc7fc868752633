"""GPU: recordings of any length (flowmse_amd.chunked) -- the chunked STFT against slices of ``analyze``, the keyed noise
at frame offsets against slices of the offset-free stream, the seam kernel against the float64 blend, ``enhance_long``
against the oracle composition (oracle sampler per chunk + the same cross-fade on the host), and the
``flowmse_amd.enhance`` CLI in child processes, one after the other, each under its own time limit.  No test asserts a time.
"""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cases as C
from flowmse_amd import _lib
from flowmse_amd.chunked import blend_chunks_reference, enhance_long, plan_chunks
from flowmse_amd.util import synth
from flowmse_amd.util.noise import keyed_noise_reference

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
KEY, SEED = 0x912975D344AF26C6, 0x1F2E3D4C5B6A7988
NOISE_BOUND = 4 * 3.755e-7        # tests/test_gpu_keyed_noise.py: 4 x the largest |kernel - float64| measured there
ISTFT_TOL = 2e-5                  # tests/test_gpu_ops.py: the fused iSTFT against torch.istft
GEOMETRIES = [(64, 0), (64, 16), (128, 64), (256, 32)]


def _dev_keys(keys):
    return torch.tensor([k - 2 ** 64 if k >= 2 ** 63 else k for k in keys], dtype=torch.int64, device="cuda")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _model(cfg):
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **cfg)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def full():
    assert torch.cuda.is_available()
    return _model(C.FULL)


@pytest.fixture(scope="module")
def dm():
    from flowmse_amd.data_module import SpecTransform
    return SpecTransform()


def _signal(seed, n, std=0.1):
    return torch.from_numpy(synth.normal(seed, 9, (1, n), std))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("Ls", [20000, 64000, 98765])
def test_chunked_stft_is_slices_of_analyze(dm, Ls):
    sig = _signal(Ls % 97, Ls).cuda()
    whole = dm.analyze(sig, 0.37)                                                  # [1,1,256,Tpad], zeros past T
    T = Ls // 128 + 1
    for Tc, To in GEOMETRIES:
        K, hop, Tg = plan_chunks(T, Tc, To)
        ext = torch.nn.functional.pad(whole, (0, max(Tg - whole.size(3), 0)))
        got = dm.analyze_chunks(sig, Tc, hop, 0.37)
        torch.cuda.synchronize()
        assert got.shape == (K, 1, 256, Tc) and got.dtype == torch.complex64
        for k in range(K):
            assert torch.equal(got[k], ext[0, :, :, k * hop:k * hop + Tc]), (Ls, Tc, To, k)
        assert bool((got[-1][..., T - (K - 1) * hop:] == 0).all())                 # the tail chunk's padding


def test_chunked_stft_shape_errors_return_a_status_and_launch_nothing():
    sig = _signal(1, 20000).cuda()                                                 # 157 frames: 3 chunks at (64, 16)
    out = torch.full((3, 1, 256, 64), 7.0, dtype=torch.complex64, device="cuda")
    s, p = _lib.current_stream(), _lib.ptr
    bad = [(20000, 2, 64, 48), (20000, 0, 64, 48), (20000, 3, 64, 0), (20000, 3, 64, 65), (20000, 3, 64, 30), (200, 1, 64, 48),
           (20000, 70000, 64, 48)]
    for Ls, K, Tc, hop in bad:
        assert L.flowse_stft_compress_chunks(p(sig), Ls, 1.0, p(out), K, Tc, hop, 0.15, 0.5, s) == ERR_SHAPE, (Ls, K, Tc, hop)
        assert b"stft chunks" in L.flowse_last_error()
    assert L.flowse_stft_compress_chunks(None, 20000, 1.0, p(out), 3, 64, 48, 0.15, 0.5, s) == ERR_ARG
    assert L.flowse_stft_compress_chunks(p(sig), 20000, 1.0, None, 3, 64, 48, 0.15, 0.5, s) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _lib.check(L.flowse_stft_compress_chunks(p(sig), 20000, 1.0, p(out), 3, 64, 48, 0.15, 0.5, s))
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("F,Tc,To,K", [(256, 64, 16, 5), (64, 256, 32, 3), (8, 128, 64, 4)])
def test_keyed_noise_at_offsets_is_slices_of_the_stream(F, Tc, To, K):
    hop = Tc - To
    Tg = (K - 1) * hop + Tc
    offs = [k * hop for k in range(K)]
    s, p = _lib.current_stream(), _lib.ptr
    whole = torch.empty(1, 1, F, Tg, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_op_keyed_noise(p(_dev_keys([KEY])), SEED, p(whole), 1, F, Tg, s))
    rows = torch.empty(K, 1, F, Tc, dtype=torch.complex64, device="cuda")
    kd, fd = _dev_keys([KEY] * K), _i32(offs)
    _lib.check(L.flowse_op_keyed_noise_at(p(kd), p(fd), SEED, p(rows), K, F, Tc, s))
    torch.cuda.synchronize()
    for k, o in enumerate(offs):
        assert torch.equal(rows[k], whole[0, :, :, o:o + Tc]), k
    # zero offsets are the offset-free call
    z0, z1 = torch.empty_like(rows), torch.empty_like(rows)
    _lib.check(L.flowse_op_keyed_noise(p(kd), SEED, p(z0), K, F, Tc, s))
    _lib.check(L.flowse_op_keyed_noise_at(p(kd), p(_i32([0] * K)), SEED, p(z1), K, F, Tc, s))
    assert torch.equal(z0, z1) and not torch.equal(z0, rows)
    # the prior sample of the rows against slices of the prior sample of the whole Tg-frame row
    y = C.c64(synth.synth_spectrogram(4, 1, F, Tg)).cuda()
    xw = torch.empty_like(y)
    _lib.check(L.flowse_prior_sample_keyed(p(y), p(_dev_keys([KEY])), SEED, 0.487, p(xw), 1, F, Tg, s))
    yr = torch.cat([y[..., o:o + Tc] for o in offs], dim=0).contiguous()
    xr = torch.empty_like(yr)
    _lib.check(L.flowse_prior_sample_keyed_at(p(yr), p(kd), p(fd), SEED, 0.487, p(xr), K, F, Tc, s))
    torch.cuda.synchronize()
    for k, o in enumerate(offs):
        assert torch.equal(xr[k], xw[0, :, :, o:o + Tc]), k
    assert not torch.equal(xr, yr)
    # and the float64 restatement, within the bound of the offset-free kernel
    ref = keyed_noise_reference([KEY] * K, SEED, F, Tc, frame0=offs)
    d = rows.cpu().numpy().astype(np.complex128) - ref
    worst = max(np.abs(d.real).max(), np.abs(d.imag).max())
    print(f"keyed noise at offsets [{K},{F},{Tc}] hop {hop}: max |kernel - float64| = {worst:.3e}")
    assert worst <= NOISE_BOUND, worst
    # the facade and the solver argument take the same path
    from flowmse_amd.odes import FLOWMATCHING
    ode = FLOWMATCHING()
    x, none = ode.prior_sampling(yr.shape, yr, keys=[KEY] * K, seed=SEED, frame0=offs)
    assert none is None and torch.equal(x, ode.prior_sampling(yr.shape, yr, rows)[0])


def test_keyed_noise_bad_offsets_return_a_status_and_leave_the_output_untouched():
    B, F, T = 3, 8, 16
    y = torch.zeros(B, 1, F, T, dtype=torch.complex64, device="cuda")
    out = torch.full_like(y, 7.0)
    kd = _dev_keys([KEY] * B)
    s, p = _lib.current_stream(), _lib.ptr
    for offs in ([0, 1, 2], [0, -2, 4], [15, 0, 0], [0, 0, 2 ** 31 - 2]):
        assert L.flowse_prior_sample_keyed_at(p(y), p(kd), p(_i32(offs)), 1, 0.5, p(out), B, F, T, s) == ERR_ARG, offs
        assert b"flowse_prior_sample_keyed_at" in L.flowse_last_error() and b"frame0" in L.flowse_last_error()
        assert L.flowse_op_keyed_noise_at(p(kd), p(_i32(offs)), 1, p(out), B, F, T, s) == ERR_ARG, offs
        assert b"flowse_op_keyed_noise_at" in L.flowse_last_error()
    assert L.flowse_op_keyed_noise_at(p(kd), None, 1, p(out), B, F, T, s) == ERR_ARG
    assert L.flowse_prior_sample_keyed_at(p(y), p(kd), None, 1, 0.5, p(out), B, F, T, s) == ERR_ARG
    assert L.flowse_op_keyed_noise_at(p(kd), p(_i32([0, 2, 4])), 1, p(out), B, F, T - 1, s) == ERR_ARG      # odd T
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    from flowmse_amd.odes import FLOWMATCHING
    with pytest.raises(ValueError):
        FLOWMATCHING().prior_sampling(y.shape, y, keys=[KEY] * B, frame0=[0, 2, 5])
    _lib.check(L.flowse_op_keyed_noise_at(p(kd), p(_i32([0, 2, 2 ** 31 - 2 - T])), 1, p(out), B, F, T, s))
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("Tc,To,K", [(64, 16, 4), (128, 64, 3), (256, 32, 3), (64, 0, 3)])
def test_seams_match_the_float64_blend(dm, Tc, To, K):
    """Independent random chunks: neighbouring chunks disagree completely on their shared frames, so a wrong weight is
    visible far above the bound -- the blend with w = j / To instead of (j + 0.5) / To is asserted to be > 1e-3 away.
    Measured on an MI355X: 3.5e-8 .. 9.8e-8 against the bound of 2e-5."""
    hop = Tc - To
    Tg = (K - 1) * hop + Tc
    chunks = C.c64(synth.synth_spectrogram(30 + Tc + To, K, 256, Tc)).cuda()
    length = 128 * (Tg - 1) - 37
    got = dm.synthesize_chunks(chunks, hop, length, 0.7)
    blend = blend_chunks_reference(chunks, hop)
    want = dm.synthesize(torch.from_numpy(blend).to(torch.complex64).cuda(), length, 0.7)
    torch.cuda.synchronize()
    assert got.shape == (1, length) and torch.isfinite(got).all()
    err = C.rel_l2(got.cpu(), want.cpu())
    print(f"seams Tc {Tc} To {To} K {K}: rel-L2 vs synthesize(float64 blend) = {err:.3e}")
    assert err < ISTFT_TOL
    if To:
        c = chunks.cpu().numpy().astype(np.complex128)
        wrong = blend.copy()
        w = np.arange(To) / To
        for k in range(1, K):
            a, b = c[k - 1][:, :, hop:], c[k][:, :, :To]
            wrong[0, :, :, k * hop:k * hop + To] = a + w * (b - a)
        off = dm.synthesize(torch.from_numpy(wrong).to(torch.complex64).cuda(), length, 0.7)
        assert C.rel_l2(got.cpu(), off.cpu()) > 1e-3


@pytest.mark.parametrize("Tc,To", GEOMETRIES, ids=lambda v: str(v))
def test_chunks_cut_from_one_spectrogram_synthesize_bit_for_bit(dm, Tc, To):
    K, hop, Tg = plan_chunks(3 * Tc + 5, Tc, To)
    S = C.c64(synth.synth_spectrogram(7, 1, 256, Tg)).cuda()
    chunks = torch.cat([S[..., k * hop:k * hop + Tc] for k in range(K)], dim=0).contiguous()
    for length in (128 * (Tg - 1), 128 * (Tg - 1) + 255, 12345):
        got, want = dm.synthesize_chunks(chunks, hop, length, 1.3), dm.synthesize(S, length, 1.3)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (Tc, To, length)


def test_seam_kernel_shape_errors_return_a_status_and_launch_nothing():
    chunks = torch.zeros(3, 1, 256, 64, dtype=torch.complex64, device="cuda")     # Tg = 160 at hop 48
    out = torch.full((1, 128 * 159 + 255 + 1), 7.0, device="cuda")
    s, p = _lib.current_stream(), _lib.ptr
    bad = [(0, 64, 48, 1000, 0.15), (3, 64, 30, 1000, 0.15), (3, 64, 65, 1000, 0.15), (3, 64, 0, 1000, 0.15),
           (3, 64, 48, 0, 0.15), (3, 64, 48, 128 * 159 + 256, 0.15), (3, 64, 48, 1000, 0.0)]
    for K, Tc, hop, Lout, factor in bad:
        assert L.flowse_istft_decompress_chunks(p(chunks), K, Tc, hop, factor, 0.5, p(out), Lout, 1.0, s) == ERR_SHAPE
        assert b"istft chunks" in L.flowse_last_error()
    assert L.flowse_istft_decompress_chunks(None, 3, 64, 48, 0.15, 0.5, p(out), 1000, 1.0, s) == ERR_ARG
    assert L.flowse_istft_decompress_chunks(p(chunks), 3, 64, 48, 0.15, 0.5, None, 1000, 1.0, s) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _lib.check(L.flowse_istft_decompress_chunks(p(chunks), 3, 64, 48, 0.15, 0.5, p(out), 128 * 159 + 255, 1.0, s))
    torch.cuda.synchronize()
    assert bool((out[0, :-1] == 0.0).all()) and float(out[0, -1]) == 7.0


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.timeout(900)
def test_enhance_long_vs_oracle_composition(full):
    """Full net, synthetic weights, 20000 samples as three chunks of 64 frames overlapping by 16, N = 2, explicit global
    z: the HIP path against the oracle field per chunk driven through the same host code and the float64 cross-fade.
    Bound: 1e-3 waveform rel-L2, that of test_end_to_end_utterance_vs_oracle.  Measured on an MI355X: 5.2e-7 (and 0.13
    between the chunked and the single-tensor result on these synthetic weights: different computations)."""
    from oracle import ncsnpp_oracle as O
    tb = C.param_tables()["full"]
    w = C.synth_weights(tb["names"], tb["shapes"])
    sig = _signal(3, 20000)
    K, hop, Tg = plan_chunks(20000 // 128 + 1, 64, 16)
    assert (K, Tg) == (3, 160)
    z = C.c64(synth.synth_noise(2, 1, 256, Tg))
    kw = dict(chunk_frames=64, overlap_frames=16, N=2)
    ref = enhance_long(full, sig, z=z, VF_fn=lambda x, t, y: O.vf_forward(w, O.make_cfg(), x, t, y), device="cpu", **kw)
    got = enhance_long(full, sig.cuda(), z=z.cuda(), **kw)
    err = _rel(got, ref)
    print("chunked end-to-end waveform rel-L2 vs oracle composition", err)
    assert got.shape == ref.shape == (20000,) and np.isfinite(got).all() and err < 1e-3
    # the chunks matter: the single-tensor path on the same recording is a different computation
    from flowmse_amd.evaluate import enhance_waveform
    one = enhance_waveform(full, sig.cuda(), N=2, z=torch.nn.functional.pad(z, (0, 192 - Tg)).cuda())
    print("chunked vs single-tensor path, waveform rel-L2", _rel(got, one))


# ---------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("n", [20000, 255 * 128])
def test_single_chunk_is_enhance_waveform(full, n):
    """157 and exactly 256 frames fit one default chunk: the same bytes as enhance_waveform with the same key and seed."""
    from flowmse_amd.evaluate import enhance_waveform
    sig = _signal(5, n).cuda()
    assert plan_chunks(n // 128 + 1)[0] == 1 and plan_chunks(255 * 128 // 128 + 2)[0] == 2
    want = enhance_waveform(full, sig, N=2, noise_keys=[KEY], noise_seed=SEED)
    got = enhance_long(full, sig, N=2, noise_key=KEY, noise_seed=SEED)
    assert got.shape == (n,) and got.tobytes() == want.tobytes()
    assert enhance_long(full, sig, N=2, noise_key=KEY, noise_seed=SEED + 1).tobytes() != want.tobytes()


# ---------------------------------------------------------------------------------------------------- 6
def test_batch_width_and_repeatability(full):
    """64000 samples = 501 frames = 11 chunks at (64, 16): batch 1 / 3 / 8 run 11 / 4 / 2 sampler calls of widths
    1 / (3,3,3,2) / (8,3).  Bound between widths: 1e-5 rel-L2, the batched-versus-alone bound.  Measured on an MI355X:
    batch 3 vs 8 4.7e-7, batch 1 vs 8 5.3e-7."""
    sig, other = _signal(6, 64000).cuda(), _signal(8, 30000).cuda()
    kw = dict(chunk_frames=64, overlap_frames=16, N=2, noise_key=KEY, noise_seed=SEED)
    assert plan_chunks(501, 64, 16)[0] == 11
    out = {b: enhance_long(full, sig, batch=b, **kw) for b in (8, 3, 1)}
    for b in (3, 1):
        err = _rel(out[b], out[8])
        print(f"batch {b} vs batch 8: waveform rel-L2 {err:.3e}")
        assert err <= 1e-5, (b, err)
    assert all(np.isfinite(v).all() and v.shape == (64000,) for v in out.values())
    assert enhance_long(full, sig, batch=8, **kw).tobytes() == out[8].tobytes()            # the same call twice
    enhance_long(full, other, batch=8, **dict(kw, noise_key=KEY + 1))                      # another recording in between
    enhance_long(full, other, batch=3, **kw)
    assert enhance_long(full, sig, batch=3, **kw).tobytes() == out[3].tobytes()
    assert enhance_long(full, sig, batch=8, **dict(kw, noise_seed=SEED + 1)).tobytes() != out[8].tobytes()
    # the torch generator: one draw for the recording, the same files under the same seed
    tk = dict(chunk_frames=64, overlap_frames=16, N=2)
    torch.manual_seed(4)
    a = enhance_long(full, sig, **tk)
    torch.manual_seed(4)
    assert enhance_long(full, sig, **tk).tobytes() == a.tobytes() and a.tobytes() != out[8].tobytes()


# ---------------------------------------------------------------------------------------------------- 7
@pytest.mark.timeout(900)
def test_memory_does_not_grow_with_the_recording():
    """A 60 s recording (7501 frames, 34 chunks at the defaults) after a 10 s one (1251 frames, 6 chunks) on a fresh model,
    N = 1, batch 4 -- a width both recordings fill, so that every buffer the handle owns (the workspace and the N x B
    floats of the time table) has its final size after the first: the owned device bytes must not move."""
    model = _model(C.FULL)
    h = model.dnn._handle
    assert plan_chunks(160000 // 128 + 1) == (6, 224, 1376) and plan_chunks(960000 // 128 + 1) == (34, 224, 7648)
    kw = dict(batch=4, N=1, noise_key=KEY, noise_seed=SEED)
    x10 = enhance_long(model, _signal(10, 160000).cuda(), **kw)
    b10 = int(L.flowse_model_device_bytes(h, _lib.FLOWSE_BYTES_OWNED))
    x60 = enhance_long(model, _signal(60, 960000).cuda(), **kw)
    b60 = int(L.flowse_model_device_bytes(h, _lib.FLOWSE_BYTES_OWNED))
    print(f"owned device bytes after 10 s: {b10}, after 60 s: {b60}; workspace of [4,1,256,256]: {model.dnn.reserve(4, 256, 256)}")
    assert x10.shape == (160000,) and np.isfinite(x10).all()
    assert x60.shape == (960000,) and np.isfinite(x60).all() and float(np.abs(x60).max()) > 0
    assert b10 > 0 and b60 == b10
    assert b10 >= model.dnn.reserve(4, 256, 256)


# ---------------------------------------------------------------------------------------------------- 8
def _enhance(out, extra, limit=500):
    return subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "flowmse_amd.enhance", "--output", str(out)]
                          + extra, cwd=ROOT, capture_output=True, text=True)


@pytest.mark.timeout(1200)
def test_enhance_cli_in_a_child_process_twice(tmp_path):
    """``--synthetic 2 --synthetic_seconds 1,7``: a single-chunk file (126 frames) and a chunked one (876 frames, 4 chunks);
    the second run writes the same bytes.  Children run one after the other; a failed one ends the test."""
    from scipy.io import wavfile
    args = ["--synthetic", "2", "--synthetic_seconds", "1,7", "--N", "2", "--seed", "3"]
    assert plan_chunks(16000 // 128 + 1)[0] == 1 and plan_chunks(112000 // 128 + 1)[0] == 4
    for tag in ("a", "b"):
        r = _enhance(tmp_path / tag, args)
        assert r.returncode == 0, f"run {tag} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    names = sorted(n for n in os.listdir(tmp_path / "a") if n.endswith(".wav"))
    assert names == ["synthetic_00.wav", "synthetic_01.wav"]
    for n, samples in zip(names, (16000, 112000)):
        sr, data = wavfile.read(tmp_path / "a" / n)
        assert sr == 16000 and data.shape == (samples,) and data.dtype == np.int16 and np.abs(data).max() > 0
        assert filecmp.cmp(tmp_path / "a" / n, tmp_path / "b" / n, shallow=False), n
    settings = (tmp_path / "a" / "_settings.txt").read_text()
    assert "chunk_frames: 256\noverlap_frames: 32\n" in settings and settings.endswith("noise: keyed\nnoise seed: 3\n")
    assert settings == (tmp_path / "b" / "_settings.txt").read_text()
