"""GPU: the pooled mode (flowmse_amd.pooled) -- ``flowse_stft_compress_rows`` against rows of ``analyze_chunks``,
``flowse_istft_decompress_stacks`` against ``synthesize_chunks`` per stack, ``enhance_pooled`` against ``enhance_long`` and
against each channel alone through the existing pieces, folder independence bit for bit, and ``enhance --pool`` in child
processes, one after the other, each under its own time limit.  No test asserts a time.
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
from flowmse_amd.chunked import enhance_long, plan_chunks
from flowmse_amd.pooled import channel_key, enhance_pooled, plan_pool
from flowmse_amd.util import synth
from flowmse_amd.util.noise import utterance_key

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
SEED = 0x1F2E3D4C5B6A7988
ALONE_BOUND = 1e-5               # tests/test_gpu_chunked.py::test_batch_width_and_repeatability: batched versus alone
TC, TO, HOP = 64, 16, 48


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


def _table(rows):
    t = (_lib.flowse_spec_row * max(len(rows), 1))()
    for d, (ptr, n, frame0, scale) in zip(t, rows):
        d.sig, d.L, d.frame0, d.scale_in = ptr, n, frame0, scale
    return t


# ---------------------------------------------------------------------------------------------------- 1
def test_rows_stft_is_rows_of_analyze_chunks(dm):
    """Rows from three signals under three scales in one launch: chunk rows (tail chunks with their zero padding), rows
    that start inside and past a signal's last frame, one signal named by several rows.  R = 1, 17 and 64."""
    sigs = [(_signal(1, 20000).cuda(), 0.37), (_signal(2, 64000).cuda(), 1.9), (_signal(3, 300).cuda(), 0.5)]
    want = []                                                       # (signal, frame0, expected [1,256,64])
    for s, (sig, scale) in enumerate(sigs):
        chunks = dm.analyze_chunks(sig, TC, HOP, scale)
        assert chunks.shape[0] == (3, 11, 1)[s]
        want += [(s, k * HOP, chunks[k]) for k in range(chunks.shape[0])]
    # 20000 samples = 157 frames: the row at 144 ends in padding, the row at 192 is padding only
    whole = torch.nn.functional.pad(dm.analyze(sigs[0][0], sigs[0][1]), (0, 64))
    want += [(0, 144, whole[0, :, :, 144:208]), (0, 192, torch.zeros(1, 256, 64, dtype=torch.complex64, device="cuda"))]
    assert bool((whole[0, :, :, 157:] == 0).all()) and bool((want[-2][2][..., :13] != 0).any())
    order = np.random.default_rng(0).permutation(len(want)).tolist()
    for R in (len(want), 1, 64):
        pick = [want[order[i % len(want)]] for i in range(R)]
        got = dm.analyze_rows([(sigs[s][0][0], f0, sigs[s][1]) for s, f0, _ in pick], TC)
        torch.cuda.synchronize()
        assert got.shape == (R, 1, 256, TC) and got.dtype == torch.complex64
        for r, (s, f0, ref) in enumerate(pick):
            assert torch.equal(got[r], ref), (R, r, s, f0)
    # the training crop's width
    sig, scale = sigs[1]
    chunks = dm.analyze_chunks(sig, 256, 224, scale)
    got = dm.analyze_rows([(sig[0], k * 224, scale) for k in (2, 0, 1)] + [(sigs[2][0][0], 0, 0.5)], 256)
    torch.cuda.synchronize()
    assert chunks.shape[0] == 3 and all(torch.equal(got[r], chunks[k]) for r, k in enumerate((2, 0, 1)))
    assert torch.equal(got[3][..., :64], want[14][2]) and bool((got[3][..., 3:] == 0).all())


# ---------------------------------------------------------------------------------------------------- 2
def test_rows_stft_errors_return_a_status_and_launch_nothing():
    sig = _signal(1, 20000).cuda()
    out = torch.full((64, 1, 256, 64), 7.0, dtype=torch.complex64, device="cuda")
    s, p, a = _lib.current_stream(), _lib.ptr, sig.data_ptr()
    good = (a, 20000, 48, 1.0)
    for rows, R, Tw, rc in [([good], 0, 64, ERR_SHAPE), ([good] * 65, 65, 64, ERR_SHAPE), ([good, (a, 255, 0, 1.0)], 2, 64, ERR_SHAPE),
                            ([good], 1, 0, ERR_SHAPE), ([good, (a, 20000, 2 ** 23 - 63, 1.0)], 2, 64, ERR_SHAPE),
                            ([(a, 20000, -2, 1.0), good], 2, 64, ERR_ARG), ([good, good, (None, 20000, 0, 1.0)], 3, 64, ERR_ARG)]:
        assert L.flowse_stft_compress_rows(_table(rows), R, Tw, p(out), 0.15, 0.5, s) == rc, (R, Tw, rows[-1][1:])
        assert b"stft rows" in L.flowse_last_error()
    assert L.flowse_stft_compress_rows(None, 1, 64, p(out), 0.15, 0.5, s) == ERR_ARG
    assert L.flowse_stft_compress_rows(_table([good]), 1, 64, None, 0.15, 0.5, s) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _lib.check(L.flowse_stft_compress_rows(_table([good, (a, 20000, 2 ** 23 - 64, 1.0)]), 2, 64, p(out), 0.15, 0.5, s))
    torch.cuda.synchronize()
    assert not bool((out[0] == 7.0).any()) and bool((out[1] == 0.0).all()) and bool((out[2:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("S,K,Tc,hop,lengths", [(3, 3, 64, 48, (128 * 159, 128 * 159 + 255, 12345)),
                                                (1, 1, 64, 64, (128 * 63, 128 * 63 + 255, 5000)),
                                                (2, 1, 128, 128, (128 * 127 + 255, 12345))])
def test_stacks_istft_is_synthesize_chunks_per_stack(dm, S, K, Tc, hop, lengths):
    chunks = C.c64(synth.synth_spectrogram(40 + S + Tc, S * K, 256, Tc)).cuda()
    for length in lengths:
        got = dm.synthesize_stacks(chunks, S, hop, length, 0.7)
        torch.cuda.synchronize()
        assert got.shape == (S, length) and torch.isfinite(got).all()
        for s in range(S):
            assert torch.equal(got[s:s + 1], dm.synthesize_chunks(chunks[s * K:(s + 1) * K], hop, length, 0.7)), (s, length)
        assert S == 1 or not torch.equal(got[0], got[1])
    if K == 1:                                                      # a one-chunk stack is the plain inverse transform
        assert torch.equal(got, dm.synthesize(chunks, lengths[-1], 0.7))


def test_stacks_istft_shape_errors_return_a_status_and_launch_nothing(dm):
    chunks = torch.zeros(6, 1, 256, 64, dtype=torch.complex64, device="cuda")     # 2 stacks, Tg = 160 at hop 48
    top = 128 * 159 + 255
    out = torch.full((2, top + 1), 7.0, device="cuda")
    s, p = _lib.current_stream(), _lib.ptr
    bad = [(0, 3, 64, 48, 1000, 0.15), (65536, 3, 64, 48, 1000, 0.15), (-1, 3, 64, 48, 1000, 0.15),
           (2, 0, 64, 48, 1000, 0.15), (2, 3, 64, 30, 1000, 0.15), (2, 3, 64, 65, 1000, 0.15), (2, 3, 64, 0, 1000, 0.15),
           (2, 3, 64, 48, 0, 0.15), (2, 3, 64, 48, top + 1, 0.15), (2, 3, 64, 48, 1000, 0.0)]
    for S, K, Tc, hop, Lout, factor in bad:
        assert L.flowse_istft_decompress_stacks(p(chunks), S, K, Tc, hop, factor, 0.5, p(out), Lout, 1.0, s) == ERR_SHAPE
        assert b"istft stacks" in L.flowse_last_error()
    assert L.flowse_istft_decompress_stacks(None, 2, 3, 64, 48, 0.15, 0.5, p(out), 1000, 1.0, s) == ERR_ARG
    assert L.flowse_istft_decompress_stacks(p(chunks), 2, 3, 64, 48, 0.15, 0.5, None, 1000, 1.0, s) == ERR_ARG
    with pytest.raises(ValueError):
        dm.synthesize_stacks(chunks, 4, 48, 1000)                   # 6 rows are not 4 equal stacks
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _lib.check(L.flowse_istft_decompress_stacks(p(chunks), 2, 3, 64, 48, 0.15, 0.5, p(out), top, 1.0, s))
    torch.cuda.synchronize()
    assert bool((out.reshape(-1)[:2 * top] == 0.0).all()) and bool((out.reshape(-1)[2 * top:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 4, 5
FILES = [("a.wav", 1, 20000), ("b.wav", 2, 12000), ("c.wav", 1, 5000)]


def _samples():
    b = torch.cat([_signal(12, 12000), 0.5 * _signal(13, 12000)], dim=0)         # channel 1 at half level
    return {"a.wav": _signal(11, 20000), "b.wav": b, "c.wav": _signal(14, 5000)}


def _run_pooled(full, items, batch=3):
    samples, out = _samples(), {}
    loads = []

    def load(i):
        loads.append(items[i][0])
        return samples[items[i][0]].cuda()

    def write(i, x_hat):
        out[items[i][0]] = x_hat.cpu()

    stats = enhance_pooled(full, load, items, write, batch=batch, chunk_frames=TC, overlap_frames=TO, N=2, noise_seed=SEED)
    assert loads == [n for n, _, _ in items] and set(out) == set(loads)          # each file loaded once, in order
    return out, stats


@pytest.fixture(scope="module")
def folder_abc(full):
    return _run_pooled(full, FILES)


def test_pooled_run_against_the_existing_pieces(full, dm, folder_abc):
    """Three files, 8 rows, batch 3: three calls with one filler.  a.wav fills a call alone and is ``enhance_long``'s bytes;
    every other channel is held to the channel alone through analyze_chunks (scale 1 / the FILE's peak) -> the solver with
    ``channel_key`` and the same ``frame0`` -> synthesize_chunks, within the batched-versus-alone bound of 1e-5 rel-L2.
    Measured on an MI355X: see DESIGN 6d."""
    from flowmse_amd.sampling import get_white_box_solver
    out, stats = folder_abc
    calls = plan_pool(FILES, 3, TC, TO)
    assert [plan_chunks(n // 128 + 1, TC, TO)[0] for _, _, n in FILES] == [3, 2, 1]
    assert stats == dict(calls=3, rows=8, fillers=1) and [c.width for c in calls] == [64, 64, 64]
    assert [r.item for r in calls[0].rows] == [0, 0, 0] and [r.filler for r in calls[2].rows] == [False, False, True]
    samples = _samples()
    for name, ch, n in FILES:
        assert out[name].shape == (ch, n) and out[name].dtype == torch.float32 and torch.isfinite(out[name]).all()
    want = enhance_long(full, samples["a.wav"].cuda(), chunk_frames=TC, overlap_frames=TO, batch=3, N=2,
                        noise_key=utterance_key("a.wav"), noise_seed=SEED)
    assert out["a.wav"][0].numpy().tobytes() == want.tobytes()

    def alone(name, c, peak):
        sig = samples[name][c:c + 1].cuda()
        Y = dm.analyze_chunks(sig, TC, HOP, 1.0 / peak)
        K = Y.shape[0]
        x = get_white_box_solver("euler", full.ode, full, Y=Y, Y_prior=Y, N=2, noise_keys=[channel_key(name, c)] * K,
                                 noise_seed=SEED, noise_frame0=[k * HOP for k in range(K)])()[0]
        return dm.synthesize_chunks(x, HOP, sig.shape[1], peak)[0].cpu()

    for name, c in (("b.wav", 0), ("b.wav", 1), ("c.wav", 0), ("a.wav", 0)):
        err = _rel(out[name][c], alone(name, c, samples[name].abs().max().item()))
        print(f"pooled vs alone, {name} channel {c}: waveform rel-L2 {err:.3e}")
        assert err <= ALONE_BOUND, (name, c, err)
    # two channels, each its own signal under its own key, both under the file's ONE factor: channel 1 normalised by its own
    # peak meets a prior noise twice as loud relative to it -- another computation, far outside the bound
    b = out["b.wav"]
    assert not torch.equal(b[0], b[1]) and _rel(b[1], b[0]) > 0.1
    own = _rel(b[1], alone("b.wav", 1, samples["b.wav"][1].abs().max().item()))
    print(f"b.wav channel 1 under its own peak instead of the file's: rel-L2 {own:.3e}")
    assert own > 1e-3


def test_a_files_samples_do_not_depend_on_the_folder(full, folder_abc):
    """{a, b, c} against {c, a}: a.wav's rows sit at other positions beside other neighbours (c, a0, a1 | a2, filler, filler
    against a0, a1, a2), c.wav moves from the middle of a call to its head.  Bit for bit, no tolerance."""
    out, _ = folder_abc
    other, stats = _run_pooled(full, [FILES[2], FILES[0]])
    assert stats == dict(calls=2, rows=4, fillers=2)
    for name in ("a.wav", "c.wav"):
        assert torch.equal(other[name], out[name]), name


# ---------------------------------------------------------------------------------------------------- 6
def _enhance(out, extra, limit=500):
    return subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "flowmse_amd.enhance", "--output", str(out)]
                          + extra, cwd=ROOT, capture_output=True, text=True)


@pytest.mark.timeout(1800)
def test_enhance_pool_cli_in_child_processes(tmp_path):
    """1 s mono, 7 s stereo (4 chunks per channel), 2 s mono at ``--batch 1``: the pooled run twice (same bytes), the
    unpooled run (width-1 calls are the same computation: the mono files are byte-identical), and the pooled run from and
    back to 44.1 kHz.  Children run one after the other; a failed one ends the test."""
    from scipy.io import wavfile
    base = ["--synthetic", "3", "--synthetic_seconds", "1,7,2", "--synthetic_channels", "1,2,1", "--batch", "1", "--N", "2",
            "--seed", "3"]
    pool = base + ["--pool", "--channels", "all"]
    runs = [("a", pool), ("b", pool), ("plain", base),
            ("r", pool + ["--synthetic_rate", "44100", "--resample", "--output_rate", "input"])]
    for tag, args in runs:
        r = _enhance(tmp_path / tag, args)
        assert r.returncode == 0, f"run {tag} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    names = ["synthetic_00.wav", "synthetic_01.wav", "synthetic_02.wav"]
    assert sorted(n for n in os.listdir(tmp_path / "a") if n.endswith(".wav")) == names
    for n, secs, ch in zip(names, (1, 7, 2), (1, 2, 1)):
        sr, data = wavfile.read(tmp_path / "a" / n)
        assert sr == 16000 and data.dtype == np.int16 and data.shape == ((16000 * secs,) if ch == 1 else (16000 * secs, ch))
        assert np.abs(data).max() > 0
        assert filecmp.cmp(tmp_path / "a" / n, tmp_path / "b" / n, shallow=False), n
        if ch == 1:
            assert filecmp.cmp(tmp_path / "a" / n, tmp_path / "plain" / n, shallow=False), n
        else:
            mono = wavfile.read(tmp_path / "plain" / n)[1]
            assert mono.shape == (16000 * secs,) and not np.array_equal(data[:, 0], data[:, 1])
        sr, data = wavfile.read(tmp_path / "r" / n)
        assert sr == 44100 and data.shape == ((44100 * secs,) if ch == 1 else (44100 * secs, ch)) and np.abs(data).max() > 0
    settings = (tmp_path / "a" / "_settings.txt").read_text()
    assert "pool: True\nchannels: all\n" in settings and settings.endswith("noise: keyed\nnoise seed: 3\n")
    assert settings == (tmp_path / "b" / "_settings.txt").read_text()
    assert "pool" not in (tmp_path / "plain" / "_settings.txt").read_text()
