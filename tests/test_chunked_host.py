"""CPU: chunk geometry, the seam rule's float64 restatement, the keyed noise stream at frame offsets, the C-ABI surface
of the chunked calls and the ``flowmse_amd.enhance`` command line (no GPU compute calls)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(64, 0), (64, 16), (128, 64), (256, 32)]
NEW_SYMBOLS = ("flowse_stft_compress_chunks", "flowse_istft_decompress_chunks", "flowse_prior_sample_keyed_at",
               "flowse_op_keyed_noise_at")


@pytest.mark.parametrize("Tc,To", GEOMETRIES, ids=lambda v: str(v))
def test_plan_chunks_covers_minimally_with_at_most_two_chunks_per_frame(Tc, To):
    from flowmse_amd.chunked import plan_chunks
    for T in range(1, 2001):
        K, hop, Tg = plan_chunks(T, Tc, To)
        assert hop == Tc - To and K >= 1 and Tg == (K - 1) * hop + Tc
        assert (K == 1) == (T <= Tc)
        cover = np.zeros(Tg, dtype=np.int64)
        for k in range(K):
            cover[k * hop:k * hop + Tc] += 1
        assert cover[:T].min() >= 1, (T, "a real frame lies in no chunk")
        assert cover.max() <= 2, (T, "three chunks over one frame")
        assert int((cover == 2).sum()) == (K - 1) * To
        assert K == 1 or (K - 2) * hop + Tc < T, (T, K, "one chunk fewer would cover the recording")


def test_plan_chunks_defaults_and_argument_errors():
    from flowmse_amd.chunked import plan_chunks
    assert plan_chunks(7501) == (34, 224, 7648)                    # 60 s at 16 kHz
    assert plan_chunks(1251) == (6, 224, 1376)                     # 10 s
    assert plan_chunks(157, 64, 16) == (3, 48, 160)                # 20000 samples, the end-to-end case
    assert plan_chunks(256) == (1, 224, 256) and plan_chunks(257) == (2, 224, 480)
    for bad in [(0, 256, 32), (10, 0, 0), (10, 100, 32), (10, 96, 32), (10, 256, 31), (10, 256, -2), (10, 256, 130),
                (10, 64, 34), (10, -64, 0)]:
        with pytest.raises(ValueError):
            plan_chunks(*bad)
    assert plan_chunks(10, 256, 128) == (1, 128, 256)              # To == Tc / 2 is allowed


def test_keyed_noise_reference_at_offsets_is_a_slice_of_the_stream():
    from flowmse_amd.util.noise import keyed_noise_reference
    keys = [0x0123456789ABCDEF, 2 ** 64 - 1, 3]
    whole = keyed_noise_reference(keys, 11, 8, 400)
    assert np.array_equal(keyed_noise_reference(keys, 11, 8, 400, frame0=None), whole)
    assert np.array_equal(keyed_noise_reference(keys, 11, 8, 400, frame0=[0, 0, 0]), whole)
    offs = [48, 0, 336]
    got = keyed_noise_reference(keys, 11, 8, 64, frame0=offs)
    for b, o in enumerate(offs):
        assert np.array_equal(got[b], whole[b, :, :, o:o + 64]), b
    # the chunks of one recording share its key: the frames two of them share carry the same noise
    rows = keyed_noise_reference([keys[0]] * 3, 11, 8, 64, frame0=[0, 48, 96])
    assert np.array_equal(rows[0][..., 48:], rows[1][..., :16]) and np.array_equal(rows[1][..., 48:], rows[2][..., :16])
    for bad in ([1, 0, 0], [0, -2, 0], [0, 0], [0, 2, 4, 6]):
        with pytest.raises(ValueError):
            keyed_noise_reference(keys, 11, 8, 64, frame0=bad)


def test_prior_sampling_and_solver_take_frame_offsets_on_cpu_tensors():
    from flowmse_amd.odes import FLOWMATCHING
    from flowmse_amd.sampling import get_white_box_solver
    from flowmse_amd.util.noise import keyed_noise_reference
    ode = FLOWMATCHING()
    y = torch.view_as_complex(torch.randn(2, 1, 16, 64, 2, generator=torch.Generator().manual_seed(0)))
    keys, offs = [5, 5], [0, 48]
    x, z = ode.prior_sampling(y.shape, y, keys=keys, seed=9, frame0=offs)
    ref = torch.from_numpy(keyed_noise_reference(keys, 9, 16, 64, frame0=offs)).to(torch.complex64)
    assert torch.equal(z, ref) and torch.equal(x, y + ref * ode.prior_std())
    assert torch.equal(z[0][..., 48:], z[1][..., :16])
    assert torch.equal(ode.prior_sampling(y.shape, y, keys=keys, seed=9, frame0=None)[1],
                       ode.prior_sampling(y.shape, y, keys=keys, seed=9)[1])
    with pytest.raises(ValueError):
        ode.prior_sampling(y.shape, y, keys=keys, seed=9, frame0=[0, 47])
    with pytest.raises(ValueError):
        ode.prior_sampling(y.shape, y, frame0=offs)                # offsets address the keyed stream only
    # the solver passes the offsets through: a field of zeros returns the prior sample
    got, n = get_white_box_solver("euler", ode, lambda x, t, y: torch.zeros_like(x), y, N=2, noise_keys=keys, noise_seed=9,
                                  noise_frame0=offs)()
    assert n == 2 and torch.equal(got, x)
    with pytest.raises(ValueError):
        get_white_box_solver("euler", ode, lambda x, t, y: torch.zeros_like(x), y, N=2, noise_frame0=offs)()


@pytest.mark.parametrize("Tc,To", GEOMETRIES, ids=lambda v: str(v))
def test_blend_of_chunks_cut_from_one_spectrogram_returns_it_exactly(Tc, To):
    from flowmse_amd.chunked import blend_chunks_reference, plan_chunks
    g = np.random.default_rng(Tc + To)
    K, hop, Tg = plan_chunks(5 * Tc + 7, Tc, To)
    S = (g.standard_normal((1, 1, 6, Tg)) + 1j * g.standard_normal((1, 1, 6, Tg))).astype(np.complex64)
    chunks = np.concatenate([S[..., k * hop:k * hop + Tc] for k in range(K)], axis=0)
    out = blend_chunks_reference(chunks, hop)
    assert out.dtype == np.complex128 and out.shape == S.shape and np.array_equal(out, S.astype(np.complex128))
    assert np.array_equal(blend_chunks_reference(torch.from_numpy(chunks), hop), out)     # tensors are accepted too


def test_blend_weights():
    """Constant chunks make the rule visible: outside the seams a frame is its chunk's value, inside it moves from the
    previous chunk's value to this one's in To equal steps centred on the half-frames."""
    from flowmse_amd.chunked import blend_chunks_reference
    Tc, To = 64, 16
    hop = Tc - To
    chunks = np.stack([np.full((1, 2, Tc), v, dtype=np.complex64) for v in (1.0, 3.0 + 2.0j, -1.0)])
    out = blend_chunks_reference(chunks, hop)[0, 0, 0]
    assert out.shape == (2 * hop + Tc,)
    assert np.all(out[:hop] == 1.0) and np.all(out[hop + To:2 * hop] == 3.0 + 2.0j) and np.all(out[2 * hop + To:] == -1.0)
    w = (np.arange(To) + 0.5) / To
    assert np.allclose(out[hop:hop + To], 1.0 + w * (2.0 + 2.0j), rtol=0, atol=1e-15)
    assert np.allclose(out[2 * hop:2 * hop + To], (3.0 + 2.0j) + w * (-4.0 - 2.0j), rtol=0, atol=1e-15)
    assert w[0] == 1 / 32 and w[-1] == 31 / 32
    with pytest.raises(ValueError):
        blend_chunks_reference(chunks, 16)                          # three chunks would cover a frame


def test_cabi_declares_and_exports_chunked_calls():
    from flowmse_amd import _lib
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.flowse_abi_version() == 3
    assert re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)


def test_enhance_long_rejects_bad_arguments_before_any_device_call():
    import types
    from flowmse_amd.chunked import enhance_long
    from flowmse_amd.data_module import SpecTransform
    model = types.SimpleNamespace(data_module=SpecTransform())     # no network: nothing may get that far
    y = torch.zeros(1, 40000)
    for kw in (dict(chunk_frames=100), dict(overlap_frames=31), dict(overlap_frames=200), dict(batch=0)):
        with pytest.raises(ValueError):
            enhance_long(model, y, **kw)
    with pytest.raises(ValueError):
        enhance_long(model, torch.zeros(2, 40000))
    with pytest.raises(ValueError):                                 # z and a key at once
        enhance_long(model, y, chunk_frames=64, overlap_frames=16, z=torch.zeros(1, 1, 256, 352, dtype=torch.complex64),
                     noise_key=1, VF_fn=lambda x, t, y: x)


def test_enhance_command_line(tmp_path, capsys):
    from flowmse_amd import enhance
    a = enhance.parse_args(["--output", "o", "--synthetic", "2"])
    assert (a.noise, a.seed, a.batch, a.chunk_frames, a.overlap_frames, a.N, a.precision, a.odesolver) == \
        ("keyed", None, 8, 256, 32, 5, "fp32", "euler")
    assert (a.reverse_starting_point, a.last_eval_point, a.synthetic_seconds) == (1.0, 0.03, [2.0])
    a = enhance.parse_args(["--input", "in", "--output", "o", "--ckpt", "m.ckpt", "--noise", "torch", "--seed", "4",
                            "--chunk_frames", "128", "--overlap_frames", "64", "--synthetic_seconds", "1,7"])
    assert (a.noise, a.seed, a.chunk_frames, a.overlap_frames, a.synthetic_seconds) == ("torch", 4, 128, 64, [1.0, 7.0])
    for bad, word in [(["--output", "o"], "--input and --ckpt"),
                      (["--output", "o", "--input", "in"], "--input and --ckpt"),
                      (["--output", "o", "--synthetic", "1", "--batch", "0"], "--batch"),
                      (["--output", "o", "--synthetic", "1", "--N", "0"], "--N"),
                      (["--output", "o", "--synthetic", "1", "--chunk_frames", "100"], "multiple of 64"),
                      (["--output", "o", "--synthetic", "1", "--overlap_frames", "33"], "even"),
                      (["--output", "o", "--synthetic", "1", "--chunk_frames", "64", "--overlap_frames", "34"], "0.."),
                      (["--synthetic", "1"], "--output"),
                      (["--output", "o", "--synthetic", "1", "--noise", "philox"], "--noise")]:
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    text = enhance.build_parser().format_help()
    assert "test_dir" not in text and "clean" in text              # no clean files, and the help says so

    # inputs: a file or a folder's *.wav sorted by name; other sample rates are refused by name
    from scipy.io import wavfile
    d = tmp_path / "in"
    d.mkdir()
    for name, sr in (("b.wav", 16000), ("a.wav", 16000), ("c_8k.wav", 8000), ("d_48k.wav", 48000)):
        wavfile.write(d / name, sr, np.zeros(100, dtype=np.int16))
    (d / "notes.txt").write_text("x")
    files = enhance.list_inputs(str(d))
    assert [os.path.basename(f) for f in files] == ["a.wav", "b.wav", "c_8k.wav", "d_48k.wav"]
    assert enhance.list_inputs(str(d / "a.wav")) == [str(d / "a.wav")]
    assert enhance.sample_rate(str(d / "c_8k.wav")) == 8000
    enhance.refuse_other_rates(files[:2])
    with pytest.raises(SystemExit) as e:
        enhance.refuse_other_rates(files)
    msg = str(e.value)
    assert "c_8k.wav (8000 Hz)" in msg and "d_48k.wav (48000 Hz)" in msg and "a.wav" not in msg
    with pytest.raises(SystemExit):
        enhance.list_inputs(str(tmp_path / "missing"))
    with pytest.raises(SystemExit):
        enhance.list_inputs(str(tmp_path))                          # a folder without wavs
