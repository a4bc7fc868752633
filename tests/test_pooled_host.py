"""CPU: the pooled mode's plan (``flowmse_amd.pooled.plan_pool``), channel keys, the multi-channel wav reader and writer,
the ``enhance --pool`` command line and the C-ABI surface of the two new spectrogram calls (no GPU compute calls)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("flowse_stft_compress_rows", "flowse_istft_decompress_stacks")

# (name, channels, samples).  At (Tc, To) = (64, 16): K = 11, 2, 1, 3, 1.
MIXED_64 = [("a.wav", 1, 64000), ("b.wav", 2, 12000), ("c.wav", 3, 5000), ("d.wav", 1, 20000), ("e.wav", 2, 300)]
# At (128, 32): widths 64, 128 (K = 1), 128 (K = 3), 64, 128 (K = 1, exactly 128 frames).
MIXED_128 = [("s.wav", 1, 5000), ("t.wav", 2, 12000), ("u.wav", 1, 40000), ("v.wav", 3, 8000), ("w.wav", 1, 128 * 127)]


def _check_plan(items, batch, Tc, To):
    from flowmse_amd.chunked import plan_chunks
    from flowmse_amd.pooled import plan_pool
    calls = plan_pool(items, batch, Tc, To)
    want = {}                                                       # (item, channel, chunk) -> (width, frame0)
    for i, (_, C, L) in enumerate(items):
        T = L // 128 + 1
        K, hop, _ = plan_chunks(T, Tc, To)
        width = Tc if K > 1 else -(-T // 64) * 64
        assert width <= Tc
        for c in range(C):
            for k in range(K):
                want[(i, c, k)] = (width, k * hop)
    seen = []
    widths = [c.width for c in calls]
    assert widths == sorted(widths), "buckets in ascending width, one after another"
    for n, call in enumerate(calls):
        assert len(call.rows) == batch
        last_of_bucket = n + 1 == len(calls) or calls[n + 1].width != call.width
        fillers = [r for r in call.rows if r.filler]
        assert len(fillers) < batch and (not fillers or last_of_bucket)
        assert all(not r.filler for r in call.rows[:batch - len(fillers)]), "fillers come last"
        for r in fillers:
            assert r == call.rows[0]._replace(filler=True)
        for r in call.rows:
            assert want[(r.item, r.channel, r.chunk)] == (call.width, r.frame0)
            if not r.filler:
                seen.append((r.item, r.channel, r.chunk))
    assert len(seen) == len(set(seen)) == len(want) and set(seen) == set(want)
    # order: within a bucket the files as listed, a file's rows (channel, chunk)
    for width in set(widths):
        rows = [(r.item, r.channel, r.chunk) for c in calls if c.width == width for r in c.rows if not r.filler]
        assert rows == sorted(rows)
    # a file is open from the call of its first row to the call of its last
    first, last = {}, {}
    for n, call in enumerate(calls):
        for r in call.rows:
            first.setdefault(r.item, n)
            last[r.item] = n
    for n in range(len(calls)):
        assert sum(1 for i in first if first[i] <= n <= last[i]) <= batch
    return calls


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_plan_pool_mixed_table(batch):
    from flowmse_amd.chunked import plan_chunks
    assert [plan_chunks(L // 128 + 1, 64, 16)[0] for _, _, L in MIXED_64] == [11, 2, 1, 3, 1]
    calls = _check_plan(MIXED_64, batch, 64, 16)
    assert {c.width for c in calls} == {64}
    rows = 11 + 2 * 2 + 3 + 3 + 2
    assert len(calls) == -(-rows // batch)
    assert [plan_chunks(L // 128 + 1, 128, 32)[0] for _, _, L in MIXED_128] == [1, 1, 3, 1, 1]
    calls = _check_plan(MIXED_128, batch, 128, 32)
    by_width = {w: sum(1 for c in calls for r in c.rows if c.width == w and not r.filler) for w in (64, 128)}
    assert by_width == {64: 1 + 3, 128: 2 + 3 + 1}                  # w.wav (K = 1, 128 frames) shares the Tc bucket
    assert len(calls) == -(-4 // batch) - (-6 // batch)


def test_plan_pool_argument_errors():
    from flowmse_amd.pooled import plan_pool
    for bad in (dict(batch=0), dict(Tc=100), dict(To=31)):
        with pytest.raises(ValueError):
            plan_pool(MIXED_64, **dict(dict(batch=3, Tc=64, To=16), **bad))
    with pytest.raises(ValueError, match="short.wav"):
        plan_pool([("short.wav", 1, 255)], 3, 64, 16)
    with pytest.raises(ValueError):
        plan_pool([("x.wav", 0, 5000)], 3, 64, 16)
    assert plan_pool([], 3, 64, 16) == []


def test_a_files_rows_do_not_depend_on_the_folder():
    from flowmse_amd.pooled import channel_key, plan_pool

    def rows_of(items, name, batch):
        i = [n for n, _, _ in items].index(name)
        return [(c.width, r.frame0, channel_key(name, r.channel), r.channel, r.chunk)
                for c in plan_pool(items, batch, 64, 16) for r in c.rows if r.item == i and not r.filler]

    other = [MIXED_64[3], MIXED_64[1], ("z.wav", 1, 9000), MIXED_64[0]]
    for batch in (1, 3, 8):
        for name in ("a.wav", "b.wav", "d.wav"):
            assert rows_of(MIXED_64, name, batch) == rows_of(other, name, batch) != []


def test_channel_keys():
    from flowmse_amd.pooled import channel_key
    from flowmse_amd.util.noise import utterance_key
    assert channel_key("p232_001.wav", 0) == utterance_key("p232_001.wav")
    assert channel_key("/some/dir/p232_001.wav", 0) == utterance_key("p232_001.wav")
    keys = [channel_key("p232_001.wav", c) for c in range(3)]
    assert len(set(keys)) == 3 and all(0 <= k < 2 ** 64 for k in keys)
    assert channel_key("p232_001.wav", 1) != channel_key("p232_002.wav", 1)
    with pytest.raises(ValueError):
        channel_key("p232_001.wav", -1)


def test_read_wav_channels(tmp_path):
    from scipy.io import wavfile
    from flowmse_amd.util.other import read_wav, read_wav_channels
    g = np.random.default_rng(0)
    stereo = g.integers(-32768, 32768, size=(500, 2), dtype=np.int16)
    stereo[0] = (-32768, 32767)
    wavfile.write(tmp_path / "stereo.wav", 16000, stereo)
    y, sr = read_wav_channels(tmp_path / "stereo.wav")
    assert sr == 16000 and y.dtype == torch.float32 and tuple(y.shape) == (2, 500) and y.is_contiguous()
    assert np.array_equal(y.numpy(), stereo.T.astype(np.float32) / 32768.0)
    assert torch.equal(y[:1], read_wav(tmp_path / "stereo.wav")[0])             # channel 0 is what read_wav keeps
    three = g.uniform(-1, 1, size=(300, 3)).astype(np.float32)
    wavfile.write(tmp_path / "three.wav", 44100, three)
    y, sr = read_wav_channels(tmp_path / "three.wav")
    assert sr == 44100 and tuple(y.shape) == (3, 300) and np.array_equal(y.numpy(), three.T)
    for name, mono in (("mono16.wav", stereo[:, 0].copy()), ("mono32.wav", three[:, 1].copy())):
        wavfile.write(tmp_path / name, 16000, mono)
        a, b = read_wav_channels(tmp_path / name), read_wav(tmp_path / name)
        assert a[1] == b[1] and a[0].dtype == b[0].dtype and tuple(a[0].shape) == (1, len(mono))
        assert a[0].numpy().tobytes() == b[0].numpy().tobytes()


def _check_write_wav(tmp_path, x):
    from scipy.io import wavfile
    from flowmse_amd.evaluate import _write_wav
    _write_wav(str(tmp_path / "three.wav"), x, 22050)
    sr, data = wavfile.read(tmp_path / "three.wav")
    assert sr == 22050 and data.dtype == np.int16 and data.shape == (400, 3)
    for c in range(3):
        _write_wav(str(tmp_path / "one.wav"), x[:, c], 22050)
        assert np.array_equal(wavfile.read(tmp_path / "one.wav")[1], data[:, c])
    return data


def test_write_wav_keeps_the_channels(tmp_path, monkeypatch):
    """``[L, C]`` input becomes a C-channel 16-bit file whose channels are what the mono writer gives for each, on both
    paths of ``_write_wav``.  The scipy path is forced by making ``import soundfile`` fail and is held to the rule its
    docstring states (float32 product, round half to even, low 16 bits); the soundfile path runs where the package is
    importable and is UNCHECKED where it is not."""
    import sys
    x = np.random.default_rng(1).uniform(-1.2, 1.2, size=(400, 3)).astype(np.float32)
    x[:4, 0] = (0.5 / 32767, 1.5 / 32767, -2.5 / 32767, 1.0)                    # halves round to even; full scale
    with monkeypatch.context() as m:
        m.setitem(sys.modules, "soundfile", None)                              # import soundfile -> ImportError
        data = _check_write_wav(tmp_path, x)
    want = np.rint(x * np.float32(32767.0)).astype(np.int64).astype(np.uint16).view(np.int16)
    assert np.array_equal(data, want)
    try:
        import soundfile  # noqa: F401
    except ImportError:
        return
    _check_write_wav(tmp_path, np.clip(x, -1.0, 1.0))                           # in range: no dependence on clipping mode


def test_pool_command_line(capsys):
    from flowmse_amd import enhance
    a = enhance.parse_args(["--output", "o", "--synthetic", "2"])
    assert (a.pool, a.channels, a.synthetic_channels) == (False, "first", [1])
    a = enhance.parse_args(["--output", "o", "--synthetic", "3", "--pool", "--channels", "all", "--synthetic_channels", "1,2,1"])
    assert (a.pool, a.channels, a.synthetic_channels, a.noise) == (True, "all", [1, 2, 1], "keyed")
    assert enhance.parse_args(["--output", "o", "--synthetic", "3", "--pool"]).channels == "first"
    for bad, words in [(["--output", "o", "--synthetic", "1", "--channels", "all"], ("--channels all", "--pool")),
                       (["--output", "o", "--synthetic", "1", "--pool", "--noise", "torch"], ("--pool", "--noise torch")),
                       (["--output", "o", "--synthetic", "1", "--pool", "--batch", "65"], ("--pool", "--batch")),
                       (["--output", "o", "--synthetic", "1", "--synthetic_channels", "0"], ("--synthetic_channels",)),
                       (["--output", "o", "--synthetic", "1", "--channels", "both"], ("--channels",))]:
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(bad)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (bad, err)


def test_synthetic_channels():
    from flowmse_amd import enhance
    from flowmse_amd.evaluate import _synthetic_pairs
    sig = enhance.synthetic_signals(3, [1.0, 0.5], [1, 3], 16000)
    pairs = _synthetic_pairs(3, seconds=[1.0, 0.5], sr=16000)
    assert [s.shape for _, s in sig] == [(1, 16000), (3, 8000), (1, 16000)]
    for (name, s), (pname, _, noisy) in zip(sig, pairs):
        assert name == pname and s.dtype == np.float32 and np.array_equal(s[0], noisy)     # channel 0: the mono signal
    s = sig[1][1]
    assert not np.array_equal(s[1], s[2]) and abs(np.corrcoef(s[1], s[2])[0, 1]) < 0.2
    for c in (1, 2):                                                # half the level
        assert 0.4 < np.sqrt(np.mean(s[c] ** 2)) / np.sqrt(np.mean(s[0] ** 2)) < 0.6


def test_wav_shape(tmp_path):
    from scipy.io import wavfile
    from flowmse_amd import enhance
    wavfile.write(tmp_path / "m.wav", 8000, np.zeros(123, dtype=np.int16))
    wavfile.write(tmp_path / "s.wav", 8000, np.zeros((77, 2), dtype=np.float32))
    assert enhance.wav_shape(str(tmp_path / "m.wav")) == (123, 1) and enhance.wav_shape(str(tmp_path / "s.wav")) == (77, 2)


def test_cabi_declares_and_exports_the_rows_and_stacks_calls():
    import ctypes
    from flowmse_amd import _lib
    text = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.flowse_abi_version() == 3
    assert re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)
    assert re.search(r"#define\s+FLOWSE_MAX_SPEC_ROWS\s+64\b", header) and _lib.FLOWSE_MAX_SPEC_ROWS == 64
    assert re.search(r"typedef\s+struct\s+flowse_spec_row\s*\{", header)
    assert ctypes.sizeof(_lib.flowse_spec_row) == 24               # 64 rows by value: 1536 bytes of the argument block
    # argument errors are answered before any device call
    out = ctypes.create_string_buffer(8)
    assert _lib.lib.flowse_stft_compress_rows(None, 1, 64, out, 0.15, 0.5, None) == 1
    rows = (_lib.flowse_spec_row * 1)()
    assert _lib.lib.flowse_stft_compress_rows(rows, 0, 64, out, 0.15, 0.5, None) == 4
    assert _lib.lib.flowse_stft_compress_rows(rows, 1, 64, out, 0.15, 0.5, None) == 1       # null sig
    assert b"stft rows" in _lib.lib.flowse_last_error()
    assert _lib.lib.flowse_istft_decompress_stacks(None, 1, 1, 64, 64, 0.15, 0.5, None, 100, 1.0, None) == 1


def test_enhance_pooled_rejects_bad_arguments_before_any_device_call():
    import types
    from flowmse_amd.data_module import SpecTransform
    from flowmse_amd.pooled import enhance_pooled
    model = types.SimpleNamespace(data_module=SpecTransform())     # no network: nothing may get that far

    def load(i):
        raise AssertionError("load() reached")

    for kw in (dict(batch=0), dict(batch=65), dict(chunk_frames=100), dict(overlap_frames=31)):
        with pytest.raises(ValueError):
            enhance_pooled(model, load, [("a.wav", 1, 5000)], None, **kw)
    with pytest.raises(ValueError):
        enhance_pooled(model, load, [("a.wav", 1, 100)], None)
