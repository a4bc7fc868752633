"""CPU: the schedule of ``flowmse_amd.live`` against its plain definition, the latency formula, the ``--live`` command line,
the PCM conversions and the C-ABI surface of the two window entries (no GPU compute calls)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(64, 0), (64, 16), (128, 64), (256, 32)]
NEW_SYMBOLS = ("flowse_stft_compress_window", "flowse_istft_decompress_window")


def _ready_at(k, Tc, hop):
    """n_k from the frame definition: the last frame of chunk k, k hop + Tc - 1, reads samples up to 128 t + 254."""
    return 128 * (k * hop + Tc - 1) + 254 + 1


def _final_samples(frames_final, n_frames, n_samples):
    """The largest e such that every frame over every sample < e is final: frame t lies over the output samples
    [128 t - 255, 128 t + 254]; frames >= frames_final are not final."""
    waiting = np.zeros(n_samples, dtype=bool)
    for t in range(frames_final, n_frames):
        waiting[max(128 * t - 255, 0):max(128 * t + 255, 0)] = True
    hit = np.flatnonzero(waiting)
    return int(hit[0]) if hit.size else n_samples


@pytest.mark.parametrize("Tc,To", GEOMETRIES, ids=lambda v: str(v))
def test_live_plan_against_the_plain_definition(Tc, To):
    from flowmse_amd.chunked import plan_chunks
    from flowmse_amd.live import live_plan
    hop = Tc - To
    n_max = _ready_at(4, Tc, hop) + 300                            # spans chunks 0..4
    n_frames = n_max // 128 + 8
    final_of = {r: _final_samples(r * hop, n_frames, 128 * n_frames) for r in range(6)}
    assert final_of[0] == 0
    last = (0, 0)
    seen = set()
    for n in list(range(0, n_max, 37)) + [_ready_at(k, Tc, hop) + d for k in range(5) for d in (-1, 0, 1)]:
        ready = sum(1 for k in range(8) if n >= _ready_at(k, Tc, hop))
        got = live_plan(n, Tc, To)
        assert got == (ready, final_of[ready]), (n, got, ready)
        seen.add(ready)
        assert live_plan(n, Tc, To, finished=True) == (plan_chunks(n // 128 + 1, Tc, To)[0], n)
    assert seen == {0, 1, 2, 3, 4, 5}
    ns = sorted(set(range(0, n_max, 37)))
    for n in ns:
        got = live_plan(n, Tc, To)
        assert got[0] >= last[0] and got[1] >= last[1] and got[1] <= n
        last = got
    fin = [live_plan(n, Tc, To, finished=True) for n in ns]
    assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(fin, fin[1:]))
    # what is final while the recording is open stays within what is final once it has ended
    assert all(live_plan(n, Tc, To)[0] <= live_plan(n, Tc, To, finished=True)[0] for n in ns)


@pytest.mark.parametrize("Tc,To", GEOMETRIES, ids=lambda v: str(v))
def test_latency_formula_is_the_worst_wait_of_the_plan(Tc, To):
    from flowmse_amd.live import latency_samples, live_plan
    hop = Tc - To
    waits = []
    for k in range(6):
        n_k = _ready_at(k, Tc, hop)
        assert live_plan(n_k - 1, Tc, To)[0] == k and live_plan(n_k, Tc, To)[0] == k + 1
        waits.append(n_k - live_plan(n_k - 1, Tc, To)[1])          # the oldest sample not yet returned when chunk k runs
    assert max(waits) == latency_samples(Tc) == 128 * Tc + 382
    assert waits[1:] == [128 * Tc + 382] * 5 and waits[0] == 128 * Tc + 127
    assert (latency_samples(256), latency_samples(64)) == (33150, 8574)      # 2.07 s and 0.54 s at 16 kHz


def test_live_plan_argument_errors_are_plan_chunks():
    from flowmse_amd.live import live_plan
    for bad in [(100, 100, 32), (100, 256, 31), (100, 256, 130), (100, 0, 0)]:
        with pytest.raises(ValueError, match="plan_chunks"):
            live_plan(*bad)
    with pytest.raises(ValueError):
        live_plan(-1, 64, 16)
    assert live_plan(0, 64, 16) == (0, 0)


def test_live_command_line(capsys):
    from flowmse_amd import enhance
    a = enhance.parse_args(["--live", "--ckpt", "m.ckpt"])
    assert (a.live, a.live_pcm, a.live_block, a.live_norm, a.noise, a.chunk_frames, a.overlap_frames, a.N) == \
        (True, "s16le", 2048, "first", "keyed", 256, 32, 5)
    a = enhance.parse_args(["--live", "--synthetic", "1", "--live_pcm", "f32le", "--live_block", "1000", "--live_norm", "0.5",
                            "--seed", "3", "--chunk_frames", "64", "--overlap_frames", "16", "--odesolver", "heun",
                            "--precision", "bf16", "--N", "2", "--reverse_starting_point", "0.9", "--last_eval_point", "0.05"])
    assert (a.live_pcm, a.live_block, a.live_norm, a.seed, a.chunk_frames, a.overlap_frames) == ("f32le", 1000, 0.5, 3, 64, 16)
    assert (a.odesolver, a.precision, a.N, a.reverse_starting_point, a.last_eval_point) == ("heun", "bf16", 2, 0.9, 0.05)
    live = ["--live", "--ckpt", "m.ckpt"]
    for extra, word in [(["--input", "in"], "--input"), (["--pool"], "--pool"), (["--resample"], "--resample"),
                        (["--samples", "2", "--pool"], "--pool"), (["--samples", "2"], "--samples 2"),
                        (["--channels", "all"], "--channels all"), (["--noise", "torch"], "--noise torch"),
                        (["--output", "o"], "--output"), (["--live_block", "0"], "--live_block"),
                        (["--live_norm", "0"], "--live_norm"), (["--live_norm", "loud"], "--live_norm"),
                        (["--live_pcm", "u8"], "--live_pcm"), (["--chunk_frames", "100"], "multiple of 64"),
                        (["--overlap_frames", "33"], "even"), (["--N", "0"], "--N")]:
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(live + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and word in err, (extra, err)
        if extra[0] in ("--input", "--pool", "--resample", "--samples", "--channels", "--noise", "--output"):
            assert "--live does not take" in err, (extra, err)
    with pytest.raises(SystemExit):
        enhance.parse_args(["--live"])                              # no weights named
    assert "--ckpt" in capsys.readouterr().err
    # without --live nothing moved: --output is still required, by argparse's own words
    with pytest.raises(SystemExit):
        enhance.parse_args(["--synthetic", "1"])
    assert "the following arguments are required: --output" in capsys.readouterr().err
    a = enhance.parse_args(["--output", "o", "--synthetic", "1"])
    assert a.live is False and a.output == "o"


def test_pcm_round_trip():
    from flowmse_amd.live import PCM_FORMATS, pcm_decode, pcm_encode
    assert PCM_FORMATS == {"s16le": 2, "f32le": 4}
    every = np.arange(-32768, 32768, dtype="<i2").tobytes()
    x = pcm_decode(every, "s16le")
    assert x.dtype == np.float32 and x[0] == -1.0 and x[-1] == np.float32(32767 / 32768) and x[32768] == 0.0
    assert pcm_encode(x, "s16le") == every                          # every 16-bit value comes back
    # nearest, ties to even, saturation at both ends, non-finite -> 0
    q = np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, 0.49 / 32768, 1.0, 7.0, -1.0, -1.5, np.nan],
                 dtype=np.float32)
    assert np.frombuffer(pcm_encode(q, "s16le"), dtype="<i2").tolist() == [0, 2, 2, 0, 0, 32767, 32767, -32768, -32768, 0]
    f = np.array([0.0, -0.0, 1e-30, 3.5, -np.inf, np.float32(1 / 3)], dtype=np.float32)
    assert pcm_encode(f, "f32le") == f.astype("<f4").tobytes()
    assert pcm_decode(pcm_encode(f, "f32le"), "f32le").tobytes() == f.tobytes()
    assert pcm_decode(every[:5], "s16le").shape == (2,) and pcm_decode(b"", "f32le").shape == (0,)
    assert pcm_encode(np.empty(0, dtype=np.float32), "s16le") == b""


def test_cabi_declares_and_exports_window_calls():
    from flowmse_amd import _lib
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(args) == len(decl.split(",")) and getattr(_lib.lib, name).argtypes == args
    assert _lib.lib.flowse_abi_version() == 3
    assert re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)


def test_live_enhancer_refuses_a_model_without_the_hip_kernels():
    import types
    import torch
    from flowmse_amd.data_module import SpecTransform
    from flowmse_amd.live import LiveEnhancer
    model = types.SimpleNamespace(data_module=SpecTransform(), dnn=torch.nn.Identity())
    with pytest.raises(ValueError, match="plan_chunks"):            # geometry first, and in plan_chunks' words
        LiveEnhancer(model, norm=1.0, key=1, chunk_frames=100)
    with pytest.raises(ValueError, match="key"):
        LiveEnhancer(model, norm=1.0, key=None)
    for norm in (0.0, -1.0, float("nan"), "last"):
        with pytest.raises(ValueError, match="norm"):
            LiveEnhancer(model, norm=norm, key=1)
    with pytest.raises(RuntimeError, match="HIP"):
        LiveEnhancer(model, norm=1.0, key=1)
    with pytest.raises(RuntimeError, match="HIP"):
        LiveEnhancer(model, norm=1.0, key=1, device="cpu")
