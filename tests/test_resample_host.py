"""CPU: the sample-rate converter's host side -- the taps from ``flowse_resample_taps`` against scipy's ``firwin``, the
float64 restatement ``resample_reference`` against ``scipy.signal.resample_poly``, ratio reduction, the C entries' argument
checks and the ``--resample`` options of the ``flowmse_amd.enhance`` command line (no GPU compute calls)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = 1, 4
TOL = 1e-12                      # two double evaluations of one closed form (taps: only the I0 series differs)
RATE_CASES = [(48000, 16000, 1000), (44100, 16000, 1327), (22050, 16000, 700), (8000, 16000, 333), (16000, 48000, 257),
              (16000, 44100, 320)]
EDGE_CASES = [(a, b, n) for a, b, _ in RATE_CASES for n in (5, 1)]             # every tap hangs over an edge


def _firwin_taps(up, down):
    from scipy.signal import firwin
    R = max(up, down)
    return up * firwin(20 * R + 1, 1.0 / R, window=("kaiser", 5.0))


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (441, 160), (2, 1), (320, 441), (1, 12)])
def test_design_taps_match_firwin(up, down):
    from flowmse_amd import _lib
    from flowmse_amd.resample import design_taps
    want = _firwin_taps(up, down)
    got = design_taps(up, down)
    assert got.dtype == np.float64 and got.shape == want.shape == (20 * max(up, down) + 1,)
    assert _lib.lib.flowse_resample_num_taps(up, down) == 20 * max(up, down) + 1
    err = float(np.abs(got - want).max())
    print(f"taps {up}/{down}: max |library - firwin| = {err:.3e}")
    assert err <= TOL
    assert abs(got.sum() - up) <= 1e-9 and np.array_equal(got, got[::-1])          # unit DC gain times up; symmetric


def test_unreduced_pair_gives_the_reduced_taps():
    from flowmse_amd import _lib
    from flowmse_amd.resample import design_taps
    assert np.array_equal(design_taps(16000, 48000), design_taps(1, 3))
    assert np.array_equal(design_taps(32000, 88200), design_taps(160, 441))
    assert _lib.lib.flowse_resample_num_taps(16000, 48000) == 61
    assert _lib.lib.flowse_resample_num_taps(16000, 44100) == 8821
    assert _lib.lib.flowse_resample_num_taps(1, 1024) == 20481


@pytest.mark.parametrize("sr_in,sr_out,n", RATE_CASES + EDGE_CASES, ids=lambda v: str(v))
def test_reference_matches_scipy_resample_poly(sr_in, sr_out, n):
    from scipy.signal import resample_poly
    from flowmse_amd.resample import out_len, rational, resample_reference
    up, down = rational(sr_in, sr_out)
    x = np.random.default_rng(sr_in + sr_out + n).standard_normal(n)
    want = resample_poly(x, up, down)
    got = resample_reference(x, sr_in, sr_out)
    assert got.dtype == np.float64 and got.shape == want.shape == (out_len(n, up, down),)
    err = float(np.abs(got - want).max())
    print(f"{sr_in} -> {sr_out}, L = {n}: max |reference - resample_poly| = {err:.3e}")
    assert err <= TOL
    # a window of outputs equals that slice of the full result exactly
    n0, n1 = got.shape[0] // 3, min(got.shape[0], got.shape[0] // 3 + 77)
    assert np.array_equal(resample_reference(x, sr_in, sr_out, n0, n1), got[n0:n1])
    assert resample_reference(x, sr_in, sr_out, n1, n1).shape == (0,)


def test_reference_window_from_the_input_slice_it_touches():
    """The far end of a signal from the last samples only: ``m0`` places the slice, whose first sample is the first one
    the window's outputs touch (q - (P - 1) of the first output)."""
    from flowmse_amd.resample import rational, resample_reference
    x = np.random.default_rng(5).standard_normal(30000)
    full = resample_reference(x, 44100, 16000)
    up, down = rational(44100, 16000)
    half, P = 10 * down, -(-(20 * down + 1) // up)
    n1 = full.shape[0]
    n0 = n1 - 500
    q0 = (half + n0 * down) // up - (P - 1)
    assert 0 < q0 < 30000 and P == 56
    assert np.array_equal(resample_reference(x[q0:], 44100, 16000, n0, n1, m0=q0), full[n0:])
    with pytest.raises(ValueError):
        resample_reference(x, 44100, 16000, 0, n1 + 1)
    with pytest.raises(ValueError):
        resample_reference(x[None], 44100, 16000)


def test_rational_and_out_len():
    from flowmse_amd.resample import out_len, rational
    assert rational(44100, 16000) == (160, 441)
    assert rational(16000, 16000) == (1, 1)
    assert rational(16000, 48000) == (3, 1) and rational(8000, 16000) == (2, 1) and rational(88200, 16000) == (80, 441)
    for sr in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        assert max(rational(sr, 16000)) <= 1024 and rational(16000, sr) == rational(sr, 16000)[::-1]
    with pytest.raises(ValueError) as e:
        rational(16001, 16000)
    assert "16001" in str(e.value) and "16000" in str(e.value)
    for bad in ((0, 16000), (16000, 0), (-1, 16000)):
        with pytest.raises(ValueError):
            rational(*bad)
    assert out_len(1000, 1, 3) == 334 and out_len(999, 1, 3) == 333 and out_len(1, 160, 441) == 1
    assert out_len(14_000_000, 160, 441) == 5_079_366             # past 2^31 / 441 outputs


def test_c_entries_refuse_bad_arguments_with_a_message():
    from flowmse_amd import _lib
    L = _lib.lib
    buf = (C.c_double * 61)()
    assert L.flowse_resample_taps(1, 3, buf, 61) == 0
    for args, rc in [((1, 1025), ERR_SHAPE), ((16001, 16000), ERR_SHAPE), ((0, 3), ERR_ARG), ((3, 0), ERR_ARG),
                     ((-2, 3), ERR_ARG)]:
        assert L.flowse_resample_num_taps(*args) == -rc, args
        assert len(L.flowse_last_error()) > 0 and b"flowse_resample_num_taps" in L.flowse_last_error()
        assert L.flowse_resample_taps(*args, buf, 61) == rc, args
        assert b"flowse_resample_taps" in L.flowse_last_error()
    assert L.flowse_resample_taps(1, 3, buf, 60) == ERR_ARG                          # a short cap
    assert b"61 taps" in L.flowse_last_error()
    assert L.flowse_resample_taps(1, 3, None, 61) == ERR_ARG
    assert L.flowse_resample_num_taps(2048, 2048) == 21                              # reduced before the limit applies
    # the device entry checks its arguments before any device call
    assert L.flowse_resample_poly(None, 1, 100, 1, 3, None, 34, None) == ERR_ARG
    assert L.flowse_resample_poly(C.c_void_p(256), 1, 100, 1, 1025, C.c_void_p(256), 1, None) == ERR_SHAPE
    assert L.flowse_resample_poly(C.c_void_p(256), 1, 100, 1, 3, C.c_void_p(256), 33, None) == ERR_SHAPE
    assert b"34" in L.flowse_last_error()
    assert L.flowse_resample_poly(C.c_void_p(256), 0, 100, 1, 3, C.c_void_p(256), 34, None) == ERR_ARG


def test_cabi_declares_and_exports_the_resampler():
    from flowmse_amd import _lib
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("flowse_resample_num_taps", "flowse_resample_taps", "flowse_resample_poly"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.flowse_abi_version() == 3
    assert re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)


def test_resample_on_cpu_tensors():
    from flowmse_amd.resample import resample, resample_reference
    x = torch.randn(3, 441, generator=torch.Generator().manual_seed(1))
    assert resample(x, 16000, 16000) is x
    assert resample(x, 48000, 48000) is x
    y = resample(x, 44100, 16000)
    assert y.dtype == torch.float32 and y.shape == (3, 160)
    for b in range(3):
        assert np.array_equal(y[b].numpy(), resample_reference(x[b].numpy(), 44100, 16000).astype(np.float32))
    with pytest.raises(ValueError):
        resample(x, 16001, 16000)
    with pytest.raises(ValueError):
        resample(x[0], 44100, 16000)
    with pytest.raises(ValueError):
        resample(x.double(), 44100, 16000)


def test_enhance_command_line_resample_options(tmp_path, capsys):
    from scipy.io import wavfile
    from flowmse_amd import enhance
    a = enhance.parse_args(["--output", "o", "--synthetic", "1"])
    assert (a.resample, a.output_rate, a.synthetic_rate) == (False, "16000", 16000)
    a = enhance.parse_args(["--output", "o", "--synthetic", "1", "--resample", "--output_rate", "input",
                            "--synthetic_rate", "44100"])
    assert (a.resample, a.output_rate, a.synthetic_rate) == (True, "input", 44100)
    for bad, word in [(["--output", "o", "--synthetic", "1", "--output_rate", "input"], "needs --resample"),
                      (["--output", "o", "--synthetic", "1", "--synthetic_rate", "48000"], "needs --resample"),
                      (["--output", "o", "--synthetic", "1", "--resample", "--synthetic_rate", "16001"], "16001"),
                      (["--output", "o", "--synthetic", "1", "--resample", "--output_rate", "44100"], "--output_rate")]:
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    text = " ".join(enhance.build_parser().format_help().split())
    assert "--resample" in text and "nothing above 8 kHz" in text
    assert "NOTHING above 8 kHz" in " ".join(enhance.__doc__.split())

    d = tmp_path / "in"
    d.mkdir()
    for name, sr in (("a_8k.wav", 8000), ("b.wav", 16000), ("c_44k.wav", 44100), ("d_48k.wav", 48000)):
        wavfile.write(d / name, sr, np.zeros(100, dtype=np.int16))
    files = enhance.list_inputs(str(d))
    assert enhance.resampling_rates(files) == [8000, 16000, 44100, 48000]
    wavfile.write(d / "e_odd.wav", 16001, np.zeros(100, dtype=np.int16))
    files = enhance.list_inputs(str(d))
    with pytest.raises(SystemExit) as e:
        enhance.resampling_rates(files)
    msg = str(e.value)
    assert "e_odd.wav (16001 Hz)" in msg and "16000 Hz" in msg and "c_44k.wav" not in msg and "b.wav" not in msg
    # without the flag the refusal is what it was
    with pytest.raises(SystemExit) as e:
        enhance.refuse_other_rates(files)
    msg = str(e.value)
    assert msg.startswith("not 16 kHz (resample first): ") and "a_8k.wav (8000 Hz)" in msg and "e_odd.wav (16001 Hz)" in msg
    assert "b.wav" not in msg
    enhance.refuse_other_rates([str(d / "b.wav")])
