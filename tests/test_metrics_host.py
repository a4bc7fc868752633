"""CPU: the host side of the device metrics -- the ESTOI taps of the library against the numpy formula, the band table
against pystoi's ``thirdoct`` formula, the float64 restatement ``estoi_reference`` on the degenerate cases, the
``--metrics`` option of evaluate, the declared symbols, and (where a user has pystoi) the restatement against ``pystoi.stoi``.
"""
import os
import re
import types

import numpy as np
import pytest

import _metrics_cases as MC
from flowmse_amd import _lib
from flowmse_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("flowse_estoi_num_taps", "flowse_estoi_taps", "flowse_metrics_workspace_bytes", "flowse_estoi", "flowse_energy_ratios")


def test_taps_match_the_numpy_formula():
    assert _lib.lib.flowse_estoi_num_taps() == 581
    h = M.estoi_taps()
    want = M.taps_formula()
    assert h.shape == want.shape == (581,)
    assert np.max(np.abs(h - want)) <= 1e-12
    assert abs(h.sum() - 1.0) <= 1e-12 and np.array_equal(want, want[::-1])
    # written out once more, independent of the module: section 1 of the definition
    fc = 1 / 16
    half = int(np.ceil((60 - 8) / (28.714 * fc / 10)))
    assert half == 290
    t = np.arange(-half, half + 1)
    again = np.kaiser(581, 0.1102 * (60 - 8.7)) * 2 * 5 * fc * np.sinc(2 * fc * t)
    assert np.max(np.abs(h - again / again.sum())) <= 1e-12
    small = np.empty(580)
    import ctypes as C
    assert _lib.lib.flowse_estoi_taps(small.ctypes.data_as(C.POINTER(C.c_double)), 580) == 1
    assert _lib.lib.flowse_estoi_taps(None, 581) == 1 and b"flowse_estoi_taps" in _lib.lib.flowse_last_error()


def test_band_table_matches_the_thirdoct_formula():
    """pystoi's thirdoct(10000, 512, 15, 150): centre 150 2^(k/3), edges 150 2^((2k -+ 1)/6), nearest bin of
    linspace(0, 10000, 513)[:257]."""
    f = np.linspace(0, 10000, 513)[:257]
    k = np.arange(15, dtype=np.float64)
    lo = 150.0 * 2.0 ** ((2 * k - 1) / 6)
    hi = 150.0 * 2.0 ** ((2 * k + 1) / 6)
    bands = tuple((int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi))
    assert bands == M.BANDS
    assert M.BANDS[0][0] == 7 and M.BANDS[-1][1] == 219 and all(a[1] == b[0] for a, b in zip(M.BANDS, M.BANDS[1:]))


def test_reference_identical_signals_and_degenerate_cases():
    x, y = MC.signals(1)
    st = M.reference_stages(x, y)
    assert (len(st["energies"]), st["kept"], st["frames"]) == MC.EXPECT[1]
    assert abs(st["d"] - 0.577759) < 5e-7                          # the figure the definition's author measured for this signal
    assert abs(M.estoi_reference(*MC.signals(2)) - 0.539282) < 5e-7
    assert abs(M.estoi_reference(x, x) - 1.0) <= 1e-12
    for case in (4, 7):
        xs, ys = MC.signals(case)
        st = M.reference_stages(xs, ys)
        assert (len(st["energies"]), st["kept"], st["frames"]) == MC.EXPECT[case]
        assert st["d"] == 1e-5 and st["frames"] < 30
    assert M.estoi_reference(np.zeros(300, np.float32), np.ones(300, np.float32)) == 1e-5    # L10 <= 256: no frame at all
    x9, y9 = MC.signals(9)
    st = M.reference_stages(x9, y9)
    assert st["d"] == 0.0 and st["kept"] == len(st["energies"]) and st["frames"] >= 30
    with pytest.raises(ValueError, match="8000"):
        M.estoi_reference(x, y, sr=8000)
    with pytest.raises(ValueError):
        M.estoi_reference(x, y[:-1])


def test_reference_exclusive_frame_range():
    """Case 6: L10 = 5376, L10 - 256 a multiple of 128: ``range(0, L10 - 256, 128)`` stops one frame short of the last full
    one, in the first pass and (the rebuilt length has the same form) in the second, for both signals alike."""
    x, y = MC.signals(6)
    st = M.reference_stages(x, y)
    assert st["L10"] == 5376 and (st["L10"] - 256) % 128 == 0
    assert len(st["energies"]) == (st["L10"] - 256) // 128 == 40    # not 41
    assert (st["kept"], st["frames"]) == (40, 39)
    assert 0.0 < st["d"] < 1.0
    # one more sample at 10 kHz and the last full frame is there
    x2, y2 = MC.sig(8602, 7)
    st2 = M.reference_stages(x2, y2)
    assert st2["L10"] == 5377 and len(st2["energies"]) == 41


def test_parser_metrics_option_and_host_settings_file(tmp_path):
    from flowmse_amd import evaluate as E
    base = ["--folder_destination", str(tmp_path)]
    assert E.parse_args(base).metrics == "host"
    assert E.parse_args(base + ["--metrics", "host"]).metrics == "host"
    assert E.parse_args(base + ["--metrics", "device"]).metrics == "device"
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--metrics", "gpu"])
    model = types.SimpleNamespace(ode=types.SimpleNamespace(sigma_min=0.0, sigma_max=0.487))
    data = {c: [] for c in E._COLUMNS}
    texts = {}
    for tag in ("host", "device"):
        out = tmp_path / tag
        out.mkdir()
        E._write_reports(str(out), data, E.parse_args(base + ["--metrics", tag]), model, "n/a", None)
        texts[tag] = (out / "_settings.txt").read_text()
    assert "metrics" not in texts["host"] and texts["host"].endswith("gpus: 1\n")
    assert texts["device"] == texts["host"] + "metrics: device\n"


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in flowse_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "metrics.hip" in __import__("flowmse_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.lib.flowse_abi_version() == 3                      # additive entries: the version stays
    assert "pystoi" in header and "NOT been checked" in header     # the caveat travels with the declaration
    assert "NOT BEEN CHECKED" in M.__doc__


def test_restatement_against_pystoi():
    """Equality with pystoi cannot be checked where the package is absent: this test skips there and tells a user who has
    it whether the float64 restatement matches ``pystoi.stoi(x, y, 16000, extended=True)``."""
    pystoi = pytest.importorskip("pystoi")
    for case in (1, 2):
        x, y = MC.signals(case)
        want = pystoi.stoi(x.astype(np.float64), y.astype(np.float64), 16000, extended=True)
        assert abs(M.estoi_reference(x, y) - want) <= 1e-9, (case, want)
