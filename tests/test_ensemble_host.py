"""CPU: ensembles of draws (``flowmse_amd.ensemble``) -- the plan with the draw as a fourth row coordinate, the draw keys, the
float64 reference of the mean and the agreement tracks, the ``--samples`` command lines and the C-ABI surface of
``flowse_istft_decompress_ensemble`` (no GPU compute calls)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flowse_istft_decompress_ensemble"
MIXED = [("a.wav", 1, 64000), ("b.wav", 2, 12000), ("c.wav", 3, 5000), ("d.wav", 1, 20000), ("e.wav", 2, 300)]   # K = 11, 2, 1, 3, 1
ERR_ARG, ERR_SHAPE = 1, 4


def _parent_plan(items, batch, Tc, To):
    """The rule of ``plan_pool`` before it knew draws, restated: rows (item, channel, chunk, frame0, filler)."""
    from flowmse_amd.chunked import plan_chunks
    buckets = {}
    for i, (_, C, L) in enumerate(items):
        T = L // 128 + 1
        K, hop, _ = plan_chunks(T, Tc, To)
        width = Tc if K > 1 else -(-T // 64) * 64
        buckets.setdefault(width, []).extend((i, c, k, k * (hop if K > 1 else width), False) for c in range(C) for k in range(K))
    calls = []
    for width in sorted(buckets):
        rows = buckets[width]
        for r0 in range(0, len(rows), batch):
            group = rows[r0:r0 + batch]
            calls.append((width, group + [group[0][:4] + (True,)] * (batch - len(group))))
    return calls


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("draws", [(0, 1, 2), (5, 0), (3,)])
def test_plan_pool_with_draws(batch, draws):
    from flowmse_amd.chunked import plan_chunks
    from flowmse_amd.pooled import plan_pool
    D = len(draws)
    calls = plan_pool(MIXED, batch, 64, 16, draws=draws)
    Ks = [plan_chunks(L // 128 + 1, 64, 16)[0] for _, _, L in MIXED]
    real = [r for c in calls for r in c.rows if not r.filler]
    assert len(real) == sum(C * D * K for (_, C, _), K in zip(MIXED, Ks))
    for call in calls:
        assert len(call.rows) == batch
        fillers = [r for r in call.rows if r.filler]
        assert all(not r.filler for r in call.rows[:batch - len(fillers)]) and len(fillers) < batch
        assert all(r == call.rows[0]._replace(filler=True) for r in fillers)
    for i, ((_, C, _), K) in enumerate(zip(MIXED, Ks)):
        mine = [(r.channel, r.draw, r.chunk) for r in real if r.item == i]
        assert mine == [(c, d, k) for c in range(C) for d in draws for k in range(K)], i
        hop = 48 if K > 1 else None
        assert all(r.frame0 == (r.chunk * hop if hop else 0) for r in real if r.item == i)
    # a file's rows are consecutive within its bucket, so at most `batch` files are open at any call
    for width in {c.width for c in calls}:
        items = [r.item for c in calls if c.width == width for r in c.rows if not r.filler]
        assert items == sorted(items)


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_plan_pool_draw_zero_is_the_plan_without_draws(batch):
    from flowmse_amd.pooled import plan_pool
    for Tc, To in ((64, 16), (128, 32)):
        with_arg = plan_pool(MIXED, batch, Tc, To, draws=(0,))
        assert with_arg == plan_pool(MIXED, batch, Tc, To)
        assert [(c.width, [tuple(r)[:5] for r in c.rows]) for c in with_arg] == _parent_plan(MIXED, batch, Tc, To)
        assert all(r.draw == 0 for c in with_arg for r in c.rows)


def test_plan_pool_refuses_bad_draws():
    from flowmse_amd.pooled import enhance_pooled, plan_pool
    for bad in ((0, 0), (1, 2, 1), (-1,), (0, -3), (), tuple(range(65))):
        with pytest.raises(ValueError, match="draws"):
            plan_pool(MIXED, 3, 64, 16, draws=bad)
        with pytest.raises(ValueError, match="draws"):
            enhance_pooled(None, None, MIXED, None, batch=3, chunk_frames=64, overlap_frames=16, draws=bad)


# ---------------------------------------------------------------------------------------------------- 2
def test_draw_keys():
    from flowmse_amd.ensemble import draw_keys
    from flowmse_amd.pooled import channel_key
    from flowmse_amd.util.noise import draw_key, utterance_key
    k = utterance_key("p232_001.wav")
    assert draw_key(k, 0) == k and draw_keys(k, (0,)) == [k]
    keys = [key for c in range(3) for key in draw_keys(channel_key("p232_001.wav", c), range(64))]
    assert len(set(keys)) == 3 * 64 and all(0 <= v < 2 ** 64 for v in keys)
    assert draw_keys(k, (2, 0)) == [draw_key(k, 2), k]


# ---------------------------------------------------------------------------------------------------- 3
def _rows(seed, n, Tc=64, std=0.1):
    from flowmse_amd.util import synth
    return synth.synth_spectrogram(seed, n, 256, Tc, std).astype(np.complex128)


def _composition(chunks, hop, length, scale):
    from flowmse_amd.chunked import blend_chunks_reference
    from flowmse_amd.data_module import SpecTransform
    st = SpecTransform()
    Z = st.spec_back(torch.from_numpy(blend_chunks_reference(chunks, hop)[0, 0]))
    w = torch.hann_window(510, periodic=True, dtype=torch.float64)
    return Z.numpy(), torch.istft(Z, n_fft=510, hop_length=128, window=w, center=True, length=length).numpy() * scale


def test_reference_with_one_draw_is_the_existing_composition():
    from flowmse_amd.ensemble import ensemble_reference
    c = _rows(1, 6)                                                 # 2 stacks of 3 chunks, Tg = 160
    for length in (19200, 20607, 5000):
        wave, tracks = ensemble_reference(c, 2, 1, 48, length, 0.7)
        assert tracks is None and wave.shape == (2, length) and wave.dtype == np.float64
        for s in range(2):
            assert np.array_equal(wave[s], _composition(c[3 * s:3 * s + 3], 48, length, 0.7)[1])


def test_reference_mean_tracks_and_agreement():
    from flowmse_amd.ensemble import agreement_db, agreements, ensemble_reference
    c = _rows(2, 3)
    Z, _ = _composition(c, 48, 1000, 1.0)
    # identical draws: the mean is the draw, no deviation, infinite agreement
    # (four of them: z + z + z + z and the division by 4 are exact, which a division by 3 is not)
    wave, tracks = ensemble_reference(np.concatenate([c, c, c, c]), 1, 4, 48, 19200)
    assert tracks.shape == (1, 2, 160) and np.all(tracks[0, 0] == 0.0)
    assert np.allclose(tracks[0, 1], (np.abs(Z) ** 2).sum(axis=0), rtol=1e-12)
    assert agreement_db(tracks[0, 0], tracks[0, 1], 19200) == math.inf
    assert np.allclose(wave, ensemble_reference(c, 1, 1, 48, 19200)[0], rtol=0, atol=1e-12)
    # Z and -Z (spec_back keeps the phase, so negating the compressed rows negates Z): the mean is zero
    wave, tracks = ensemble_reference(np.concatenate([c, -c]), 1, 2, 48, 19200)
    power = (np.abs(Z) ** 2).sum(axis=0)
    assert np.abs(wave).max() <= 1e-12 * np.abs(_composition(c, 48, 19200, 1.0)[1]).max()
    assert np.all(tracks[0, 1] <= 1e-24 * power)                    # to the rounding of the phase of -z
    assert np.allclose(tracks[0, 0], 2 * power, rtol=1e-12)         # 2 |Z|^2 / (2 - 1)
    assert agreement_db(tracks[0, 0], tracks[0, 1], 19200) < -240.0
    assert agreement_db(np.ones(160), np.zeros(160), 19200) == -math.inf
    # two independent draws, both layouts: [S][D][K] against rows ordered (draw, stack) with K = 1
    one = _rows(3, 6)
    wave, tracks = ensemble_reference(one, 3, 2, 64, 8000)
    perm = np.stack([one[2 * s + d] for d in range(2) for s in range(3)])
    wave2, tracks2 = ensemble_reference(perm, 3, 2, 64, 8000, stack_stride=1, draw_stride=3)
    assert np.array_equal(wave, wave2) and np.array_equal(tracks, tracks2) and tracks.shape == (3, 2, 64)
    Z0, Z1 = (_composition(one[r:r + 1], 64, 8000, 1.0)[0] for r in (0, 1))
    M = (Z0 + Z1) / 2
    assert np.allclose(tracks[0, 0], (np.abs(Z0 - M) ** 2 + np.abs(Z1 - M) ** 2).sum(axis=0), rtol=1e-12)
    # the agreement counts the real frames only: 8000 samples = 63 of the 64 frames
    want = 10 * math.log10(tracks[0, 1, :63].sum() / tracks[0, 0, :63].sum())
    assert agreement_db(tracks[0, 0], tracks[0, 1], 8000) == pytest.approx(want, abs=1e-12)
    assert agreements(torch.from_numpy(tracks), 8000)[0] == pytest.approx(want, abs=1e-12)
    assert abs(want - 10 * math.log10(1 / 2)) < 1.0                 # independent draws of equal power: |M|^2 is half a draw's
    with pytest.raises(ValueError):
        ensemble_reference(one, 3, 2, 64, 8000, stack_stride=4, draw_stride=1)               # reads past the rows


# ---------------------------------------------------------------------------------------------------- 4
def test_samples_command_lines(capsys):
    from flowmse_amd import enhance, evaluate
    en, ev = ["--output", "o", "--synthetic", "2"], ["--folder_destination", "o", "--synthetic", "2"]
    for bad, words in [(lambda: enhance.parse_args(en + ["--samples", "2"]), ("--samples", "--pool")),
                       (lambda: enhance.parse_args(en + ["--pool", "--samples", "65"]), ("--samples", "1..64")),
                       (lambda: enhance.parse_args(en + ["--pool", "--samples", "0"]), ("--samples", "1..64")),
                       (lambda: evaluate.parse_args(ev + ["--samples", "2", "--noise", "torch"]), ("--samples", "--noise keyed")),
                       (lambda: evaluate.parse_args(ev + ["--batch", "8", "--samples", "16"]), ("--batch", "--samples", "64")),
                       (lambda: evaluate.parse_args(ev + ["--samples", "65"]), ("--samples", "1..64"))]:
        with pytest.raises(SystemExit) as e:
            bad()
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err
    # --samples 1 is not passing the flag
    for mod, base in ((enhance, en), (enhance, en + ["--pool", "--channels", "all"]), (evaluate, ev),
                      (evaluate, ev + ["--gpus", "2"]), (evaluate, ev + ["--batch", "64"])):
        a, b = vars(mod.parse_args(base)), vars(mod.parse_args(base + ["--samples", "1"]))
        assert a == b and a["samples"] == 1
    # one draw: --batch is not capped by the rows of an ensemble call, as it never was
    for extra in ([], ["--samples", "1"]):
        a = evaluate.parse_args(ev + ["--batch", "65"] + extra)
        assert (a.batch, a.samples, a.noise) == (65, 1, "torch")
        assert evaluate.parse_args(ev + ["--batch", "4096"] + extra).batch == 4096
    assert evaluate.parse_args(ev + ["--batch", "32", "--samples", "2"]).batch == 32          # 64 rows: the limit itself
    with pytest.raises(SystemExit):
        evaluate.parse_args(ev + ["--batch", "33", "--samples", "2"])
    capsys.readouterr()
    assert evaluate.parse_args(ev).noise == "torch"
    a = evaluate.parse_args(ev + ["--samples", "4", "--batch", "16"])
    assert (a.samples, a.noise) == (4, "keyed")                     # not given: the ensemble selects keyed noise
    assert enhance.parse_args(en + ["--pool", "--samples", "64"]).samples == 64


def test_the_command_lines_parse_without_loading_the_library():
    """``import flowmse_amd.evaluate`` and its parser (``--help``, ``parse_args``) do not open ``libflowse_hip.so``: the
    ensemble module they import restates ``FLOWSE_MAX_DRAWS`` instead of importing it.  A fresh interpreter, host only."""
    import subprocess
    import sys
    code = ("import sys; from flowmse_amd import evaluate; "
            "a = evaluate.parse_args(['--folder_destination', 'o', '--synthetic', '1', '--samples', '2']); "
            "assert a.samples == 2 and 'flowmse_amd.ensemble' in sys.modules; "
            "assert 'flowmse_amd._lib' not in sys.modules, 'the parser loaded the library'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    from flowmse_amd import _lib, ensemble
    assert ensemble.MAX_DRAWS == _lib.FLOWSE_MAX_DRAWS == 64


# ---------------------------------------------------------------------------------------------------- 5
def test_cabi_declares_exports_and_checks_the_ensemble_call():
    from flowmse_amd import _lib
    text = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header)
    assert NAME in _lib.SIGNATURES and hasattr(_lib.lib, NAME)
    assert _lib.lib.flowse_abi_version() == 3 and re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)
    assert re.search(r"#define\s+FLOWSE_MAX_DRAWS\s+64\b", header) and _lib.FLOWSE_MAX_DRAWS == 64
    # argument errors are answered before any device call: host memory stands in for the device buffers
    rows, out, tracks = (ctypes.create_string_buffer(8) for _ in range(3))
    fn = getattr(_lib.lib, NAME)

    def call(S=2, D=3, K=3, Tc=64, hop=48, ss=9, ds=3, Lout=1000, tr=None, chunks=rows, dst=out, factor=0.15):
        return fn(chunks, S, D, K, Tc, hop, ss, ds, factor, 0.5, dst, Lout, 1.0, tr, None)

    for kw, words in [(dict(D=0), (b"D=0",)), (dict(D=65), (b"D=65",)), (dict(D=1, tr=tracks), (b"D=1", b"tracks")),
                      (dict(ss=8), (b"alias", b"stack_stride=8")),                      # stacks overlap by one row
                      (dict(ds=2), (b"alias", b"draw_stride=2")),                       # draws overlap by one row
                      (dict(ss=3, ds=3), (b"alias",)), (dict(ss=-9), (b"alias",)), (dict(ds=0), (b"alias",)),
                      (dict(K=1, Tc=64, hop=64, ss=1, ds=1), (b"alias",)),               # (draw, stack) order needs ds >= S
                      (dict(S=0), (b"S=0",)), (dict(hop=30), (b"hop=30",)), (dict(Lout=0), (b"Lout=0",)),
                      (dict(Lout=128 * 159 + 256), (b"Lout",)), (dict(factor=0.0), (b"factor",))]:
        assert call(**kw) == ERR_SHAPE, kw
        err = _lib.lib.flowse_last_error()
        assert b"istft ensemble" in err and all(w in err for w in words), (kw, err)
    assert call(chunks=None) == ERR_ARG and call(dst=None) == ERR_ARG
    assert NAME.encode() in _lib.lib.flowse_last_error()


def test_synthesize_ensemble_rejects_bad_arguments_before_any_device_call():
    from flowmse_amd.data_module import SpecTransform
    dm, c = SpecTransform(), torch.zeros(6, 1, 256, 64, dtype=torch.complex64)
    for args, kw in [((4, 1, 48, 1000), {}), ((2, 2, 48, 1000), {}), ((0, 1, 48, 1000), {}), ((2, 0, 48, 1000), {}),
                     ((2, 1, 48, 1000), dict(tracks=True)), ((3, 2, 64, 1000), dict(stack_stride=2, draw_stride=3)),
                     ((1, 2, 64, 1000), dict(K=1, draw_stride=6)), ((3, 2, 64, 1000), dict(stack_stride=-1, draw_stride=3))]:
        with pytest.raises(ValueError, match="synthesize_ensemble"):
            dm.synthesize_ensemble(c, *args, **kw)
