"""CPU: the evaluate front end's call plan (``plan_calls``) pinned for both noise modes, and its one driver loop (``run_calls``)
driven with stand-ins for the model, the enhance core and the loss: call order, keys, files, rows and the settings file."""
import csv
import types

import numpy as np
import pytest
from scipy.io import wavfile

from flowmse_amd import evaluate as E
from flowmse_amd.util.noise import utterance_key

LENS = [128, 256, 384, 128, 256]           # padded frames of --synthetic 5 --synthetic_seconds 1.0,2.0,3.0
SET = ["--synthetic", "5", "--synthetic_seconds", "1.0,2.0,3.0", "--seed", "7"]

# (noise, world, batch, streams) -> per rank, the calls in order; a call is a list of groups of file indices.  Computed
# with the previous commit's batches_by_length / plan_shards for LENS.
PLAN = {
    ("torch", 1, 1, 1): [[[[0]], [[1]], [[2]], [[3]], [[4]]]],
    ("torch", 1, 2, 1): [[[[2]], [[1, 4]], [[0, 3]]]],
    ("torch", 1, 1, 2): [[[[0], [1], [2], [3], [4]]]],
    ("torch", 1, 2, 2): [[[[2], [1, 4], [0, 3]]]],
    ("keyed", 1, 1, 1): [[[[2]], [[1]], [[4]], [[0]], [[3]]]],
    ("keyed", 1, 2, 1): [[[[2]], [[1, 4]], [[0, 3]]]],
    ("keyed", 1, 1, 2): [[[[2], [1], [4], [0], [3]]]],
    ("keyed", 1, 2, 2): [[[[2], [1, 4], [0, 3]]]],
    ("keyed", 2, 1, 1): [[[[2]], [[0]], [[3]]], [[[1]], [[4]]]],
    ("keyed", 2, 2, 1): [[[[2]]], [[[1, 4]], [[0, 3]]]],
}


def test_synthetic_set_has_the_pinned_lengths():
    pairs = E._synthetic_pairs(5, seconds=[1.0, 2.0, 3.0])
    assert [E._padded_frames(p[2].shape[0]) for p in pairs] == LENS


@pytest.mark.parametrize("case", sorted(PLAN), ids=lambda c: "{}-world{}-batch{}-streams{}".format(*c))
def test_plan_calls_pinned(case):
    noise, world, batch, streams = case
    for rank, want in enumerate(PLAN[case]):
        assert E.plan_calls(noise, batch, streams, LENS, world, rank) == want, rank


@pytest.mark.parametrize("noise,valid_loss", [("torch", 0), ("keyed", 0), ("keyed", 2)])
def test_run_calls_with_stand_ins(tmp_path, monkeypatch, capsys, noise, valid_loss):
    """batch 2, one stream.  The stand-in for the enhance core returns the constant (file index + 1) / 16 for every file."""
    args = E.parse_args(["--folder_destination", str(tmp_path / "out"), "--noise", noise, "--batch", "2"] + SET
                        + (["--valid_loss", str(valid_loss)] if valid_loss else []))
    model = types.SimpleNamespace(ode=types.SimpleNamespace(sigma_min=0.0, sigma_max=0.487))
    names, n_samples, load = E._sources(args)
    index_of = {load(i)[1].tobytes(): i for i in range(5)}
    calls, written = [], []

    def enhance(m, ys, groups, lanes, noise_keys=None, noise_seed=0, as_tensor=False, **solver):
        ids = [index_of[y[0].numpy().tobytes()] for y in ys]
        assert m is model and not as_tensor and all(y.device.type == "cpu" for y in ys)
        assert solver == dict(N=5, T_rev=1.0, t_eps=0.03, odesolver="euler")
        calls.append(dict(files=[[ids[j] for j in g] for g in groups], flat=ids, lanes=lanes, keys=noise_keys, seed=noise_seed))
        return [np.full(y.size(1), (i + 1) / 16, dtype=np.float32) for i, y in zip(ids, ys)]

    def valid_losses(m, waves, file_names, seed, draws, batch, device):
        assert (seed, draws, batch) == (7, valid_loss, 2)
        return [0.25 + names.index(n) for n in file_names]

    real_write = E._write_wav
    monkeypatch.setattr(E, "_enhance", enhance)
    monkeypatch.setattr(E, "_valid_losses", valid_losses)
    monkeypatch.setattr(E, "_write_wav", lambda path, x, sr=16000: (written.append(path), real_write(path, x, sr)))
    seed = 7 if noise == "keyed" else None
    E.run_calls(args, model, "n/a", names, n_samples, load, seed, device="cpu")

    # the enhance calls: planned order, keys only in keyed mode and in the order of the flattened groups
    want = PLAN[(noise, 1, 2, 1)][0]
    assert [c["files"] for c in calls] == want
    for c, call in zip(calls, want):
        flat = [i for g in call for i in g]
        assert c["flat"] == flat and c["lanes"] is None
        assert c["keys"] == ([utterance_key(names[i]) for i in flat] if noise == "keyed" else None)
        assert c["seed"] == (7 if noise == "keyed" else 0)
    # every file exactly once, holding its own constant
    out = tmp_path / "out"
    assert sorted(written) == [str(out / "files" / n) for n in names]
    for i, n in enumerate(names):
        sr, pcm = wavfile.read(out / "files" / n)
        assert sr == 16000 and pcm.shape == (n_samples[i],) and (pcm == round((i + 1) / 16 * 32767)).all()
    # rows in file order under the columns of the run
    with open(out / "_results.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == E._COLUMNS + (("valid_loss",) if valid_loss else ())
    assert [r[0] for r in rows[1:]] == names and all(len(r) == len(rows[0]) for r in rows)
    if valid_loss:
        assert [float(r[-1]) for r in rows[1:]] == [0.25 + i for i in range(5)]
    # the settings file is what _write_reports writes for these arguments
    (tmp_path / "want").mkdir()
    E._write_reports(str(tmp_path / "want"), {c: [] for c in E._COLUMNS}, args, model, "n/a", seed)
    text = (out / "_settings.txt").read_text()
    assert text == (tmp_path / "want" / "_settings.txt").read_text()
    assert f"noise: {noise}\nnoise seed: {seed}\ngpus: 1\n" in text
    assert ("valid_loss draws: 2\n" in text) == bool(valid_loss)
    # the last line of the run, in the wording of its mode
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("enhanced 5 utterances (1130 frames) in ")
    assert ("on 1 GPU(s), keyed noise seed 7 -> " in line) == (noise == "keyed")
