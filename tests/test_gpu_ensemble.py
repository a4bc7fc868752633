"""GPU: ensembles of draws (flowmse_amd.ensemble) -- ``flowse_istft_decompress_ensemble`` against the stacks kernel (one draw:
bit for bit) and against the float64 ``ensemble_reference`` (mean and tracks), both row layouts, ``enhance_pooled(draws=...)``
against the single-draw runs, and ``evaluate --samples`` in child processes, one after the other, each under its own time
limit.  No test asserts a time.
"""
import csv
import filecmp
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cases as C
from flowmse_amd.ensemble import agreements, ensemble_reference
from flowmse_amd.pooled import enhance_pooled
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1F2E3D4C5B6A7988
HARD_CAP = 1e-5                  # of the mean waveform, relative to the largest single-draw peak, whatever is measured
MARGIN = 4                       # times the stacks kernel's own error: D - 1 fp32 additions and one product per bin
S, D, K, TC, HOP = 2, 3, 3, 64, 48
TG = (K - 1) * HOP + TC          # 160
LENGTHS = (19200, 19201, 20607)  # a multiple of 128 (the last real frame has no block of its own), one more, the largest
SCALE = 0.7


@pytest.fixture(scope="module")
def dm():
    assert torch.cuda.is_available()
    from flowmse_amd.data_module import SpecTransform
    return SpecTransform()


def _rows(seed, n, Tc=TC):
    return C.c64(synth.synth_spectrogram(seed, n, 256, Tc))


def _err(got, ref, peak=None):
    """max abs error over the reference's peak (or the given one)."""
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() if peak is None else peak))


@pytest.fixture(scope="module")
def independent():
    """[S][D][K] rows of independent draws, and their float64 references per length: computed once, never written to."""
    rows = _rows(70, S * D * K)
    ref = {}
    for length in LENGTHS:
        wave, tracks = ensemble_reference(rows, S, D, HOP, length, SCALE)
        singles = [ensemble_reference(_draw(rows, d), S, 1, HOP, length, SCALE)[0] for d in range(D)]
        ref[length] = (wave, tracks, singles)
    return rows, ref


def _draw(rows, d):
    """The [S][K] rows of draw d out of [S][D][K]."""
    return torch.cat([rows[(s * D + d) * K:(s * D + d + 1) * K] for s in range(S)])


# ---------------------------------------------------------------------------------------------------- 6
def test_one_draw_is_the_stacks_kernel_bit_for_bit(dm):
    rows = _rows(60, S * K).cuda()
    for length in LENGTHS + (5000,):
        got = dm.synthesize_ensemble(rows, S, 1, HOP, length, SCALE)
        assert got.shape == (S, length) and torch.equal(got, dm.synthesize_stacks(rows, S, HOP, length, SCALE)), length
    # strides wider than the stack: rows 0..2 and 3..5 of 6, read as 2 stacks of K = 2 that are 3 rows apart
    got = dm.synthesize_ensemble(rows, 2, 1, HOP, 12000, SCALE, stack_stride=3, K=2)
    want = dm.synthesize_stacks(torch.cat([rows[0:2], rows[3:5]]), 2, HOP, 12000, SCALE)
    assert torch.equal(got, want)
    one = _rows(61, 2).cuda()                                       # K = 1, Tc = hop = 64: the plain inverse transform
    got = dm.synthesize_ensemble(one, 2, 1, 64, 300, SCALE)
    assert torch.equal(got, dm.synthesize(one, 300, SCALE)) and torch.isfinite(got).all()
    with pytest.raises(Exception, match="tracks"):
        dm.synthesize_ensemble(one, 2, 1, 64, 300, tracks=True)


# ---------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("length", LENGTHS)
def test_mean_of_three_draws_against_float64(dm, independent, length):
    """The mean waveform is within 4 x the stacks kernel's own error (``e_parent``: the worst of ``synthesize_stacks`` on each
    draw alone against the float64 reference of that draw, max abs over the reference's peak) of ``ensemble_reference``,
    relative to the largest single-draw peak, and within 1e-5 whatever is measured.  Figures: DESIGN 6f."""
    rows, ref = independent
    wave, _, singles = ref[length]
    dev = rows.cuda()
    e_parent = max(_err(dm.synthesize_stacks(_draw(dev, d), S, HOP, length, SCALE), singles[d]) for d in range(D))
    peak = max(np.abs(s).max() for s in singles)
    got = dm.synthesize_ensemble(dev, S, D, HOP, length, SCALE)
    err = _err(got, wave, peak)
    print(f"ensemble mean, Lout={length}: e_parent {e_parent:.3e}, ensemble error {err:.3e} (bound {MARGIN} x e_parent, cap {HARD_CAP})")
    assert got.shape == (S, length) and torch.isfinite(got).all()
    assert err <= MARGIN * e_parent and err <= HARD_CAP, (length, err, e_parent)
    # what the bound is there to catch lies far outside it: a dropped draw, for one
    dropped = np.mean([singles[0], singles[1]], axis=0)
    assert _err(dropped, wave, peak) > 100 * HARD_CAP


# ---------------------------------------------------------------------------------------------------- 8
def _check_tracks(dm, rows, bound_dev, bound_pow, label):
    length = 19200                                                  # 151 real frames of the 160
    _, tracks_ref = ensemble_reference(rows, S, D, HOP, length, SCALE)
    wave, tracks = dm.synthesize_ensemble(rows.cuda(), S, D, HOP, length, SCALE, tracks=True)
    assert tracks.shape == (S, 2, TG) and tracks.dtype == torch.float32 and torch.isfinite(tracks).all()
    assert torch.equal(wave, dm.synthesize_ensemble(rows.cuda(), S, D, HOP, length, SCALE))
    got = tracks.cpu().numpy().astype(np.float64)
    rel = np.abs(got - tracks_ref) / tracks_ref                     # all Tg frames, the padded ones included
    e_dev, e_pow = float(rel[:, 0].max()), float(rel[:, 1].max())
    a_got, a_ref = agreements(tracks, length), agreements(tracks_ref, length)
    print(f"tracks, {label}: per-frame relative error dev {e_dev:.3e} (bound {bound_dev}), pow {e_pow:.3e} (bound {bound_pow}); "
          f"agreement {a_got[0]:.4f} dB against {a_ref[0]:.4f} dB")
    assert e_dev <= bound_dev and e_pow <= bound_pow, (e_dev, e_pow)
    assert all(abs(a - b) <= 1e-2 for a, b in zip(a_got, a_ref)), (a_got, a_ref)
    return a_ref


def test_tracks_of_independent_draws(dm, independent):
    """A fixed-order fp32 sum of 256 D non-negative terms: worst case 256 D 2^-24 = 4.6e-5 at D = 3; bound 1e-4."""
    a = _check_tracks(dm, independent[0], 1e-4, 1e-4, "independent draws")
    # independent draws of equal power: |M|^2 is 1 / D of a draw's, the deviation a draw's own -- the output is mostly the draw
    assert all(abs(v - 10 * math.log10(1 / D)) < 0.5 for v in a)


def test_tracks_of_draws_that_nearly_agree(dm):
    """Draws within 1e-3 of a common row IN THE LINEAR DOMAIN: the compressed rows are ``base (1 + 5e-4 w)``, ``w`` complex
    standard normal (unbounded, so 1e-3 is the typical size and not a cap), and the square-law decompression doubles a
    relative perturbation -- deviations of about 1e-3 of ``|Z|``, agreement about 60 dB (62 dB on these rows; the issue's
    simulation had 59 dB: smaller deviations are the harder case for a small term).  The deviations are a small term, which
    the second pass from the finished mean finds (a decompressed value carries <= 4 2^-24 relative error, the mean <= (D + 1) 2^-24, against deviations of 1e-3:
    worst case 8e-4; bound 2e-3) and ``sum |Z_d|^2 - D |M|^2`` would not (it misses the bound by more than a factor of ten)."""
    base = synth.synth_spectrogram(71, S * K, 256, TC).astype(np.complex128).reshape(S, 1, K, 1, 256, TC)
    wobble = synth.complex_normal(72, 5, (S, D, K, 1, 256, TC), 1.0).astype(np.complex128)
    rows = C.c64((base * (1.0 + 5e-4 * wobble)).reshape(S * D * K, 1, 256, TC).astype(np.complex64))
    a = _check_tracks(dm, rows, 2e-3, 1e-4, "draws within 1e-3")
    assert all(55.0 < v < 65.0 for v in a)


# ---------------------------------------------------------------------------------------------------- 9
def test_row_layouts_many_draws_and_repeatability(dm):
    rows = _rows(73, 6).cuda()                                      # S = 3, D = 2, K = 1, contiguous [S][D]
    want, want_tracks = dm.synthesize_ensemble(rows, 3, 2, 64, 8000, SCALE, tracks=True)
    by_draw = torch.stack([rows[2 * s + d] for d in range(2) for s in range(3)])          # rows ordered (draw, stack)
    got, got_tracks = dm.synthesize_ensemble(by_draw, 3, 2, 64, 8000, SCALE, stack_stride=1, draw_stride=3, tracks=True)
    assert torch.equal(got, want) and torch.equal(got_tracks, want_tracks)
    assert not torch.equal(want[0], want[1])
    # one utterance out of a (draw, utterance) group: the view evaluate passes
    got1, tr1 = dm.synthesize_ensemble(by_draw[1:5], 1, 2, 64, 8000, SCALE, draw_stride=3, K=1, tracks=True)
    assert torch.equal(got1[0], want[1]) and torch.equal(tr1[0], want_tracks[1])
    many = _rows(74, 64).cuda()
    a, ta = dm.synthesize_ensemble(many, 1, 64, 64, 8191, SCALE, tracks=True)
    b, tb = dm.synthesize_ensemble(many, 1, 64, 64, 8191, SCALE, tracks=True)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(ta).all() and bool((ta > 0).all())
    assert torch.equal(a, b) and torch.equal(ta, tb)
    tref = ensemble_reference(many, 1, 64, 64, 8191, SCALE)[1]     # worst case of the fixed-order sum of 256 D terms
    assert float((np.abs(ta.cpu().numpy() - tref) / tref).max()) <= 256 * 64 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- 10, 11
FILES = [("a.wav", 1, 20000), ("b.wav", 2, 12000), ("c.wav", 1, 5000)]


def _signal(seed, n, std=0.1):
    return torch.from_numpy(synth.normal(seed, 9, (1, n), std))


def _samples():
    b = torch.cat([_signal(12, 12000), 0.5 * _signal(13, 12000)], dim=0)
    return {"a.wav": _signal(11, 20000), "b.wav": b, "c.wav": _signal(14, 5000)}


@pytest.fixture(scope="module")
def full():
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **C.FULL)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


def _run_pooled(full, items, **kw):
    samples, out, agree = _samples(), {}, {}

    def write(i, x_hat):
        assert items[i][0] not in out
        out[items[i][0]] = x_hat.cpu()

    def agreement(i, values):
        assert items[i][0] not in agree and items[i][0] not in out  # once per file, before its write
        agree[items[i][0]] = values

    stats = enhance_pooled(full, lambda i: samples[items[i][0]].cuda(), items, write, batch=3, chunk_frames=64,
                           overlap_frames=16, N=2, noise_seed=SEED, agreement=agreement, **kw)
    return out, agree, stats


@pytest.fixture(scope="module")
def single_draws(full):
    """The three runs ``draws=(d,)``, with the stacks each file was finished from (a spy on ``synthesize_stacks``)."""
    dm = full.data_module
    real, runs = dm.synthesize_stacks, []
    for d in range(3):
        stacks = []

        def spy(chunks, n, hop, length, scale=1.0):
            stacks.append((chunks.cpu(), n, hop, length, scale))
            return real(chunks, n, hop, length, scale)

        dm.synthesize_stacks = spy
        try:
            out, agree, stats = _run_pooled(full, FILES, draws=(d,))
        finally:
            del dm.synthesize_stacks
        assert agree == {} and stats == dict(calls=3, rows=8, fillers=1) and len(stacks) == 3
        runs.append((out, stacks))
    return runs


def test_draw_zero_is_the_run_without_the_argument(full, single_draws):
    plain, agree, stats = _run_pooled(full, FILES)
    assert agree == {} and stats == dict(calls=3, rows=8, fillers=1)
    for name, ch, n in FILES:
        assert plain[name].shape == (ch, n) and torch.equal(plain[name], single_draws[0][0][name]), name
    assert not torch.equal(plain["a.wav"], single_draws[1][0]["a.wav"])


def test_pooled_ensemble_against_the_single_draw_runs(full, single_draws):
    """``draws=(0, 1, 2)`` samples the rows of the three runs ``draws=(d,)`` bit for bit (every call has ``batch`` rows), so
    only the finish differs: every file and channel against the float64 mean of the three single-draw outputs, under the
    bound of the kernel test -- 4 x the stacks kernel's error on these very stacks, and 1e-5."""
    out, agree, stats = _run_pooled(full, FILES, draws=(0, 1, 2))
    assert stats == dict(calls=8, rows=24, fillers=0)
    # folder independence: c.wav moves to the head of the run, a.wav to other calls beside other neighbours
    other, other_agree, stats = _run_pooled(full, [FILES[2], FILES[0]], draws=(0, 1, 2))
    assert stats == dict(calls=4, rows=12, fillers=0)
    for name in ("a.wav", "c.wav"):
        assert torch.equal(other[name], out[name]) and other_agree[name] == agree[name], name
    for i, (name, ch, n) in enumerate(FILES):
        singles = [run[0][name].numpy().astype(np.float64) for run in single_draws]
        e_parent = 0.0
        for out_d, (_, stacks) in zip(singles, single_draws):
            chunks, S_, hop, length, scale = stacks[i]                    # one width: files finish in the order of the items
            assert (S_, length) == (ch, n)
            e_parent = max(e_parent, _err(out_d, ensemble_reference(chunks, ch, 1, hop, n, scale)[0]))
        want, peak = np.mean(singles, axis=0), max(np.abs(s).max() for s in singles)
        err = _err(out[name], want, peak)
        print(f"pooled ensemble, {name}: e_parent {e_parent:.3e}, error against the mean of the single-draw runs {err:.3e}; "
              f"agreement {agree[name]}")
        assert out[name].shape == (ch, n) and err <= MARGIN * e_parent and err <= HARD_CAP, (name, err, e_parent)
        assert len(agree[name]) == ch and all(math.isfinite(v) for v in agree[name])
        assert _err(singles[0], want, peak) > 100 * HARD_CAP        # the draws do differ: the mean is not any one of them
    assert set(agree) == {n for n, _, _ in FILES}


# ---------------------------------------------------------------------------------------------------- 12
def _evaluate(out, extra, limit=500):
    return subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "flowmse_amd.evaluate",
                           "--folder_destination", str(out), "--synthetic", "2", "--noise", "keyed", "--seed", "7",
                           "--batch", "2"] + extra, cwd=ROOT, capture_output=True, text=True)


@pytest.mark.timeout(1800)
def test_evaluate_samples_in_child_processes(tmp_path):
    """``--samples 1`` writes the bytes of the run without the flag; ``--samples 2 --metrics device`` writes the mean's wavs,
    an ``agreement_db`` column and the ``samples: 2`` line, the same bytes twice.  Children run one after the other; a
    failed one ends the test."""
    from scipy.io import wavfile
    runs = [("plain", []), ("one", ["--samples", "1"]), ("two", ["--samples", "2", "--metrics", "device"]),
            ("again", ["--samples", "2", "--metrics", "device"])]
    for tag, args in runs:
        r = _evaluate(tmp_path / tag, args)
        assert r.returncode == 0, f"run {tag} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    names = ["synthetic_00.wav", "synthetic_01.wav"]
    reports = ["_results.csv", "_avg_results.txt", "_settings.txt"]
    for a, b in (("plain", "one"), ("two", "again")):
        for n in [os.path.join("files", n) for n in names] + reports:
            assert filecmp.cmp(tmp_path / a / n, tmp_path / b / n, shallow=False), (a, b, n)
    assert "samples" not in (tmp_path / "one" / "_settings.txt").read_text()
    assert "Agreement" not in (tmp_path / "one" / "_avg_results.txt").read_text()
    assert "samples: 2\n" in (tmp_path / "two" / "_settings.txt").read_text()
    assert "Agreement: " in (tmp_path / "two" / "_avg_results.txt").read_text()
    with open(tmp_path / "one" / "_results.csv", newline="") as f:
        assert "agreement_db" not in next(csv.reader(f))
    with open(tmp_path / "two" / "_results.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0][-1] == "agreement_db" and [r[0] for r in rows[1:]] == names
    assert all(math.isfinite(float(r[-1])) for r in rows[1:])
    assert all(math.isfinite(float(v)) for r in rows[1:] for v in r[2:6])        # ESTOI and the ratios of the mean, on the device
    for n in names:
        sr, mean = wavfile.read(tmp_path / "two" / "files" / n)
        assert sr == 16000 and mean.shape == (32000,) and np.abs(mean).max() > 0
        assert not np.array_equal(mean, wavfile.read(tmp_path / "plain" / "files" / n)[1])
