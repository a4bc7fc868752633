"""Host: trailing chunks (flowmse_amd.chunked.plan_trailing / blend_trailing_reference, the trailing schedule of
flowmse_amd.live, the ``--hop_frames`` / ``--fade_frames`` command line).  No GPU: arithmetic and argument parsing only."""
import numpy as np
import pytest

from flowmse_amd import enhance
from flowmse_amd.chunked import blend_chunks_reference, blend_trailing_reference, plan_chunks, plan_trailing
from flowmse_amd.live import latency_samples, live_plan
from flowmse_amd.util import synth

GEOMETRIES = [(16, 4), (8, 8), (4, 2), (32, 0), (64, 0)]


def test_plan_trailing_values():
    assert plan_trailing(157, 64, 16, 4) == (10, 48, 160)
    assert plan_trailing(160, 64, 16, 4) == (10, 48, 160) and plan_trailing(161, 64, 16, 4) == (11, 48, 176)
    assert plan_trailing(1, 64, 16, 4) == (1, 48, 16) and plan_trailing(3, 64, 16, 0) == (1, 48, 16)    # no K = 1 special case
    assert plan_trailing(100, 64, 64, 0) == (2, 0, 128) and plan_trailing(100, 128, 4, 4) == (25, 124, 100)
    assert plan_trailing(65, 64, 32, 32) == (3, 32, 96) and plan_trailing(7, 256, 8, 2) == (1, 248, 8)
    for T in (1, 5, 63, 64, 65, 1000):
        for H, X in GEOMETRIES:
            K, P, Tg = plan_trailing(T, 64, H, X)
            assert K == -(-T // H) and P == 64 - H and Tg == K * H >= T > Tg - H


@pytest.mark.parametrize("args,word", [((0, 64, 16, 4), "T must be"), ((10, 0, 16, 4), "chunk_frames"), ((10, 96, 16, 4), "chunk_frames"),
                                       ((10, -64, 16, 4), "chunk_frames"), ((10, 64, 15, 4), "hop_frames"), ((10, 64, 2, 0), "hop_frames"),
                                       ((10, 64, 66, 0), "hop_frames"), ((10, 64, 0, 0), "hop_frames"), ((10, 64, 16, -1), "fade_frames"),
                                       ((10, 64, 16, 17), "fade_frames"), ((10, 64, 40, 30), "fade_frames"),
                                       ((10, 64, 64, 2), "fade_frames")])
def test_plan_trailing_refusals_name_the_value(args, word):
    with pytest.raises(ValueError, match="plan_trailing") as e:
        plan_trailing(*args)
    assert word in str(e.value)
    bad = {"T must be": args[0], "chunk_frames": args[1], "hop_frames": args[2], "fade_frames": args[3]}[word]
    assert f"got {bad}" in str(e.value)


@pytest.mark.parametrize("H,X", GEOMETRIES, ids=lambda v: str(v))
def test_blend_returns_a_spectrogram_cut_into_chunks_exactly(H, X):
    Tc, K, F = 64, 5, 8
    P, Tg = Tc - H, K * H
    S = synth.synth_spectrogram(3 + H + X, 1, F, Tg).astype(np.complex128)
    padded = np.concatenate([np.zeros((1, 1, F, P), dtype=np.complex128), S], axis=3)         # stream frame u = t + P
    chunks = np.concatenate([padded[..., k * H:k * H + Tc] for k in range(K)], axis=0)
    out = blend_trailing_reference(chunks, H, X)
    assert out.dtype == np.complex128 and out.shape == (1, 1, F, Tg) and np.array_equal(out, S)
    assert np.abs(S).max() > 0
    # independent chunks: every output frame is the stated combination of at most two chunks
    c = synth.synth_spectrogram(50 + H + X, K, F, Tc).astype(np.complex128)
    out = blend_trailing_reference(c, H, X)
    for t in range(Tg):
        k = min((t + X) // H, K - 1)
        j = t - k * H + P
        want = c[k, 0, :, j]
        if k > 0 and t < k * H:
            i = t - (k * H - X)
            assert 0 <= i < X
            a = c[k - 1, 0, :, j + H]
            want = a + (i + 0.5) / X * (want - a)
        assert np.array_equal(out[0, 0, :, t], want), t
    with pytest.raises(ValueError):
        blend_trailing_reference(c, H, H + 1)


def test_the_overlap_blend_is_the_trailing_blend_with_the_fade_over_the_whole_lead():
    """Chunks ``hop`` apart that share To = Tc - hop frames are trailing chunks at H = hop, X = P = To, counted from To frames
    later: the two float64 statements of the seam rule agree exactly on independent random chunks, and the To frames before
    the trailing origin are chunk 0's."""
    Tc, K, F = 64, 3, 8
    for To in range(0, 33, 2):
        hop = Tc - To
        c = synth.synth_spectrogram(70 + To, K, F, Tc).astype(np.complex128)
        over, trail = blend_chunks_reference(c, hop), blend_trailing_reference(c, hop, To)
        assert over.shape == (1, 1, F, (K - 1) * hop + Tc) and trail.shape == (1, 1, F, K * hop)
        assert np.array_equal(over[..., To:], trail), To
        assert np.array_equal(over[..., :To], c[:1, :, :, :To]) and np.abs(trail).max() > 0


@pytest.mark.parametrize("H,X", GEOMETRIES[:4], ids=lambda v: str(v))
def test_live_schedule_sample_by_sample(H, X):
    """Arrival simulated sample by sample over three hops and a little more: the chunk count and the samples final follow
    ``n_k = 128 (k H + H - 1) + 255`` and ``E_k = 128 ((k + 1) H - X) - 255`` (clamped at 0), and the worst lag between a sample's
    arrival and its return -- the oldest sample not yet returned, seen just before a chunk runs -- is ``128 (H + X) + 382``."""
    Tc = 64
    n_k = [128 * (k * H + H - 1) + 255 for k in range(5)]
    E_k = [max(128 * ((k + 1) * H - X) - 255, 0) for k in range(5)]
    worst, ready_prev = 0, 0
    for n in range(0, n_k[3] + 300):
        ready, final = live_plan(n, Tc, hop_frames=H, fade_frames=X)
        assert ready == sum(n >= x for x in n_k)
        assert final == (E_k[ready - 1] if ready else 0)
        assert final <= n
        if ready > ready_prev:                                # chunk `ready - 1` ran at this count: what was pending just before
            assert n == n_k[ready - 1]
            worst = max(worst, n - (E_k[ready - 2] if ready >= 2 else 0))
        ready_prev = ready
    assert ready_prev == 4
    assert worst == 128 * (H + X) + 382 == latency_samples(Tc, hop_frames=H, fade_frames=X)
    # a chunk that became ready this way is never the last
    for k in range(4):
        assert live_plan(n_k[k], Tc, finished=True, hop_frames=H, fade_frames=X)[0] >= k + 2
    assert live_plan(300, Tc, finished=True, hop_frames=H, fade_frames=X) == (-(-3 // H), 300)
    assert live_plan(20000, Tc, finished=True, hop_frames=H, fade_frames=X) == (-(-157 // H), 20000)


def test_latency_values_and_the_default_schedule_is_untouched():
    assert latency_samples(64, hop_frames=16, fade_frames=4) == 2942 and round(2942 / 16000, 3) == 0.184
    assert latency_samples(64, hop_frames=8, fade_frames=2) == 1662 and round(1662 / 16000, 3) == 0.104
    assert latency_samples(256, hop_frames=16, fade_frames=4) == 2942          # the hop sets it, not the chunk
    assert latency_samples(64) == 128 * 64 + 382 and latency_samples(256) == 128 * 256 + 382
    assert live_plan(128 * 63 + 255, 64, 16) == (1, 128 * 48 - 255) and live_plan(128 * 63 + 254, 64, 16) == (0, 0)
    assert live_plan(40000, 64, 16, finished=True) == (plan_chunks(40000 // 128 + 1, 64, 16)[0], 40000)
    # another rate: the worst case over k of the three schedules, never below the 16 kHz figure scaled
    at48 = latency_samples(64, 48000, "input", hop_frames=16, fade_frames=4)
    assert 3 * 2942 <= at48 <= 3 * 2942 + 3 * 30 + 64
    assert latency_samples(64, 48000, "16000", hop_frames=16, fade_frames=4) >= 3 * 2942
    for bad in (dict(hop_frames=15), dict(hop_frames=16, fade_frames=17), dict(hop_frames=128)):
        with pytest.raises(ValueError, match="plan_trailing"):
            latency_samples(64, **bad)
        with pytest.raises(ValueError, match="plan_trailing"):
            live_plan(1000, 64, **bad)


def test_command_line(capsys):
    a = enhance.parse_args(["--output", "o", "--synthetic", "1", "--chunk_frames", "64", "--hop_frames", "16", "--fade_frames", "4"])
    assert (a.hop_frames, a.fade_frames, a.overlap_frames) == (16, 4, 32)
    a = enhance.parse_args(["--live", "--synthetic", "1", "--chunk_frames", "64", "--hop_frames", "8"])
    assert (a.hop_frames, a.fade_frames) == (8, 0)
    a = enhance.parse_args(["--live", "--synthetic", "1", "--chunk_frames", "64", "--hop_frames", "16", "--live_rate", "48000",
                            "--output_rate", "input"])
    assert a.hop_frames == 16
    a = enhance.parse_args(["--output", "o", "--synthetic", "1", "--resample", "--hop_frames", "16", "--chunk_frames", "64"])
    assert a.resample and a.hop_frames == 16
    # without the flags nothing moved
    a = enhance.parse_args(["--output", "o", "--synthetic", "1"])
    assert (a.hop_frames, a.fade_frames, a.chunk_frames, a.overlap_frames) == (None, 0, 256, 32)
    assert enhance.parse_args(["--output", "o", "--synthetic", "1", "--overlap_frames", "16", "--chunk_frames", "64"]).overlap_frames == 16
    file, live, geo = ["--output", "o", "--synthetic", "1"], ["--live", "--synthetic", "1"], ["--chunk_frames", "64", "--hop_frames", "16"]
    for argv, words in ((file + geo + ["--pool"], ["--hop_frames", "--pool"]),
                        (file + geo + ["--pool", "--samples", "2"], ["--hop_frames"]),
                        (file + geo + ["--samples", "2"], ["--hop_frames", "--samples 2"]),
                        (file + geo + ["--channels", "all"], ["--hop_frames", "--channels all"]),
                        (live + geo + ["--live_channels", "2"], ["--hop_frames", "--live_channels 2"]),
                        (file + geo + ["--noise", "torch"], ["--hop_frames", "--noise torch"]),
                        (live + geo + ["--noise", "torch"], ["--hop_frames", "--noise torch"]),
                        (file + geo + ["--overlap_frames", "32"], ["--hop_frames", "--overlap_frames 32"]),
                        (live + geo + ["--overlap_frames", "16"], ["--hop_frames", "--overlap_frames 16"]),
                        (file + ["--fade_frames", "4"], ["--fade_frames 4", "needs --hop_frames"]),
                        (live + ["--fade_frames", "2"], ["--fade_frames 2", "needs --hop_frames"]),
                        (file + ["--chunk_frames", "64", "--hop_frames", "15"], ["hop_frames", "got 15"]),
                        (live + ["--chunk_frames", "64", "--hop_frames", "16", "--fade_frames", "17"], ["fade_frames", "got 17"]),
                        (file + ["--hop_frames", "512"], ["hop_frames", "got 512"])):
        with pytest.raises(SystemExit) as e:
            enhance.parse_args(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (argv, err)


def test_live_pool_refuses_the_keywords_by_name():
    from flowmse_amd.livepool import LivePool
    pool = LivePool.__new__(LivePool)                                  # open() refuses before it touches the pool
    for kw in (dict(hop_frames=16), dict(hop_frames=16, fade_frames=4), dict(fade_frames=2)):
        with pytest.raises(ValueError, match="hop_frames"):
            pool.open([1], 0.5, **kw)
