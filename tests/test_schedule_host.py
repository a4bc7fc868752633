"""flowmse_amd.schedule held to the definitions, not to its closed forms (CPU, seconds).

What is taken as given: the STFT's index ranges (``n_fft = 510``, ``hop_length = 128``, ``center=True``: frame ``t`` reads and
covers the samples ``[128 t - 255, 128 t + 254]``, reflected at 0 and, once the recording has ended at ``L``, at ``L - 1``), the
frames a chunk holds (``plan_chunks`` / ``plan_trailing``) and the seam rule as ``blend_chunks_reference`` /
``blend_trailing_reference`` state it.  Everything the schedule objects answer is recomputed from those by enumeration."""
import numpy as np
import pytest

from flowmse_amd.chunked import plan_chunks, plan_trailing
from flowmse_amd.live import live_plan
from flowmse_amd.schedule import OverlapSchedule, TrailingSchedule

OVERLAP = [(64, 0), (64, 16), (64, 32), (128, 64), (256, 32)]
TRAILING = [(64, 16, 4), (64, 8, 8), (64, 4, 2), (64, 64, 0), (64, 32, 32), (128, 16, 0)]
KS = range(7)


class Geometry:
    """A geometry by its definitions: the real frames of chunk ``k``, how many chunks ``T`` frames make, and the chunks whose
    values fix output frame ``t`` (the owner, and for a blended frame the chunk before it) while the recording is open."""

    def __init__(self, *g):
        self.g, self.Tc = g, g[0]
        if len(g) == 2:
            Tc, To = g
            hop = Tc - To
            self.sched, self.live = OverlapSchedule(Tc, To), dict(Tc=Tc, To=To)
            self.frames = lambda k: range(k * hop, k * hop + Tc)
            self.column0 = lambda k: k * hop
            self.chunks = lambda T: plan_chunks(T, Tc, To)[0]
            self.owner, self.blended = (lambda t: t // hop), (lambda t, k: k > 0 and t - k * hop < To)
        else:
            Tc, H, X = g
            self.sched, self.live = TrailingSchedule(Tc, H, X), dict(Tc=Tc, hop_frames=H, fade_frames=X)
            self.frames = lambda k: range(max(k * H - (Tc - H), 0), k * H + H)
            self.column0 = lambda k: (k * H - (Tc - H)) + (Tc - H)          # stream frame u = t + P
            self.chunks = lambda T: plan_trailing(T, Tc, H, X)[0]
            self.owner, self.blended = (lambda t: (t + X) // H), (lambda t, k: k > 0 and t < k * H)

    def fixed_by(self, t):
        k = self.owner(t)
        return {k - 1, k} if self.blended(t, k) else {k}

    def reads(self, k, L=None):
        """``(lo, hi)``: the samples chunk ``k``'s frames read, open or (``L``) closed; frames ``>= T`` are zero."""
        t = np.array([t for t in self.frames(k) if L is None or t < L // 128 + 1])
        j = np.abs(128 * t[:, None] + np.arange(510)[None, :] - 255)
        if L is not None:
            j = np.where(j >= L, 2 * (L - 1) - j, j)
        return int(j.min()), int(j.max()) + 1

    def needs(self):
        """Per output sample, the chunks whose values it depends on: ``(lowest, highest)`` over the frames that cover it."""
        frames = max(self.frames(len(KS) + 1))
        lowest, highest = np.full(128 * frames, 1 << 30), np.zeros(128 * frames, dtype=np.int64)
        for t in range(frames + 2):
            lo, hi, by = max(128 * t - 255, 0), 128 * t + 255, self.fixed_by(t)
            lowest[lo:hi] = np.minimum(lowest[lo:hi], min(by))
            highest[lo:hi] = np.maximum(highest[lo:hi], max(by))
        return lowest, highest


@pytest.fixture(scope="module", params=OVERLAP + TRAILING, ids=str)
def geo(request):
    g = Geometry(*request.param)
    g.lowest, g.highest = g.needs()
    return g


def test_ready_at_is_the_first_count_at_which_no_frame_of_the_chunk_reads_past_the_end(geo):
    for k in KS:
        assert geo.sched.ready_at(k) == geo.reads(k)[1]


def test_final_after_is_the_first_sample_under_a_frame_that_a_later_chunk_fixes(geo):
    assert geo.sched.final_after(-1) == 0
    for k in KS:
        assert geo.sched.final_after(k) == int(np.argmax(geo.highest > k))
        assert (geo.highest[:geo.sched.final_after(k)] <= k).all() and geo.highest[geo.sched.final_after(k)] == k + 1


def test_the_emitted_range_needs_two_previous_chunks_exactly_when_keep_two_says_so(geo):
    s = geo.sched
    for k in KS:
        e0, e1 = s.final_after(k - 1), s.final_after(k)
        if e1 == e0:                                          # trailing, E_0 = 0: nothing is emitted with chunk 0
            assert k == 0 and len(geo.g) == 3
            continue
        assert geo.highest[e0:e1].max() == k and geo.lowest[e0:e1].min() >= max(k - 2, 0)
        if k >= 2:
            assert (geo.lowest[e0:e1].min() == k - 2) == s.keep_two, k


def test_the_window_is_what_the_chunk_reads_and_nothing_dropped_is_read_again(geo):
    """``drop_before(k - 1)`` keeps exactly one sample more than chunk ``k`` reads while the recording is open, clamped at 0
    where that chunk reads from sample 0 -- and a recording that ends there (the three shortest ``T`` that have a chunk ``k``,
    ``L`` at, just past and just before a multiple of 128) reads nothing below it through its right reflection."""
    s = geo.sched
    for k in KS:
        lo, hi = geo.reads(k)
        assert (s.window_lo(k), s.ready_at(k)) == (lo, hi)
        if k == 0:
            assert hi - 1 <= s.min_capacity or len(geo.g) == 2
            continue
        assert s.drop_before(k - 1) == max(lo - 1, 0) <= max(s.window_lo(k) - 1, 0)
        if len(geo.g) == 3:
            assert s.ready_at(k) - 1 - s.drop_before(k - 1) <= s.min_capacity
        T0 = next(T for T in range(1, 1 << 20) if geo.chunks(T) > k)          # the shortest recording that has a chunk k
        for L in (128 * (T0 - 1 + a) + d for a in (0, 1, 2) for d in (0, 1, 127)):
            assert geo.reads(k, L)[0] >= s.drop_before(k - 1), (k, L)
    assert s.min_capacity == (0 if len(geo.g) == 2 else 128 * geo.Tc + 382)


def test_latency_and_plan(geo):
    s = geo.sched
    ready = [geo.reads(k)[1] for k in KS]
    final = [0] + [int(np.argmax(geo.highest > k)) for k in KS]                    # final[k + 1] = E_k
    assert max(ready[k] - final[k] for k in KS) == s.latency16 == s.latency(16000, "16000")
    for n in sorted({max(r + d, 0) for r in ready for d in (-1, 0, 1)} | {0}):
        done = sum(n >= r for r in ready)
        if done < len(KS):                                    # past the last enumerated chunk the count is not known here
            assert s.plan(n) == (done, final[done])
        assert s.plan(n, False) == live_plan(n, finished=False, **geo.live)
        assert s.plan(n, True) == live_plan(n, finished=True, **geo.live) == (geo.chunks(n // 128 + 1), n)
    for k in KS:                                              # column 0 of row k, on the stream the noise is cut from
        assert s.noise_frame0(k) == geo.column0(k) and s.first_frame(k) == geo.frames(k)[0]


@pytest.mark.parametrize("Tc", [64, 256])
def test_single_width_is_the_file_geometry_of_a_one_chunk_file(Tc):
    from flowmse_amd.pooled import file_geometry
    s = OverlapSchedule(Tc, 32)
    for L in (256, 8191, 8192, 32767, 32768):
        T = L // 128 + 1
        K, _, width = file_geometry(L, Tc, 32)
        assert s.single_width(T) == (-(-T // 64) * 64 if K == 1 else None)
        assert width == (s.single_width(T) if K == 1 else Tc) and (K == 1) == (T <= Tc) and s.chunks(T) == K
    assert TrailingSchedule(Tc, 16, 4).single_width(1) is None
