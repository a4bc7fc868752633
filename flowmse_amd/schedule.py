"""Chunk schedules: the geometry of a chunked recording as one object, for the file, live and pool paths.

Host arithmetic only.  A schedule answers, for chunk ``k`` of a recording cut by ``chunked.plan_chunks`` (``OverlapSchedule``)
or ``chunked.plan_trailing`` (``TrailingSchedule``), the questions every consumer asks: where the chunk's frames and its
keyed noise start, at which sample count it is ready, which output samples are final after it, which samples it reads,
which may be dropped after it, and how much history the emitted range needs.  ``flowmse_amd.live``'s module docstring
states the schedule and why it holds; tests/test_schedule_host.py holds every answer to the STFT's index ranges (frame ``t``
reads and covers the samples ``[128 t - 255, 128 t + 254]``, reflected at 0).
"""
from flowmse_amd.chunked import plan_chunks, plan_trailing

HOP, PADC = 128, 255                # hop_length and n_fft // 2 of the released STFT, the only one the kernels cover
RATE = 16000                        # the network's sample rate
KEEP = PADC + 1                     # samples kept before the next chunk's first frame centre


class _Schedule:
    """What both geometries share.  A subclass sets ``Tc``, ``hop`` (frames between two chunks' noise origins),
    ``keep_two``, ``min_capacity`` and ``latency16`` and defines ``chunks``, ``first_frame``, ``ready_at``, ``final_after``
    and ``single_width``."""

    def noise_frame0(self, k):
        """The stream frame at which row ``k`` addresses the keyed noise, and its slice origin in the chunk stack."""
        return k * self.hop

    def window_lo(self, k):
        """First sample chunk ``k`` reads while the recording is open."""
        return max(HOP * self.first_frame(k) - PADC, 0)

    def drop_before(self, k):
        """After chunk ``k`` the samples before this are dropped: one more than chunk ``k + 1`` reads, for the right
        reflection of a recording that ends one frame past chunk ``k``."""
        return max(HOP * self.first_frame(k + 1) - KEEP, 0)

    def plan(self, n_samples, finished=False):
        """``(chunks_ready, samples_final)`` after ``n_samples`` samples; ``finished``: the recording ended there."""
        n = int(n_samples)
        if n < 0:
            raise ValueError(f"live_plan: n_samples must be >= 0, got {n}")
        if finished:
            return self.chunks(n // HOP + 1), n
        if n < self.ready_at(0):
            return 0, 0
        ready = (n - self.ready_at(0)) // (HOP * self.hop) + 1
        return ready, self.final_after(ready - 1)

    def latency(self, input_rate=RATE, output_rate="16000"):
        """Worst algorithmic latency in samples at ``input_rate``: ``latency16`` at 16 kHz; at another rate the worst case
        over ``k = 0 .. up`` of (input samples arrived when chunk ``k`` runs) - (input samples returned before it)."""
        if int(input_rate) == RATE:
            return self.latency16
        from flowmse_amd.resample import rational, stream_plan
        up, down = rational(input_rate, RATE)
        half = 10 * max(up, down)
        worst = 0
        for k in range(up + 1):
            arrived = (half + (self.ready_at(k) - 1) * down) // up + 1
            e = self.final_after(k - 1)
            returned = stream_plan(e, down, up) if output_rate == "input" else e * down // up
            worst = max(worst, arrived - returned)
        return worst


class OverlapSchedule(_Schedule):
    """``plan_chunks``: chunk ``k`` holds the frames ``[k hop, k hop + Tc)``, ``hop = Tc - To``."""

    def __init__(self, Tc, To):
        _, self.hop, _ = plan_chunks(1, Tc, To)
        self.Tc, self.To = int(Tc), int(To)
        self.keep_two = self.Tc - 2 * self.To < 3           # To = Tc / 2: the emitted range reaches a blended frame of chunk k-1
        self.min_capacity = 0                               # the buffer grows with the backlog
        self.latency16 = HOP * self.Tc + 382

    def chunks(self, T):
        return plan_chunks(T, self.Tc, self.To)[0]

    def first_frame(self, k):
        return k * self.hop

    def ready_at(self, k):
        return HOP * (k * self.hop + self.Tc - 1) + PADC

    def final_after(self, k):
        return HOP * (k + 1) * self.hop - PADC if k >= 0 else 0

    def single_width(self, T):
        """``K == 1``: the one row's width, ``T`` padded to a multiple of 64; None when ``T`` frames make several chunks."""
        return -(-int(T) // 64) * 64 if T <= self.Tc else None


class TrailingSchedule(_Schedule):
    """``plan_trailing``: chunk ``k`` holds the frames ``[k H - P, k H + H)``, ``P = Tc - H``, those ``< 0`` zero."""

    def __init__(self, Tc, H, X):
        _, self.P, _ = plan_trailing(1, Tc, H, X)
        self.Tc, self.H, self.X = int(Tc), int(H), int(X)
        self.hop = self.H
        self.keep_two = self.H - self.X < 3                 # the emitted range reaches a faded frame of chunk k-1
        self.min_capacity = HOP * self.Tc + 382             # held before a push, whatever k
        self.latency16 = HOP * (self.H + self.X) + 382

    def chunks(self, T):
        return plan_trailing(T, self.Tc, self.H, self.X)[0]

    def first_frame(self, k):
        return max(k * self.H - self.P, 0)

    def ready_at(self, k):
        return HOP * (k * self.H + self.H - 1) + PADC

    def final_after(self, k):
        return max(HOP * ((k + 1) * self.H - self.X) - PADC, 0) if k >= 0 else 0

    def single_width(self, T):
        """None: a recording shorter than one hop is one right-aligned chunk, there is no ``K == 1`` case."""
        return None


def schedule_for(Tc, To, hop_frames=None, fade_frames=0, who="schedule_for"):
    """The schedule of a caller's geometry keywords: trailing with ``hop_frames`` (``To`` is not read), else overlap.
    ``fade_frames`` without ``hop_frames`` is refused under the caller's name ``who``."""
    if hop_frames is not None:
        return TrailingSchedule(Tc, hop_frames, fade_frames)
    if fade_frames:
        raise ValueError(f"{who}: fade_frames={fade_frames} needs hop_frames (the trailing schedule)")
    return OverlapSchedule(Tc, To)
