"""GPU: the four trailing-chunk entries of the library (flowse_stft_compress_trailing, flowse_istft_decompress_trailing and
their window forms) -- rows against slices of ``analyze``, the seam rule against the float64 blend, the identity on chunks cut
from one spectrogram, the refusals, and the window entries against the file entries from the smallest legal windows, at small
indices and past 2^31.  Tc = 64 everywhere; no test asserts a time."""
import numpy as np
import pytest
import torch

import _cases as C
from flowmse_amd import _lib
from flowmse_amd.chunked import blend_trailing_reference, plan_trailing
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
L = _lib.lib
ERR_ARG, ERR_SHAPE = 1, 4
FACTOR, EXPONENT = 0.15, 0.5
ISTFT_TOL = 2e-5                  # tests/test_gpu_chunked.py, tests/test_gpu_ops.py: the fused iSTFT against torch.istft
TC = 64


@pytest.fixture(scope="module")
def dm():
    from flowmse_amd.data_module import SpecTransform
    return SpecTransform()


def _signal(seed, n, std=0.1):
    return torch.from_numpy(synth.normal(seed, 9, (1, n), std))


def _cut(S, K, H):
    """Trailing chunks [K,1,F,TC] of a spectrogram [1,1,F,Tg]: stream frame u = t + P, zeros before frame 0."""
    padded = torch.nn.functional.pad(S, (TC - H, max(K * H - S.size(3), 0)))
    return torch.cat([padded[..., k * H:k * H + TC] for k in range(K)], dim=0).contiguous()


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("Ls", [256, 128 * 16 * 3, 20000, 128 * 16 * 3 + 127])
def test_rows_are_slices_of_analyze(dm, Ls):
    """3, 49, 157 and 49 frames: one right-aligned chunk; T = 3 H + 1 (a last chunk of one real frame, whose right reflection
    reads back to sample L - 256 at L = 6144 and to L - 129 at L = 6271); a length that is no multiple of anything."""
    sig = _signal(Ls % 97, Ls).cuda()
    whole = dm.analyze(sig, 0.37)                                                  # [1,1,256,Tpad], zeros past T
    T = Ls // 128 + 1
    for H in (16, 4, 64):
        K, P, Tg = plan_trailing(T, TC, H, 0)
        got = dm.analyze_trailing(sig, TC, H, 0.37)
        torch.cuda.synchronize()
        assert got.shape == (K, 1, 256, TC) and got.dtype == torch.complex64
        want = _cut(whole[..., :T], K, H)
        assert torch.equal(got, want), (Ls, H, [k for k in range(K) if not torch.equal(got[k], want[k])])
        if P:
            assert bool((got[0][..., :P] == 0).all())                              # the zero frames before the recording
        if Tg > T:
            assert bool((got[-1][..., TC - (Tg - T):] == 0).all())                 # and past its end
        assert float(got[-1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("H,X", [(16, 4), (8, 8), (4, 2), (32, 0)], ids=lambda v: str(v))
def test_seams_match_the_float64_blend(dm, H, X):
    """Independent random chunks, K = 5: neighbouring chunks disagree completely wherever they overlap, so a wrong weight or a
    wrong owner is visible far above the bound.  With a fade, the blend with w = i / X and the rule with ownership
    k = (t + X - 1) // H (frame k H - X left to chunk k - 1 unblended) are each asserted to be > 1e-3 away.  At X = 0 neither
    wrong rule exists: there is no faded frame, and (t - 1) // H hands frame k H to chunk k - 1 at frame Tc, which no chunk
    has -- there the wrong owner is k = (t + H // 2) // H instead (the later half of every hop from the next chunk's lead)."""
    K = 5
    P, Tg = TC - H, K * H
    chunks = C.c64(synth.synth_spectrogram(30 + H + X, K, 256, TC)).cuda()
    length = 128 * (Tg - 1) - 37
    got = dm.synthesize_trailing(chunks, H, X, length, 0.7)
    blend = blend_trailing_reference(chunks, H, X)
    want = dm.synthesize(torch.from_numpy(blend).to(torch.complex64).cuda(), length, 0.7)
    torch.cuda.synchronize()
    assert got.shape == (1, length) and torch.isfinite(got).all() and float(want.abs().max()) > 0
    err = C.rel_l2(got.cpu(), want.cpu())
    print(f"trailing seams H {H} X {X} K {K}: rel-L2 vs synthesize(float64 blend) = {err:.3e}")
    assert err < ISTFT_TOL
    c = chunks.cpu().numpy().astype(np.complex128)

    def rule(owner, weight):
        out = np.empty_like(blend)
        for t in range(Tg):
            k = min(owner(t), K - 1)
            j = t - k * H + P
            b = c[k, 0, :, j]
            if k > 0 and t < k * H:
                a = c[k - 1, 0, :, j + H]
                b = a + weight(t - (k * H - X)) * (b - a)
            out[0, 0, :, t] = b
        return out

    assert np.array_equal(rule(lambda t: (t + X) // H, lambda i: (i + 0.5) / X), blend)
    wrongs = [rule(lambda t: (t + X - 1) // H, lambda i: (i + 0.5) / X), rule(lambda t: (t + X) // H, lambda i: i / X)] if X \
        else [rule(lambda t: (t + H // 2) // H, lambda i: 1.0)]
    for wrong in wrongs:
        off = dm.synthesize(torch.from_numpy(wrong).to(torch.complex64).cuda(), length, 0.7)
        assert C.rel_l2(got.cpu(), off.cpu()) > 1e-3


@pytest.mark.parametrize("H,X", [(16, 4), (8, 8), (4, 2), (32, 0), (64, 0)], ids=lambda v: str(v))
def test_chunks_cut_from_one_spectrogram_synthesize_bit_for_bit(dm, H, X):
    K, _, Tg = plan_trailing(100, TC, H, X)
    S = C.c64(synth.synth_spectrogram(7, 1, 256, Tg)).cuda()
    chunks = _cut(S, K, H)
    for length in (128 * (Tg - 1), 128 * (Tg - 1) + 255, 12345):
        got, want = dm.synthesize_trailing(chunks, H, X, length, 1.3), dm.synthesize(S, length, 1.3)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (H, X, length)
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("hop,To", [(48, 16), (32, 32), (64, 0)], ids=lambda v: str(v))
def test_the_overlap_synthesis_is_the_trailing_synthesis_bit_for_bit(hop, To):
    """Overlap chunks ``hop`` apart are trailing chunks at H = hop, X = P = To whose frame origin lies To frames later: on
    independent random chunks, trailing sample n is overlap sample n + 128 To.  From n = 256 on: below that, the overlap
    stack's first To frames -- which the trailing recording does not have -- lie over the sample or in its block."""
    s, p = _lib.current_stream(), _lib.ptr
    K = 3
    chunks = C.c64(synth.synth_spectrogram(60 + hop, K, 256, TC)).cuda()
    over = torch.empty(128 * ((K - 1) * hop + TC - 1), device="cuda")
    trail = torch.empty(128 * (K * hop - 1), device="cuda")
    _lib.check(L.flowse_istft_decompress_chunks(p(chunks), K, TC, hop, FACTOR, EXPONENT, p(over), over.numel(), 0.7, s))
    _lib.check(L.flowse_istft_decompress_trailing(p(chunks), K, TC, hop, To, FACTOR, EXPONENT, p(trail), trail.numel(), 0.7, s))
    torch.cuda.synchronize()
    assert over.numel() == trail.numel() + 128 * To
    got, want = trail[256:], over[256 + 128 * To:]
    assert got.numel() > 0 and float(want.abs().max()) > 0
    assert torch.equal(got, want), (hop, To, int((got != want).nonzero()[0]))


def test_the_overlap_rows_are_trailing_rows(dm):
    """97 frames at Tc = 64, hop = H = 32: overlap chunk k holds the frames [32 k, 32 k + 64) that trailing chunk k + 1 holds."""
    sig = _signal(3, 128 * 96 + 127).cuda()
    over, trail = dm.analyze_chunks(sig, TC, 32, 0.37), dm.analyze_trailing(sig, TC, 32, 0.37)
    torch.cuda.synchronize()
    assert over.shape == (3, 1, 256, TC) and trail.shape == (4, 1, 256, TC)
    assert torch.equal(over, trail[1:]) and float(over[2].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 3
def test_refusals_return_a_status_name_the_entry_and_launch_nothing():
    s, p = _lib.current_stream(), _lib.ptr
    sig = _signal(1, 20000).cuda().reshape(-1)                                     # 157 frames: 10 chunks at H = 16
    rows = torch.full((10, 1, 256, 64), 7.0, dtype=torch.complex64, device="cuda")
    # (L, K, Tc, H)
    for Ls, K, Tc, H in [(20000, 9, 64, 16), (20000, 0, 64, 16), (20000, 65536, 64, 16), (200, 1, 64, 16), (20000, 10, 96, 16),
                         (20000, 10, 0, 16), (20000, 10, 64, 15), (20000, 79, 64, 2), (20000, 10, 64, 66), (20000, 10, 64, 0),
                         (20000, 10, -64, 16)]:
        assert L.flowse_stft_compress_trailing(p(sig), Ls, 1.0, p(rows), K, Tc, H, FACTOR, EXPONENT, s) == ERR_SHAPE, (Ls, K, Tc, H)
        assert b"flowse_stft_compress_trailing:" in L.flowse_last_error()
    assert b"H=0" in L.flowse_last_error() or b"Tc=-64" in L.flowse_last_error()   # the values are in the message
    assert L.flowse_stft_compress_trailing(None, 20000, 1.0, p(rows), 10, 64, 16, FACTOR, EXPONENT, s) == ERR_ARG
    assert L.flowse_stft_compress_trailing(p(sig), 20000, 1.0, None, 10, 64, 16, FACTOR, EXPONENT, s) == ERR_ARG
    assert b"flowse_stft_compress_trailing:" in L.flowse_last_error()

    chunks = torch.zeros(10, 1, 256, 64, dtype=torch.complex64, device="cuda")     # Tg = 160 at H = 16
    top = 128 * 159 + 255
    out = torch.full((top + 1,), 7.0, device="cuda")
    # (K, Tc, H, X, Lout, factor)
    for K, Tc, H, X, Lout, factor in [(0, 64, 16, 4, 1000, 0.15), (65536, 64, 16, 4, 1000, 0.15), (10, 96, 16, 4, 1000, 0.15),
                                      (10, 64, 15, 4, 1000, 0.15), (10, 64, 2, 0, 1000, 0.15), (10, 64, 66, 0, 1000, 0.15),
                                      (10, 64, 16, -1, 1000, 0.15), (10, 64, 16, 17, 1000, 0.15), (10, 64, 40, 30, 1000, 0.15),
                                      (10, 64, 16, 4, 0, 0.15), (10, 64, 16, 4, top + 1, 0.15), (10, 64, 16, 4, 1000, 0.0)]:
        rc = L.flowse_istft_decompress_trailing(p(chunks), K, Tc, H, X, factor, EXPONENT, p(out), Lout, 1.0, s)
        assert rc == ERR_SHAPE, (K, Tc, H, X, Lout, factor)
        assert b"flowse_istft_decompress_trailing:" in L.flowse_last_error()
    assert L.flowse_istft_decompress_trailing(None, 10, 64, 16, 4, FACTOR, EXPONENT, p(out), 1000, 1.0, s) == ERR_ARG
    assert L.flowse_istft_decompress_trailing(p(chunks), 10, 64, 16, 4, FACTOR, EXPONENT, None, 1000, 1.0, s) == ERR_ARG
    assert b"flowse_istft_decompress_trailing:" in L.flowse_last_error()

    row = torch.full((1, 1, 256, 64), 7.0, dtype=torch.complex64, device="cuda")
    lo, hi = 128 * (3 * 16 - 48) - 255 + 255, 128 * (3 * 16 + 15) + 255            # chunk 3 at H = 16 reads frames 0 .. 63
    assert lo == 0
    # (buf, s0, k, Tc, H, L_total)
    for buf, s0, k, Tc, H, Ltot in [(sig[:hi - 1], 0, 3, 64, 16, -1),              # the last frame's last sample has not arrived
                                    (sig[1:hi], 1, 3, 64, 16, -1),                 # frame 0 reflects about sample 0
                                    (sig[:hi], 0, 3, 64, 16, 200), (sig[:hi], 0, 3, 64, 16, hi - 1), (sig[:hi], 0, -1, 64, 16, -1),
                                    (sig[:hi], 0, 2 ** 36, 64, 16, -1), (sig[:hi], 0, 3, 96, 16, -1), (sig[:hi], 0, 3, 64, 15, -1),
                                    (sig[:hi], 0, 3, 64, 2, -1), (sig[:hi], 0, 3, 64, 66, -1), (sig[:hi], -1, 3, 64, 16, -1),
                                    (sig[:hi], 0, 3, 64, 16, -2)]:
        rc = L.flowse_stft_compress_trailing_window(p(buf.clone()), s0, buf.numel(), 1.0, k, Tc, H, Ltot, p(row), FACTOR,
                                                    EXPONENT, s)
        assert rc == ERR_SHAPE, (s0, k, Tc, H, Ltot)
        assert b"flowse_stft_compress_trailing_window" in L.flowse_last_error()
    assert L.flowse_stft_compress_trailing_window(p(sig[:hi - 1].clone()), 0, hi - 1, 1.0, 3, 64, 16, -1, p(row), FACTOR,
                                                  EXPONENT, s) == ERR_SHAPE
    assert str(hi - 1).encode() in L.flowse_last_error()                           # the numbers are in the message
    assert L.flowse_stft_compress_trailing_window(None, 0, hi, 1.0, 3, 64, 16, -1, p(row), FACTOR, EXPONENT, s) == ERR_ARG
    assert L.flowse_stft_compress_trailing_window(p(sig), 0, hi, 1.0, 3, 64, 16, -1, None, FACTOR, EXPONENT, s) == ERR_ARG
    assert b"flowse_stft_compress_trailing_window" in L.flowse_last_error()

    ch = [C.c64(synth.synth_spectrogram(50 + i, 1, 256, 64)).cuda()[0] for i in range(3)]
    k, H, X = 3, 16, 4
    e0, e1 = 128 * (k * H - X) - 255, 128 * ((k + 1) * H - X) - 255
    wout = torch.full((e1 - e0 + 1000,), 7.0, device="cuda")
    # (prev2, prev, cur, k, Tc, H, X, last, L, e0, n_out, factor)
    bad = [(None, ch[1], ch[2], k, 64, H, X, 0, 0, e0, e1 - e0 + 1, 0.15),        # one sample into the frames that wait for chunk k+1
           (None, None, ch[2], k, 64, H, X, 0, 0, e0, e1 - e0, 0.15),             # chunk k-1 is needed and not given
           (None, ch[1], ch[2], k, 64, H, X, 0, 0, e0 - 128 * (H - X), 500, 0.15),     # a faded frame of chunk k-1: needs k-2
           (ch[0], ch[1], ch[2], k, 64, H, X, 0, 0, e0 - 128 * (2 * H - X), 500, 0.15),    # a faded frame of chunk k-2: a 4th chunk
           (None, ch[1], ch[2], k, 64, H, X, 1, e1 - 1, e0, e1 - e0, 0.15),       # past L with the last flag
           (None, ch[1], ch[2], k, 64, H, X, 1, 128 * ((k + 1) * H - 1) + 256, e0, 500, 0.15),      # L past the frames
           (None, ch[1], ch[2], k, 96, H, X, 0, 0, e0, 500, 0.15), (None, ch[1], ch[2], k, 64, 15, X, 0, 0, e0, 500, 0.15),
           (None, ch[1], ch[2], k, 64, H, 17, 0, 0, e0, 500, 0.15), (None, ch[1], ch[2], k, 64, H, -1, 0, 0, e0, 500, 0.15),
           (None, ch[1], ch[2], k, 64, 40, 30, 0, 0, e0, 500, 0.15), (None, ch[1], ch[2], -1, 64, H, X, 0, 0, e0, 500, 0.15),
           (None, ch[1], ch[2], k, 64, H, X, 0, 0, e0, 0, 0.15), (None, ch[1], ch[2], k, 64, H, X, 0, 0, -1, 500, 0.15),
           (None, ch[1], ch[2], k, 64, H, X, 0, 0, e0, 500, 0.0)]
    for p2, p1, cur, kk, tc, hh, xx, last, Ltot, a, n, factor in bad:
        rc = L.flowse_istft_decompress_trailing_window(p(p2), p(p1), p(cur), kk, tc, hh, xx, last, Ltot, factor, EXPONENT,
                                                       p(wout), a, n, 1.0, s)
        assert rc == ERR_SHAPE, (kk, tc, hh, xx, last, Ltot, a, n, factor)
        assert b"flowse_istft_decompress_trailing_window" in L.flowse_last_error()
    assert L.flowse_istft_decompress_trailing_window(None, p(ch[1]), p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wout), e0,
                                                     e1 - e0 + 1, 1.0, s) == ERR_SHAPE
    msg = L.flowse_last_error()
    assert f"[{e0}, {e1 + 1})".encode() in msg and b"k+1" in msg
    assert L.flowse_istft_decompress_trailing_window(None, p(ch[1]), None, k, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wout), e0, 500,
                                                     1.0, s) == ERR_ARG
    assert L.flowse_istft_decompress_trailing_window(None, p(ch[1]), p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, None, e0, 500,
                                                     1.0, s) == ERR_ARG
    assert b"flowse_istft_decompress_trailing_window" in L.flowse_last_error()

    torch.cuda.synchronize()
    assert bool((rows == 7.0).all()) and bool((out == 7.0).all()) and bool((row == 7.0).all()) and bool((wout == 7.0).all())
    # afterwards the stream is usable: each entry once, legally
    _lib.check(L.flowse_stft_compress_trailing(p(sig), 20000, 1.0, p(rows), 10, 64, 16, FACTOR, EXPONENT, s))
    _lib.check(L.flowse_istft_decompress_trailing(p(chunks), 10, 64, 16, 4, FACTOR, EXPONENT, p(out), top, 1.0, s))
    _lib.check(L.flowse_stft_compress_trailing_window(p(sig[:hi].clone()), 0, hi, 1.0, 3, 64, 16, -1, p(row), FACTOR, EXPONENT, s))
    _lib.check(L.flowse_istft_decompress_trailing_window(None, p(ch[1]), p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wout),
                                                         e0, e1 - e0, 1.0, s))
    torch.cuda.synchronize()
    assert float(rows[3].abs().max()) > 0 and torch.equal(row[0], rows[3])
    assert bool((out[:-1] == 0.0).all()) and float(out[-1]) == 7.0
    assert not bool((wout[:e1 - e0] == 7.0).any()) and bool((wout[e1 - e0:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 4
def _samples_read(t0, t1, Ls, closed):
    """[lo, hi): the sample indices the frames [t0, t1) read, from the STFT's definition (centre padding of 255, reflection at
    both ends) -- enumerated, not from the library's closed form."""
    t = np.arange(t0, t1)
    j = np.abs(128 * t[:, None] + np.arange(510)[None, :] - 255)
    if closed:
        j = np.where(j >= Ls, 2 * (Ls - 1) - j, j)
    return int(j.min()), int(j.max()) + 1


def _chunks_read(a, b, K, H, X, last, Tg):
    """The chunks the seam rule reads for the output samples [a, b): enumerated over the frames that lie over a sample
    (frame t covers [128 t - 255, 128 t + 254]; after the last chunk only the frames < Tg exist)."""
    need = set()
    for t in range(0, (b + 255) // 128 + 1):
        if 128 * t - 255 > b - 1 or 128 * t + 254 < a or (last and t >= Tg):
            continue
        k = (t + X) // H
        if last:
            k = min(k, K - 1)
        need.add(k)
        if k > 0 and t < k * H:
            need.add(k - 1)
    return need


@pytest.mark.parametrize("H,X", [(16, 4), (4, 2)], ids=lambda v: str(v))
def test_window_entries_are_the_file_entries_from_the_smallest_windows(H, X):
    """A recording of K = 5 chunks (T = 5 H - 1 frames).  STFT: every chunk from the smallest window that holds what its real
    frames read -- open where the recording has that many samples, closed always -- equals the file entry's row; one sample
    fewer at either end is refused.  iSTFT: the range [E_{k-1}, E_k) (the last: up to L) from exactly the chunks the seam rule
    reads equals the file entry's samples; a needed chunk withheld, or one sample more while open, is refused.  (16, 4) needs
    one previous chunk, (4, 2) two.  One call of each entry repeats chunk 3 with k and s0 / e0 moved up by 2^32 chunks."""
    s, p = _lib.current_stream(), _lib.ptr
    K, P = 5, TC - H
    Ls = 128 * (5 * H - 2) + 77
    T = Ls // 128 + 1
    assert plan_trailing(T, TC, H, X) == (K, P, K * H)
    sig = _signal(5 + H, Ls).cuda().reshape(-1)
    whole = torch.empty(K, 1, 256, TC, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_stft_compress_trailing(p(sig), Ls, 0.37, p(whole), K, TC, H, FACTOR, EXPONENT, s))
    BIG = 2 ** 32

    def stft(buf, s0, k, Ltot, row):
        return L.flowse_stft_compress_trailing_window(p(buf), s0, buf.numel(), 0.37, k, TC, H, Ltot, p(row), FACTOR, EXPONENT, s)

    done = []
    for k in range(K):
        for closed in (False, True):
            n_k = 128 * (k * H + H - 1) + 255
            if not closed and n_k > Ls:
                continue
            t0, t1 = max(k * H - P, 0), (min(k * H + H, T) if closed else k * H + H)
            lo, hi = _samples_read(t0, t1, Ls, closed)
            assert closed or hi == n_k
            row = torch.full((1, 1, 256, TC), 7.0, dtype=torch.complex64, device="cuda")
            _lib.check(stft(sig[lo:hi].clone(), lo, k, Ls if closed else -1, row))
            torch.cuda.synchronize()
            assert torch.equal(row[0], whole[k]), (k, closed)
            done.append((k, closed, lo > 0))
            assert stft(sig[lo:hi - 1].clone(), lo, k, Ls if closed else -1, row) == ERR_SHAPE
            if lo:
                assert stft(sig[lo + 1:hi].clone(), lo + 1, k, Ls if closed else -1, row) == ERR_SHAPE
            torch.cuda.synchronize()
            assert torch.equal(row[0], whole[k])
    # at H = 4 every one of the five chunks reaches back to frame 0 (P = 60); at H = 16 the last starts at frame 16
    assert (K - 1, True, H == 16) in done and (0, False, False) in done and not any(d[:2] == (K - 1, False) for d in done)
    # past 2^31: the first chunk that reads no frame that reflects about sample 0 (all Tc of its frames are real, as every
    # frame of a chunk 2^32 hops later is), open, against the same samples at k + 2^32 and s0 + 128 H 2^32
    k_s = -(-(P + 2) // H)
    lo, hi = _samples_read(k_s * H - P, k_s * H + H, 0, False)
    assert lo > 0 and hi == 128 * (k_s * H + H - 1) + 255
    sig2 = _signal(9 + H, hi + 300).cuda().reshape(-1)
    K2 = plan_trailing(sig2.numel() // 128 + 1, TC, H, X)[0]
    whole2 = torch.empty(K2, 1, 256, TC, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_stft_compress_trailing(p(sig2), sig2.numel(), 0.37, p(whole2), K2, TC, H, FACTOR, EXPONENT, s))
    row = torch.full((1, 1, 256, TC), 7.0, dtype=torch.complex64, device="cuda")
    _lib.check(stft(sig2[lo:hi].clone(), lo + 128 * H * BIG, k_s + BIG, -1, row))
    torch.cuda.synchronize()
    assert torch.equal(row[0], whole2[k_s]) and float(row.abs().max()) > 0 and lo + 128 * H * BIG > 2 ** 31
    assert stft(sig2[lo:hi - 1].clone(), lo + 128 * H * BIG, k_s + BIG, -1, row) == ERR_SHAPE
    assert stft(sig2[lo + 1:hi].clone(), lo + 1 + 128 * H * BIG, k_s + BIG, -1, row) == ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(row[0], whole2[k_s])

    # the inverse, on independent random chunks
    chunks = C.c64(synth.synth_spectrogram(40 + H + X, K, 256, TC)).cuda()
    want = torch.empty(Ls, device="cuda")
    _lib.check(L.flowse_istft_decompress_trailing(p(chunks), K, TC, H, X, FACTOR, EXPONENT, p(want), Ls, 0.7, s))
    rows = [chunks[k].clone() for k in range(K)]                                   # separate allocations, as a live session holds them

    def istft(p2, p1, cur, k, last, out, e0, n):
        return L.flowse_istft_decompress_trailing_window(p(p2), p(p1), p(cur), k, TC, H, X, int(last), Ls if last else 0, FACTOR,
                                                         EXPONENT, p(out), e0, n, 0.7, s)

    E = [0] + [max(128 * ((k + 1) * H - X) - 255, 0) for k in range(K - 1)] + [Ls]
    parts, depth = [], set()
    for k in range(K):
        last = k == K - 1
        e0, e1 = E[k], E[k + 1]
        assert e1 > e0
        need = _chunks_read(e0, e1, K, H, X, last, K * H)
        assert max(need) == k and min(need) >= k - 2
        depth.add(k - min(need))
        prev = rows[k - 1] if k - 1 in need else None
        prev2 = rows[k - 2] if k - 2 in need else None
        out = torch.full((e1 - e0,), 7.0, device="cuda")
        _lib.check(istft(prev2, prev, rows[k], k, last, out, e0, e1 - e0))
        parts.append(out)
        spare = torch.full((e1 - e0 + 1,), 7.0, device="cuda")
        if not last:                                                               # sample E_k lies under frame (k + 1) H - X
            assert istft(prev2, prev, rows[k], k, last, spare, e0, e1 - e0 + 1) == ERR_SHAPE
        if prev is not None:
            assert istft(prev2, None, rows[k], k, last, spare, e0, e1 - e0) == ERR_SHAPE
        if prev2 is not None:
            assert istft(None, prev, rows[k], k, last, spare, e0, e1 - e0) == ERR_SHAPE
            assert b"flowse_istft_decompress_trailing_window" in L.flowse_last_error()
        torch.cuda.synchronize()
        assert bool((spare == 7.0).all())
        if k == 3:                                                                 # the same chunks as chunks 1..3 + 2^32
            far = torch.full((e1 - e0,), 7.0, device="cuda")
            _lib.check(istft(prev2, prev, rows[k], k + BIG, False, far, e0 + 128 * H * BIG, e1 - e0))
            torch.cuda.synchronize()
            assert torch.equal(far, out) and e0 + 128 * H * BIG > 2 ** 31
    got = torch.cat(parts)
    torch.cuda.synchronize()
    assert got.shape == (Ls,) and torch.equal(got, want) and float(want.abs().max()) > 0
    assert max(depth) == (1 if H - X >= 3 else 2)
