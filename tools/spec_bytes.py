#!/usr/bin/env python3
"""Output bytes, refusals and launch times of the STFT / iSTFT entries (flowmse_amd/csrc/spec.hip), for comparing two builds of
the library.

    FLOWSE_LIB_PATH=<build A>/libflowse_hip.so python tools/spec_bytes.py a.json
    FLOWSE_LIB_PATH=<build B>/libflowse_hip.so python tools/spec_bytes.py b.json      # fresh process each
    cmp a.json b.json
    python tools/spec_bytes.py --time --parent DIR [--runs 3] [--raw runs.jsonl] [--out table.md]

Bytes: every ``flowse_stft_compress*`` / ``flowse_istft_decompress*`` entry on fixed seeded inputs, the SHA-256 of what it wrote
into a buffer pre-filled with 7 -- at the geometries of the GPU tests (Tc = 64 with hop 48 / To 16, with (H, X) = (16, 4),
(8, 8), (32, 0), and Tc = 256 / To 32), K = 1, 2 and 5, the first and last windows of an open and of a closed recording, a
window past sample 2^31, R = 1 and the largest R of each table, D = 1 and D = 4 with tracks -- and for a list of refused calls
the status, ``flowse_last_error()`` and the hash of the untouched output.

``--time``: microseconds per launch of single entries at the sizes of a 30 s recording (L = 480000), one live window and the
row tables at R = 8 and 16.  A sample is 200 launches between two device events after a warm-up of that shape, ending in a
synchronise; 3 samples per child process; the children alternate parent-this, ``--runs`` times, each under its own
``timeout``, and the first failure ends the tool.  Both trees are timed through this tree's Python with ``FLOWSE_LIB_PATH``
naming the library of ``--parent DIR``.  The table gives per entry the median and the range over all samples of each tree.

A tool, not a test: it pins nothing.  Seconds on one GPU.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FACTOR, EXPONENT = 0.15, 0.5
OVERLAP = [(64, 48), (256, 224)]                        # (Tc, hop): To 16 and 32
TRAILING = [(64, 16, 4), (64, 8, 8), (64, 32, 0)]       # (Tc, H, X)
BIG = 2 ** 32                                           # chunks: moves a window far past sample 2^31


class Entries:
    """The library's entries on torch tensors; every output is pre-filled with 7, so a refusal shows as an untouched buffer."""

    def __init__(self):
        import torch
        import _cases
        from flowmse_amd import _lib
        from flowmse_amd.util import synth
        self.torch, self.lib, self.L, self.synth, self.c64 = torch, _lib, _lib.lib, synth, _cases.c64
        self.s, self.p = _lib.current_stream(), _lib.ptr

    def signal(self, seed, n):
        return self.torch.from_numpy(self.synth.normal(seed, 9, (n,), 0.1)).cuda()

    def spec(self, seed, rows, Tc):
        return self.c64(self.synth.synth_spectrogram(seed, rows, 256, Tc)).cuda()

    def rows_out(self, R, Tw):
        return self.torch.full((R, 1, 256, Tw), 7.0, dtype=self.torch.complex64, device="cuda")

    def wave_out(self, *shape):
        return self.torch.full(shape, 7.0, device="cuda")

    def spec_rows(self, rows):
        table = (self.lib.flowse_spec_row * len(rows))()
        for d, (sig, frame0, scale) in zip(table, rows):
            d.sig, d.L, d.frame0, d.scale_in = sig.data_ptr(), sig.numel(), frame0, scale
        return table

    def window_rows(self, rows):
        table = (self.lib.flowse_window_row * len(rows))()
        for d, (buf, s0, frame0, L_total, scale) in zip(table, rows):
            d.buf, d.s0, d.n, d.frame0, d.L_total, d.scale_in = buf.data_ptr(), s0, buf.numel(), frame0, L_total, scale
        return table

    def window_outs(self, rows):
        table = (self.lib.flowse_window_out * len(rows))()
        for d, (p2, p1, cur, out, k, L, e0, n_out, last, scale) in zip(table, rows):
            d.prev2_c64, d.prev_c64 = (None if p2 is None else p2.data_ptr()), (None if p1 is None else p1.data_ptr())
            d.cur_c64, d.out, d.k, d.L, d.e0, d.n_out, d.last, d.scale_out = cur.data_ptr(), out.data_ptr(), k, L, e0, n_out, last, scale
        return table


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def stft_window_of(sig, t0, t1, closed):
    """(buf, s0): the samples the frames [t0, t1) read, to the end of the recording when it is closed."""
    lo = max(128 * t0 - 255, 0)
    return (sig[lo:], lo) if closed else (sig[lo:128 * (t1 - 1) + 255], lo)


def final_before(k, H, X, shift):
    """The first sample that is not final after chunk k of an open recording: it lies under frame (k + 1) H - X (+ shift)."""
    return max(128 * ((k + 1) * H - X + shift) - 255, 0)


def byte_cases(E, out):
    L, p, s, torch = E.L, E.p, E.s, E.torch

    def ok(name, rc, *tensors):
        assert rc == 0, (name, rc, L.flowse_last_error())
        torch.cuda.synchronize()
        out[name] = {"sha256": [sha(t) for t in tensors]}

    # ---- the plain pair
    for B in (1, 3):
        n = 20000
        sig = torch.stack([E.signal(10 + b, n) for b in range(B)])
        spec = E.rows_out(B, 192)
        ok(f"stft_compress/B{B}", L.flowse_stft_compress(p(sig), B, n, 0.37, p(spec), n // 128 + 1, 192, FACTOR, EXPONENT, s), spec)
        src, wave = E.spec(20 + B, B, 192), E.wave_out(B, n)
        ok(f"istft_decompress/B{B}", L.flowse_istft_decompress(p(src), B, 192, 192, FACTOR, EXPONENT, p(wave), n, 0.7, s), wave)

    # ---- overlap chunks: the file pair, stacks, ensembles, the window pair
    for Tc, hop in OVERLAP:
        To, tag = Tc - hop, f"Tc{Tc}_hop{hop}"
        for K in (1, 2, 5):
            Tg = (K - 1) * hop + Tc
            n = 128 * (Tg - 4) + 77
            sig, rows = E.signal(30 + K, n), E.rows_out(K, Tc)
            ok(f"stft_compress_chunks/{tag}/K{K}", L.flowse_stft_compress_chunks(p(sig), n, 0.37, p(rows), K, Tc, hop, FACTOR, EXPONENT, s), rows)
            chunks = E.spec(40 + K, K, Tc)
            for Lout in (128 * (Tg - 1) + 255, n):
                wave = E.wave_out(Lout)
                ok(f"istft_decompress_chunks/{tag}/K{K}/Lout{Lout}",
                   L.flowse_istft_decompress_chunks(p(chunks), K, Tc, hop, FACTOR, EXPONENT, p(wave), Lout, 0.7, s), wave)
        K, Tg = 2, hop + Tc
        for S in (1, 3):
            chunks, wave = E.spec(50 + S, S * K, Tc), E.wave_out(S, 128 * (Tg - 1))
            ok(f"istft_decompress_stacks/{tag}/S{S}",
               L.flowse_istft_decompress_stacks(p(chunks), S, K, Tc, hop, FACTOR, EXPONENT, p(wave), wave.shape[1], 0.7, s), wave)
        S = 2
        for D in (1, 4):
            chunks, wave = E.spec(60 + D, S * D * K, Tc), E.wave_out(S, 128 * (Tg - 1))
            tracks = E.wave_out(S, 2, Tg) if D > 1 else None
            ok(f"istft_decompress_ensemble/{tag}/stack_major/D{D}",
               L.flowse_istft_decompress_ensemble(p(chunks), S, D, K, Tc, hop, D * K, K, FACTOR, EXPONENT, p(wave), wave.shape[1],
                                                  0.7, p(tracks), s), *([wave] if tracks is None else [wave, tracks]))
        chunks, wave, tracks = E.spec(65, 4 * S, Tc), E.wave_out(S, 128 * (Tc - 1)), E.wave_out(S, 2, Tc)
        ok(f"istft_decompress_ensemble/{tag}/draw_major/D4",
           L.flowse_istft_decompress_ensemble(p(chunks), S, 4, 1, Tc, hop, 1, S, FACTOR, EXPONENT, p(wave), wave.shape[1], 0.7,
                                              p(tracks), s), wave, tracks)
        # a recording of K = 5 chunks, arriving: the first and the last window, open and closed, and one far away
        K = 5
        Tg = (K - 1) * hop + Tc
        n = 128 * (Tg - 4) + 77
        T = n // 128 + 1
        sig, chunks = E.signal(70, n), [E.spec(71 + k, 1, Tc) for k in range(K)]
        for k in (0, K - 1):
            for closed in (False, True):
                if not closed and 128 * (k * hop + Tc - 1) + 255 > n:
                    continue
                buf, s0 = stft_window_of(sig, k * hop, k * hop + Tc, closed)
                buf, row = buf.clone(), E.rows_out(1, Tc)
                ok(f"stft_compress_window/{tag}/k{k}/{'closed' if closed else 'open'}",
                   L.flowse_stft_compress_window(p(buf), s0, buf.numel(), 0.37, k * hop, Tc, n if closed else -1, p(row), FACTOR,
                                                 EXPONENT, s), row)
        for k, last in ((0, False), (1, False), (K - 1, False), (K - 1, True)):
            e0 = final_before(k - 1, hop, To, To) if k else 0
            e1 = n if last else final_before(k, hop, To, To)
            p1, p2, wave = (chunks[k - 1] if k >= 1 else None), (chunks[k - 2] if k >= 2 else None), E.wave_out(e1 - e0)
            ok(f"istft_decompress_window/{tag}/k{k}/{'last' if last else 'open'}",
               L.flowse_istft_decompress_window(p(p2), p(p1), p(chunks[k]), k, Tc, hop, int(last), n if last else 0, FACTOR,
                                                EXPONENT, p(wave), e0, e1 - e0, 0.7, s), wave)
        k = 3
        buf, s0 = stft_window_of(sig, k * hop, k * hop + Tc, False)
        buf, row = buf.clone(), E.rows_out(1, Tc)
        ok(f"stft_compress_window/{tag}/far", L.flowse_stft_compress_window(p(buf), s0 + 128 * hop * BIG, buf.numel(), 0.37, (k + BIG) * hop,
                                                                             Tc, -1, p(row), FACTOR, EXPONENT, s), row)
        e0, e1 = final_before(k - 1, hop, To, To), final_before(k, hop, To, To)
        wave = E.wave_out(e1 - e0)
        ok(f"istft_decompress_window/{tag}/far",
           L.flowse_istft_decompress_window(p(chunks[1]), p(chunks[2]), p(chunks[3]), k + BIG, Tc, hop, 0, 0, FACTOR, EXPONENT, p(wave),
                                            e0 + 128 * hop * BIG, e1 - e0, 0.7, s), wave)
        # the row tables: one row and the most the table holds, rows that differ in signal, window, chunk and length
        sigs = [E.signal(80 + i, n - 1000 * i) for i in range(3)]
        for R in (1, 64):
            table, rows = E.spec_rows([(sigs[r % 3], (r * 7) % (T - 8), 0.3 + 0.01 * r) for r in range(R)]), E.rows_out(R, Tc)
            ok(f"stft_compress_rows/{tag}/R{R}", L.flowse_stft_compress_rows(table, R, Tc, p(rows), FACTOR, EXPONENT, s), rows)
        for R in (1, 16):
            wins, keep = [], []
            for r in range(R):
                k, closed = r % 4, r % 3 == 2
                buf, s0 = stft_window_of(sigs[r % 3], k * hop, k * hop + Tc, closed)
                keep.append(buf.clone())
                wins.append((keep[-1], s0, k * hop, sigs[r % 3].numel() if closed else -1, 0.3 + 0.01 * r))
            rows = E.rows_out(R, Tc)
            ok(f"stft_compress_window_rows/{tag}/R{R}",
               L.flowse_stft_compress_window_rows(E.window_rows(wins), R, Tc, p(rows), FACTOR, EXPONENT, s), rows)
            outs, waves = [], []
            for r in range(R):
                k, last = (r % 4, False) if r % 5 else (K - 1, True)
                e0 = final_before(k - 1, hop, To, To) if k else 0
                e1 = n if last else final_before(k, hop, To, To) - 100 * (r % 3)
                waves.append(E.wave_out(e1 - e0))
                outs.append((chunks[k - 2] if k >= 2 else None, chunks[k - 1] if k >= 1 else None, chunks[k], waves[-1], k,
                             n if last else 0, e0, e1 - e0, int(last), 0.5 + 0.01 * r))
            ok(f"istft_decompress_window_rows/{tag}/R{R}",
               L.flowse_istft_decompress_window_rows(E.window_outs(outs), R, Tc, hop, FACTOR, EXPONENT, s), *waves)

    # ---- trailing chunks: the file pair and the window pair
    for Tc, H, X in TRAILING:
        tag = f"Tc{Tc}_H{H}_X{X}"
        for K in (1, 2, 5):
            n = 128 * (K * H - 2) + 77
            sig, rows = E.signal(90 + K, n), E.rows_out(K, Tc)
            ok(f"stft_compress_trailing/{tag}/K{K}", L.flowse_stft_compress_trailing(p(sig), n, 0.37, p(rows), K, Tc, H, FACTOR, EXPONENT, s), rows)
            chunks = E.spec(100 + K, K, Tc)
            for Lout in (128 * (K * H - 1) + 255, n):
                wave = E.wave_out(Lout)
                ok(f"istft_decompress_trailing/{tag}/K{K}/Lout{Lout}",
                   L.flowse_istft_decompress_trailing(p(chunks), K, Tc, H, X, FACTOR, EXPONENT, p(wave), Lout, 0.7, s), wave)
        K = 5
        n = 128 * (K * H - 2) + 77
        T = n // 128 + 1
        sig, chunks = E.signal(110, n), [E.spec(111 + k, 1, Tc) for k in range(K)]
        for k in (0, K - 1):
            for closed in (False, True):
                if not closed and 128 * (k * H + H - 1) + 255 > n:
                    continue
                buf, s0 = stft_window_of(sig, max(k * H - (Tc - H), 0), k * H + H, closed)
                buf, row = buf.clone(), E.rows_out(1, Tc)
                ok(f"stft_compress_trailing_window/{tag}/k{k}/{'closed' if closed else 'open'}",
                   L.flowse_stft_compress_trailing_window(p(buf), s0, buf.numel(), 0.37, k, Tc, H, n if closed else -1, p(row), FACTOR,
                                                          EXPONENT, s), row)
        for k, last in ((0, False), (2, False), (K - 1, False), (K - 1, True)):
            e0 = final_before(k - 1, H, X, 0) if k else 0
            e1 = n if last else final_before(k, H, X, 0)
            if e1 <= e0:
                continue
            p1, p2, wave = (chunks[k - 1] if k >= 1 else None), (chunks[k - 2] if k >= 2 else None), E.wave_out(e1 - e0)
            ok(f"istft_decompress_trailing_window/{tag}/k{k}/{'last' if last else 'open'}",
               L.flowse_istft_decompress_trailing_window(p(p2), p(p1), p(chunks[k]), k, Tc, H, X, int(last), n if last else 0, FACTOR,
                                                         EXPONENT, p(wave), e0, e1 - e0, 0.7, s), wave)
        k = -(-(Tc - H + 2) // H)                       # the first chunk none of whose frames reflects about sample 0
        sig2 = E.signal(120, 128 * (k * H + H - 1) + 255)
        buf, s0 = stft_window_of(sig2, k * H - (Tc - H), k * H + H, False)
        buf, row = buf.clone(), E.rows_out(1, Tc)
        ok(f"stft_compress_trailing_window/{tag}/far",
           L.flowse_stft_compress_trailing_window(p(buf), s0 + 128 * H * BIG, buf.numel(), 0.37, k + BIG, Tc, H, -1, p(row), FACTOR,
                                                  EXPONENT, s), row)
        k = 3
        e0, e1 = final_before(k - 1, H, X, 0), final_before(k, H, X, 0)
        wave = E.wave_out(e1 - e0)
        ok(f"istft_decompress_trailing_window/{tag}/far",
           L.flowse_istft_decompress_trailing_window(p(chunks[1]), p(chunks[2]), p(chunks[3]), k + BIG, Tc, H, X, 0, 0, FACTOR, EXPONENT,
                                                     p(wave), e0 + 128 * H * BIG, e1 - e0, 0.7, s), wave)


def refusal_cases(E, out):
    """Calls the GPU tests expect to be refused: the status, the text and the untouched output of each."""
    L, p, s, torch = E.L, E.p, E.s, E.torch
    sig = E.signal(1, 20000)
    rows, wave = E.rows_out(10, 64), E.wave_out(30000)
    ch = [E.spec(50 + i, 1, 64) for i in range(3)]
    chunks = E.spec(9, 10, 64)
    hi = 128 * 63 + 255
    k, H, X, hop, To = 3, 16, 4, 48, 16
    t0, t1 = final_before(k - 1, H, X, 0), final_before(k, H, X, 0)
    o0, o1 = final_before(k - 1, hop, To, To), final_before(k, hop, To, To)
    wr = lambda *a: E.window_rows([a])
    wo = lambda *a: E.window_outs([a])
    calls = {
        "stft_compress/null": lambda: L.flowse_stft_compress(None, 1, 20000, 1.0, p(rows), 157, 192, FACTOR, EXPONENT, s),
        "stft_compress/T": lambda: L.flowse_stft_compress(p(sig), 1, 20000, 1.0, p(rows), 156, 192, FACTOR, EXPONENT, s),
        "istft_decompress/Lout": lambda: L.flowse_istft_decompress(p(chunks), 1, 64, 64, FACTOR, EXPONENT, p(wave), 128 * 63 + 256, 1.0, s),
        "istft_decompress/factor": lambda: L.flowse_istft_decompress(p(chunks), 1, 64, 64, 0.0, EXPONENT, p(wave), 1000, 1.0, s),
        "stft_compress_chunks/K": lambda: L.flowse_stft_compress_chunks(p(sig), 20000, 1.0, p(rows), 2, 64, 48, FACTOR, EXPONENT, s),
        "stft_compress_chunks/hop": lambda: L.flowse_stft_compress_chunks(p(sig), 20000, 1.0, p(rows), 10, 64, 31, FACTOR, EXPONENT, s),
        "istft_decompress_chunks/hop": lambda: L.flowse_istft_decompress_chunks(p(chunks), 10, 64, 65, FACTOR, EXPONENT, p(wave), 1000, 1.0, s),
        "istft_decompress_chunks/null": lambda: L.flowse_istft_decompress_chunks(p(chunks), 10, 64, 48, FACTOR, EXPONENT, None, 1000, 1.0, s),
        "istft_decompress_stacks/S": lambda: L.flowse_istft_decompress_stacks(p(chunks), 0, 2, 64, 48, FACTOR, EXPONENT, p(wave), 1000, 1.0, s),
        "istft_decompress_ensemble/tracks_at_D1": lambda: L.flowse_istft_decompress_ensemble(
            p(chunks), 1, 1, 2, 64, 48, 2, 2, FACTOR, EXPONENT, p(wave), 1000, 1.0, p(wave), s),
        "istft_decompress_ensemble/alias": lambda: L.flowse_istft_decompress_ensemble(
            p(chunks), 2, 2, 2, 64, 48, 2, 2, FACTOR, EXPONENT, p(wave), 1000, 1.0, None, s),
        "stft_compress_rows/R": lambda: L.flowse_stft_compress_rows(E.spec_rows([(sig, 0, 1.0)]), 65, 64, p(rows), FACTOR, EXPONENT, s),
        "stft_compress_rows/frame0": lambda: L.flowse_stft_compress_rows(E.spec_rows([(sig, -1, 1.0)]), 1, 64, p(rows), FACTOR, EXPONENT, s),
        "stft_compress_rows/L": lambda: L.flowse_stft_compress_rows(E.spec_rows([(sig[:200], 0, 1.0)]), 1, 64, p(rows), FACTOR, EXPONENT, s),
        "stft_compress_window/short": lambda: L.flowse_stft_compress_window(p(sig), 0, hi - 1, 1.0, 0, 64, -1, p(rows), FACTOR, EXPONENT, s),
        "stft_compress_window/reflects": lambda: L.flowse_stft_compress_window(p(sig), 1, hi, 1.0, 0, 64, -1, p(rows), FACTOR, EXPONENT, s),
        "stft_compress_window/L_total": lambda: L.flowse_stft_compress_window(p(sig), 0, hi, 1.0, 0, 64, hi - 1, p(rows), FACTOR, EXPONENT, s),
        "istft_decompress_window/waits": lambda: L.flowse_istft_decompress_window(
            None, p(ch[1]), p(ch[2]), k, 64, hop, 0, 0, FACTOR, EXPONENT, p(wave), o0, o1 - o0 + 1, 1.0, s),
        "istft_decompress_window/prev_withheld": lambda: L.flowse_istft_decompress_window(
            None, None, p(ch[2]), k, 64, hop, 0, 0, FACTOR, EXPONENT, p(wave), o0, o1 - o0, 1.0, s),
        "istft_decompress_window/needs_prev2": lambda: L.flowse_istft_decompress_window(
            None, p(ch[1]), p(ch[2]), k, 64, hop, 0, 0, FACTOR, EXPONENT, p(wave), o0 - 128 * hop, 500, 1.0, s),
        "istft_decompress_window/past_L": lambda: L.flowse_istft_decompress_window(
            None, p(ch[1]), p(ch[2]), k, 64, hop, 1, o1 - 1, FACTOR, EXPONENT, p(wave), o0, o1 - o0, 1.0, s),
        "istft_decompress_window/hop": lambda: L.flowse_istft_decompress_window(
            None, p(ch[1]), p(ch[2]), k, 64, 31, 0, 0, FACTOR, EXPONENT, p(wave), o0, 500, 1.0, s),
        "istft_decompress_window/null": lambda: L.flowse_istft_decompress_window(
            None, p(ch[1]), None, k, 64, hop, 0, 0, FACTOR, EXPONENT, p(wave), o0, 500, 1.0, s),
        "stft_compress_window_rows/R": lambda: L.flowse_stft_compress_window_rows(wr(sig, 0, 0, -1, 1.0), 17, 64, p(rows), FACTOR, EXPONENT, s),
        "stft_compress_window_rows/row_short": lambda: L.flowse_stft_compress_window_rows(
            wr(sig[:hi - 1], 0, 0, -1, 1.0), 1, 64, p(rows), FACTOR, EXPONENT, s),
        "istft_decompress_window_rows/row_waits": lambda: L.flowse_istft_decompress_window_rows(
            wo(None, ch[1], ch[2], wave, k, 0, o0, o1 - o0 + 1, 0, 1.0), 1, 64, hop, FACTOR, EXPONENT, s),
        "istft_decompress_window_rows/row_hop": lambda: L.flowse_istft_decompress_window_rows(
            wo(None, ch[1], ch[2], wave, k, 0, o0, 500, 0, 1.0), 1, 64, 31, FACTOR, EXPONENT, s),
        "istft_decompress_window_rows/R": lambda: L.flowse_istft_decompress_window_rows(
            wo(None, ch[1], ch[2], wave, k, 0, o0, 500, 0, 1.0), 0, 64, hop, FACTOR, EXPONENT, s),
        "stft_compress_trailing/K": lambda: L.flowse_stft_compress_trailing(p(sig), 20000, 1.0, p(rows), 9, 64, 16, FACTOR, EXPONENT, s),
        "stft_compress_trailing/H_odd": lambda: L.flowse_stft_compress_trailing(p(sig), 20000, 1.0, p(rows), 10, 64, 15, FACTOR, EXPONENT, s),
        "stft_compress_trailing/Tc": lambda: L.flowse_stft_compress_trailing(p(sig), 20000, 1.0, p(rows), 10, 96, 16, FACTOR, EXPONENT, s),
        "istft_decompress_trailing/X": lambda: L.flowse_istft_decompress_trailing(p(chunks), 10, 64, 16, 17, FACTOR, EXPONENT, p(wave), 1000, 1.0, s),
        "istft_decompress_trailing/H_plus_X": lambda: L.flowse_istft_decompress_trailing(
            p(chunks), 10, 64, 40, 30, FACTOR, EXPONENT, p(wave), 1000, 1.0, s),
        "istft_decompress_trailing/Lout": lambda: L.flowse_istft_decompress_trailing(
            p(chunks), 10, 64, 16, 4, FACTOR, EXPONENT, p(wave), 128 * 159 + 256, 1.0, s),
        "stft_compress_trailing_window/short": lambda: L.flowse_stft_compress_trailing_window(
            p(sig), 0, hi - 1, 1.0, 3, 64, 16, -1, p(rows), FACTOR, EXPONENT, s),
        "stft_compress_trailing_window/k": lambda: L.flowse_stft_compress_trailing_window(
            p(sig), 0, hi, 1.0, 2 ** 36, 64, 16, -1, p(rows), FACTOR, EXPONENT, s),
        "istft_decompress_trailing_window/waits": lambda: L.flowse_istft_decompress_trailing_window(
            None, p(ch[1]), p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wave), t0, t1 - t0 + 1, 1.0, s),
        "istft_decompress_trailing_window/prev_withheld": lambda: L.flowse_istft_decompress_trailing_window(
            None, None, p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wave), t0, t1 - t0, 1.0, s),
        "istft_decompress_trailing_window/needs_prev2": lambda: L.flowse_istft_decompress_trailing_window(
            None, p(ch[1]), p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wave), t0 - 128 * (H - X), 500, 1.0, s),
        "istft_decompress_trailing_window/fourth_chunk": lambda: L.flowse_istft_decompress_trailing_window(
            p(ch[0]), p(ch[1]), p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wave), t0 - 128 * (2 * H - X), 500, 1.0, s),
        "istft_decompress_trailing_window/past_L": lambda: L.flowse_istft_decompress_trailing_window(
            None, p(ch[1]), p(ch[2]), k, 64, H, X, 1, t1 - 1, FACTOR, EXPONENT, p(wave), t0, t1 - t0, 1.0, s),
        "istft_decompress_trailing_window/L_past_frames": lambda: L.flowse_istft_decompress_trailing_window(
            None, p(ch[1]), p(ch[2]), k, 64, H, X, 1, 128 * ((k + 1) * H - 1) + 256, FACTOR, EXPONENT, p(wave), t0, 500, 1.0, s),
        "istft_decompress_trailing_window/overlap_geometry": lambda: L.flowse_istft_decompress_trailing_window(
            None, p(ch[1]), p(ch[2]), k, 65, 33, 4, 0, 0, FACTOR, EXPONENT, p(wave), t0, 500, 1.0, s),
        "istft_decompress_trailing_window/null": lambda: L.flowse_istft_decompress_trailing_window(
            None, p(ch[1]), p(ch[2]), k, 64, H, X, 0, 0, FACTOR, EXPONENT, None, t0, 500, 1.0, s),
    }
    for name, call in calls.items():
        rc = call()
        assert rc != 0, name
        out["refused/" + name] = {"status": rc, "error": L.flowse_last_error().decode(errors="replace")}
    torch.cuda.synchronize()
    out["refused/outputs"] = {"sha256": [sha(rows), sha(wave)]}


def bytes_main(path):
    E = Entries()
    assert E.torch.cuda.is_available(), "needs a GPU"
    out = {}
    byte_cases(E, out)
    refusal_cases(E, out)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {path}")


# ---------------------------------------------------------------------------------------------------- --time
LAUNCHES, SAMPLES = 200, 3


def time_cases(E):
    """name -> a callable that makes ONE launch of one entry, at sizes a user runs."""
    L, p, s = E.L, E.p, E.s
    n = 480000                                          # 30 s at 16 kHz: T = 3751 frames
    T = n // 128 + 1
    sig = E.signal(1, n)
    cases = {}
    Tpad = -(-T // 64) * 64
    spec, wave = E.rows_out(1, Tpad), E.wave_out(n)
    cases["stft_compress 30s"] = lambda: L.flowse_stft_compress(p(sig), 1, n, 0.37, p(spec), T, Tpad, FACTOR, EXPONENT, s)
    cases["istft_decompress 30s"] = lambda: L.flowse_istft_decompress(p(spec), 1, Tpad, Tpad, FACTOR, EXPONENT, p(wave), n, 0.7, s)
    Tc, hop, To = 256, 224, 32
    K = -(-(T - To) // hop)
    rows = E.spec(2, K, Tc)
    cases["stft_compress_chunks 30s 256/32"] = lambda: L.flowse_stft_compress_chunks(p(sig), n, 0.37, p(rows), K, Tc, hop, FACTOR, EXPONENT, s)
    cases["istft_decompress_chunks 30s 256/32"] = lambda: L.flowse_istft_decompress_chunks(p(rows), K, Tc, hop, FACTOR, EXPONENT, p(wave), n, 0.7, s)
    H, X = 16, 4
    Kt = -(-T // H)
    trows = E.spec(3, Kt, 64)
    cases["stft_compress_trailing 30s 64/16/4"] = lambda: L.flowse_stft_compress_trailing(p(sig), n, 0.37, p(trows), Kt, 64, H, FACTOR, EXPONENT, s)
    cases["istft_decompress_trailing 30s 64/16/4"] = lambda: L.flowse_istft_decompress_trailing(
        p(trows), Kt, 64, H, X, FACTOR, EXPONENT, p(wave), n, 0.7, s)
    # one window of a live session, chunk k = 5 (256/32) and k = 20 (64/16/4)
    k = 5
    buf, s0 = stft_window_of(sig, k * hop, k * hop + Tc, False)
    buf, row, ch = buf.clone(), E.rows_out(1, Tc), [E.spec(4 + i, 1, Tc) for i in range(3)]
    e0, e1 = final_before(k - 1, hop, To, To), final_before(k, hop, To, To)
    cases["stft_compress_window 256/32"] = lambda: L.flowse_stft_compress_window(
        p(buf), s0, buf.numel(), 0.37, k * hop, Tc, -1, p(row), FACTOR, EXPONENT, s)
    cases["istft_decompress_window 256/32"] = lambda: L.flowse_istft_decompress_window(
        p(ch[0]), p(ch[1]), p(ch[2]), k, Tc, hop, 0, 0, FACTOR, EXPONENT, p(wave), e0, e1 - e0, 0.7, s)
    kt = 20
    tbuf, ts0 = stft_window_of(sig, kt * H - (64 - H), kt * H + H, False)
    tbuf, trow, tch = tbuf.clone(), E.rows_out(1, 64), [E.spec(8 + i, 1, 64) for i in range(3)]
    f0, f1 = final_before(kt - 1, H, X, 0), final_before(kt, H, X, 0)
    cases["stft_compress_trailing_window 64/16/4"] = lambda: L.flowse_stft_compress_trailing_window(
        p(tbuf), ts0, tbuf.numel(), 0.37, kt, 64, H, -1, p(trow), FACTOR, EXPONENT, s)
    cases["istft_decompress_trailing_window 64/16/4"] = lambda: L.flowse_istft_decompress_trailing_window(
        p(tch[0]), p(tch[1]), p(tch[2]), kt, 64, H, X, 0, 0, FACTOR, EXPONENT, p(wave), f0, f1 - f0, 0.7, s)
    for R in (8, 16):
        out_rows = E.rows_out(R, Tc)
        table = E.spec_rows([(sig, 100 * r, 0.3) for r in range(R)])
        cases[f"stft_compress_rows R{R} Tw256"] = lambda table=table, R=R, o=out_rows: L.flowse_stft_compress_rows(
            table, R, Tc, p(o), FACTOR, EXPONENT, s)
        wtable = E.window_rows([(buf, s0, k * hop, -1, 0.3)] * R)
        cases[f"stft_compress_window_rows R{R} 256/32"] = lambda t=wtable, R=R, o=out_rows: L.flowse_stft_compress_window_rows(
            t, R, Tc, p(o), FACTOR, EXPONENT, s)
        waves = [E.wave_out(e1 - e0) for _ in range(R)]
        otable = E.window_outs([(ch[0], ch[1], ch[2], waves[r], k, 0, e0, e1 - e0, 0, 0.7) for r in range(R)])
        cases[f"istft_decompress_window_rows R{R} 256/32"] = lambda t=otable, R=R, w=waves: L.flowse_istft_decompress_window_rows(
            t, R, Tc, hop, FACTOR, EXPONENT, s)
        stacks, swave = E.spec(12 + R, R * 2, Tc), E.wave_out(R, 128 * (hop + Tc - 1))
        cases[f"istft_decompress_stacks S{R} K2 256/32"] = lambda c=stacks, R=R, w=swave: L.flowse_istft_decompress_stacks(
            p(c), R, 2, Tc, hop, FACTOR, EXPONENT, p(w), w.shape[1], 0.7, s)
    return cases


def time_arm():
    E = Entries()
    torch = E.torch
    assert torch.cuda.is_available(), "spec_bytes.py --time measures on the GPU; there is no CPU timing"
    for name, call in time_cases(E).items():
        for _ in range(20):                                          # warm-up of this shape
            assert call() == 0, (name, E.L.flowse_last_error())
        torch.cuda.synchronize()
        for sample in range(SAMPLES):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LAUNCHES):
                call()
            b.record()
            torch.cuda.synchronize()
            print(json.dumps(dict(entry=name, sample=sample, us=1e3 * a.elapsed_time(b) / LAUNCHES)), flush=True)


def time_main(a):
    trees = [("parent", os.path.join(os.path.abspath(a.parent), "flowmse_amd", "libflowse_hip.so")),
             ("this", os.path.join(ROOT, "flowmse_amd", "libflowse_hip.so"))]
    rows = []
    for run in range(a.runs):
        for tree, lib in trees:
            assert os.path.exists(lib), lib
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--time-arm"],
                               env=dict(os.environ, FLOWSE_LIB_PATH=lib), cwd=ROOT, capture_output=True, text=True)
            if r.returncode != 0:                                   # a failed child ends the tool: nothing more is started
                print(r.stdout[-2000:], r.stderr[-3000:], file=sys.stderr)
                return r.returncode
            rows += [dict(json.loads(line), tree=tree, run=run) for line in r.stdout.splitlines() if line.startswith("{")]
            print(f"run {run} tree {tree}: done", flush=True)
    if a.raw:
        with open(a.raw, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    lines = ["| entry | parent us per launch: median (min .. max) | this: median (min .. max) | this median inside the parent's range |",
             "|---|---|---|---|"]
    for name in dict.fromkeys(r["entry"] for r in rows):
        us = {tree: [r["us"] for r in rows if (r["entry"], r["tree"]) == (name, tree)] for tree, _ in trees}
        med = {t: statistics.median(v) for t, v in us.items()}
        inside = "yes" if min(us["parent"]) <= med["this"] <= max(us["parent"]) else ("below" if med["this"] < min(us["parent"]) else "ABOVE")
        lines.append(f"| {name} | " + " | ".join(f"{med[t]:.2f} ({min(us[t]):.2f} .. {max(us[t]):.2f})" for t in ("parent", "this"))
                     + f" | {inside} |")
    text = "\n".join(lines) + f"\n\n{a.runs} alternating child processes per tree, {SAMPLES} samples of {LAUNCHES} launches each\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_json", nargs="?", help="where the hashes go")
    ap.add_argument("--time", action="store_true", help="time single entries against the library of --parent")
    ap.add_argument("--time-arm", action="store_true", help="internal: time the library FLOWSE_LIB_PATH names in this process")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="time limit of one child process in seconds")
    ap.add_argument("--out", default=None)
    ap.add_argument("--raw", default=None)
    a = ap.parse_args()
    if a.time_arm:
        return time_arm()
    if a.time:
        if not a.parent:
            ap.error("--time needs --parent DIR")
        return time_main(a)
    if not a.out_json:
        ap.error("give the file the hashes go to")
    return bytes_main(a.out_json)


if __name__ == "__main__":
    sys.exit(main())
