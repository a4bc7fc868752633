"""Ensembles of draws: the mean of ``D`` draws of the sampler and a number that says how far the draws differ.

An opt-in mode (``--samples D`` of ``flowmse_amd.enhance --pool`` and ``flowmse_amd.evaluate``), NOT the reference's
computation: the reference draws once per file (evaluate.py:97-136).  Every output of the sampler is one draw from a
generative model; with keyed noise it is a function of (weights, file, seed).  Here a row is sampled ``D`` times under
independent keyed streams and the finish stage reduces over the draws on the device.

Definitions, all fixed:

* noise key: draw ``d >= 0`` of a row whose key is ``k`` uses ``draw_key(k, d)`` (``util.noise``); ``draw_key(k, 0) == k``, so
  draw 0 is the single draw of a run without ``--samples``.  Keyed noise only;
* linear spectrum of a draw: for a stack of ``K`` chunks ``[K,1,256,Tc]`` that start ``hop`` frames apart, ``Z_d`` is
  ``spec_back`` of the seam rule (``chunked.blend_chunks_reference``) on the compressed values of draw ``d``.  The blend is
  done per draw BEFORE the decompression: decompression is not linear, so the order is part of the definition;
* mean output: ``M = (1 / D) sum_d Z_d`` summed in the order ``d = 0 .. D-1``; the waveform is ``istft(M, length) * scale``
  over all ``Tg = (K - 1) hop + Tc`` frames.  The iSTFT is linear, so this is the mean of the ``D`` waveforms;
* per-frame tracks (``D >= 2``), over all 256 bins and every one of the ``Tg`` frames:
  ``dev[t] = sum_f sum_d |Z_d[f,t] - M[f,t]|^2 / (D - 1)`` and ``pow[t] = sum_f |M[f,t]|^2``.  The deviations are formed in
  a second pass from the finished mean, never as ``sum |Z_d|^2 - D |M|^2``: a small term is not found by cancellation;
* agreement of a file and channel: ``10 log10(sum_t pow[t] / sum_t dev[t])`` over the real frames ``t < L // 128 + 1``, in
  float64 on the host from the two tracks; ``inf`` when the draws are identical.  High: the draws agree.  Around 0 dB or
  below: the output is mostly the draw.

On the device this is ``flowse_istft_decompress_ensemble`` (``SpecTransform.synthesize_ensemble``); ``ensemble_reference``
below is the same in float64 on the CPU.
"""
import argparse
import math

import numpy as np
import torch

from flowmse_amd.chunked import blend_chunks_reference
from flowmse_amd.util.noise import draw_key

HOP = 128
# The draws one flowse_istft_decompress_ensemble call reduces: FLOWSE_MAX_DRAWS of the library, restated so that the command
# lines parse (and print their help) without loading it; tests/test_ensemble_host.py holds the two equal.
MAX_DRAWS = 64


def check_draws(draws):
    """``draws`` as a tuple of ints: 1..``MAX_DRAWS`` distinct draw indices, each ``>= 0``, else ``ValueError``."""
    out = tuple(int(d) for d in draws)
    if not 1 <= len(out) <= MAX_DRAWS or min(out) < 0 or len(set(out)) != len(out):
        raise ValueError(f"draws must be 1..{MAX_DRAWS} distinct indices >= 0, got {tuple(draws)}")
    return out


def draw_keys(key, draws):
    """The noise keys of the draws ``draws`` of a row whose key is ``key``."""
    return [draw_key(key, d) for d in draws]


def samples_arg(v):
    """``--samples``: an integer in 1..``MAX_DRAWS``."""
    try:
        d = int(v)
    except ValueError:
        d = 0
    if not 1 <= d <= MAX_DRAWS:
        raise argparse.ArgumentTypeError(f"--samples must be 1..{MAX_DRAWS}, got {v!r}")
    return d


def agreement_db(dev, pow, L):
    """``10 log10(sum pow / sum dev)`` over the real frames ``t < L // 128 + 1`` of the two tracks (1-D, numpy or torch), in
    float64; ``inf`` when ``sum dev == 0``."""
    T = int(L) // HOP + 1
    dev = np.asarray(dev.detach().cpu() if torch.is_tensor(dev) else dev, dtype=np.float64).reshape(-1)[:T]
    pw = np.asarray(pow.detach().cpu() if torch.is_tensor(pow) else pow, dtype=np.float64).reshape(-1)[:T]
    num, den = float(pw.sum()), float(dev.sum())
    if den == 0.0:
        return math.inf
    return 10.0 * math.log10(num / den) if num > 0.0 else -math.inf


def agreements(tracks, L):
    """``agreement_db`` of every stack of ``tracks`` [S, 2, Tg] (device tensor: ONE read-back)."""
    t = tracks.detach().cpu().numpy() if torch.is_tensor(tracks) else np.asarray(tracks)
    return [agreement_db(s[0], s[1], L) for s in t]


def ensemble_reference(chunks, S, D, hop, length, scale=1.0, *, stack_stride=None, draw_stride=None, K=None, factor=0.15,
                       exponent=0.5):
    """The definitions of the module docstring in float64 on the CPU.  ``chunks``: complex ``[rows,1,256,Tc]`` (numpy or
    torch), chunk ``k`` of draw ``d`` of stack ``s`` at row ``s * stack_stride + d * draw_stride + k`` (default: contiguous
    ``[S][D][K]``, ``K = rows // (S D)``).  Returns ``(waveform float64 [S, length], tracks float64 [S, 2, Tg])`` as numpy;
    the tracks are ``None`` for ``D == 1``."""
    from flowmse_amd.data_module import SpecTransform
    c = chunks.detach().cpu().numpy() if torch.is_tensor(chunks) else np.asarray(chunks)
    c = c.astype(np.complex128)
    S, D, hop = int(S), int(D), int(hop)
    rows, _, F, Tc = c.shape
    K = rows // (S * D) if K is None else int(K)
    stack_stride = D * K if stack_stride is None else int(stack_stride)
    draw_stride = K if draw_stride is None else int(draw_stride)
    if S < 1 or D < 1 or K < 1 or (S - 1) * stack_stride + (D - 1) * draw_stride + K > rows:
        raise ValueError(f"ensemble_reference: S={S} D={D} K={K} stack_stride={stack_stride} draw_stride={draw_stride} "
                         f"does not fit {rows} rows")
    st = SpecTransform(spec_factor=factor, spec_abs_exponent=exponent)
    Tg = (K - 1) * hop + Tc
    window = torch.hann_window(st.n_fft, periodic=True, dtype=torch.float64)
    waves = np.empty((S, int(length)), dtype=np.float64)
    tracks = None if D == 1 else np.empty((S, 2, Tg), dtype=np.float64)
    for s in range(S):
        Z = []
        for d in range(D):
            r0 = s * stack_stride + d * draw_stride
            blended = blend_chunks_reference(c[r0:r0 + K], hop)[0, 0]               # [F, Tg], per draw, compressed
            Z.append(st.spec_back(torch.from_numpy(blended)).numpy())
        M = Z[0].copy()
        for d in range(1, D):
            M += Z[d]
        M /= D
        waves[s] = torch.istft(torch.from_numpy(M), n_fft=st.n_fft, hop_length=st.hop_length, window=window, center=True,
                               length=int(length)).numpy() * float(scale)
        if tracks is not None:
            tracks[s, 0] = sum((np.abs(z - M) ** 2).sum(axis=0) for z in Z) / (D - 1)  # second pass, from the finished mean
            tracks[s, 1] = (np.abs(M) ** 2).sum(axis=0)
    return waves, tracks
