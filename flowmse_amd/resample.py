"""Sample-rate conversion on the device: recordings at 8 .. 192 kHz in and out of the 16 kHz network.

An opt-in step (``flowmse_amd.enhance --resample``); the reference reads 16 kHz files only.  Rational-ratio polyphase FIR
resampling, zero phase, DEFINED as what ``scipy.signal.resample_poly(x, up, down)`` computes with its defaults
(``window=("kaiser", 5.0)``, ``padtype="constant"``):

    g = gcd(sr_out, sr_in), up = sr_out / g, down = sr_in / g, R = max(up, down), half = 10 R
    h[k]  = up * firwin(2 half + 1, 1 / R, window=("kaiser", 5.0))[k],  k = 0 .. 2 half
    L_out = ceil(L up / down)
    out[n] = sum over m in [0, L) with |n down - m up| <= half of  x[m] h[half + n down - m up]

``R <= 1024`` after reduction: 8 / 11.025 / 12 / 22.05 / 24 / 32 / 44.1 / 48 / 88.2 / 96 / 176.4 / 192 kHz against 16 kHz,
both ways.  The taps come from the library (``flowse_resample_taps``, host only), the device path is one
``flowse_resample_poly`` launch (csrc/resample.hip), and ``resample_reference`` is the float64 restatement the tests hold
against scipy -- nothing here calls scipy.  ``n down`` passes 2^31 five minutes into a 44.1 kHz recording: every index is
a Python int or an int64.
"""
import ctypes as C
import math

import numpy as np
import torch

from flowmse_amd import _lib

MAX_RATE = 1024
_ROWS = 1 << 16                  # outputs per pass of resample_reference (bounds its [rows, P] work arrays)


def rational(sr_in, sr_out):
    """``(up, down)``, reduced, for a conversion from ``sr_in`` to ``sr_out`` Hz.  ``ValueError``, naming the two rates,
    for non-positive rates and for ratios beyond ``max(up, down) = 1024``."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample: sample rates must be positive, got {sr_in} Hz -> {sr_out} Hz")
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if max(up, down) > MAX_RATE:
        raise ValueError(f"resample: {sr_in} Hz -> {sr_out} Hz is the ratio {up}/{down}; supported up to "
                         f"max(up, down) = {MAX_RATE}")
    return up, down


def out_len(L, up, down):
    """``ceil(L up / down)``: the samples ``L`` input samples become."""
    return -((-int(L) * int(up)) // int(down))


def design_taps(up, down):
    """The ``2 half + 1`` taps ``h`` of a ratio (reduced or not) in float64, from ``flowse_resample_taps``."""
    n = int(_lib.lib.flowse_resample_num_taps(int(up), int(down)))
    if n < 0:
        _lib.check(-n)
    taps = np.empty(n, dtype=np.float64)
    _lib.check(_lib.lib.flowse_resample_taps(int(up), int(down), taps.ctypes.data_as(C.POINTER(C.c_double)), n))
    return taps


def resample_reference(x, sr_in, sr_out, n0=0, n1=None, m0=0):
    """Outputs ``n0 .. n1 - 1`` (default: all) of the formula above in float64, for a 1-D array ``x``.  The polyphase sum
    ``out[n] = sum_j H[p][j] x[q - j]`` with ``c = half + n down``, ``p = c mod up``, ``q = c div up``, built on
    ``design_taps``.  ``m0``: ``x[0]`` is sample ``m0`` of a longer signal -- a window far into a long recording from the
    slice its outputs touch, ``q(n0) - (P - 1) .. q(n1 - 1)``, or from there to the signal's end; samples outside ``x``
    are taken as zero."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError(f"resample_reference takes a 1-D array, got shape {x.shape}")
    up, down = rational(sr_in, sr_out)
    m0 = int(m0)
    L = m0 + x.shape[0]
    n1 = out_len(L, up, down) if n1 is None else int(n1)
    n0 = int(n0)
    if not 0 <= n0 <= n1 <= out_len(L, up, down):
        raise ValueError(f"resample_reference: outputs [{n0}, {n1}) of {out_len(L, up, down)}")
    if up == down:
        return x[n0 - m0:n1 - m0].copy()
    h = design_taps(up, down)
    half = (h.shape[0] - 1) // 2
    P = -(-h.shape[0] // up)
    H = np.zeros(up * P, dtype=np.float64)
    H[:h.shape[0]] = h
    H = np.ascontiguousarray(H.reshape(P, up).T)                   # H[p][j] = h[p + j up]
    j = np.arange(P, dtype=np.int64)
    out = np.empty(n1 - n0, dtype=np.float64)
    for a in range(n0, n1, _ROWS):
        c = half + np.arange(a, min(a + _ROWS, n1), dtype=np.int64) * down
        m = (c // up)[:, None] - j[None, :] - m0                   # index into x
        ok = (m >= 0) & (m < x.shape[0])
        xg = np.where(ok, x[np.where(ok, m, 0)], 0.0)
        out[a - n0:a - n0 + c.shape[0]] = np.einsum("ij,ij->i", H[c % up], xg)
    return out


def resample(sig, sr_in, sr_out):
    """float32 tensor ``[B, L]`` at ``sr_in`` Hz -> ``[B, ceil(L up / down)]`` at ``sr_out`` Hz, every row on its own.
    A HIP tensor: one ``flowse_resample_poly`` launch on the current stream, no host synchronisation.  A CPU tensor: the
    float64 reference rounded to float32 (the oracle composition).  Equal rates return ``sig`` itself."""
    up, down = rational(sr_in, sr_out)
    if up == down:
        return sig
    if sig.dim() != 2 or sig.dtype != torch.float32:
        raise ValueError(f"resample takes a float32 tensor [B, L], got {sig.dtype} {tuple(sig.shape)}")
    B, L = sig.shape
    if not sig.is_cuda:
        rows = [resample_reference(r.numpy(), sr_in, sr_out) for r in sig]
        return torch.from_numpy(np.stack(rows).astype(np.float32))
    sig = sig.contiguous()
    out = torch.empty(B, out_len(L, up, down), dtype=torch.float32, device=sig.device)
    with torch.cuda.device(sig.device):
        _lib.check(_lib.lib.flowse_resample_poly(_lib.ptr(sig), B, L, up, down, _lib.ptr(out), out.size(1),
                                                 _lib.current_stream()))
    return out
