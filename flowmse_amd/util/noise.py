"""Keyed prior noise: the host restatement of ``csrc/noise.hip`` and the utterance keys.

The stream is a public contract ("Keyed noise stream"): for the row of utterance key ``k`` under
``seed``, bin ``f``, frame ``t``

    (w0, w1, w2, w3) = Philox4x32-10(counter = (t >> 1, f, lo32(k), hi32(k)), key = (lo32(seed), hi32(seed)))
    (w_a, w_b)       = (w0, w1) at even t, (w2, w3) at odd t
    u1 = ((w_a >> 9) + 0.5) * 2**-23,   u2 = (w_b >> 8) * 2**-24
    z  = sqrt(-log(u1)) * exp(2 pi i u2)                     complex standard normal, E|z|^2 = 1

so the value at (f, t) depends on nothing but (seed, k, f, t): not on the batch, the row, the padded length or the
order of calls.  ``t`` is the ABSOLUTE frame of the utterance: a row that starts at frame ``frame0`` of it (a chunk of a
long recording, ``flowmse_amd.chunked``) uses ``t = frame0 + index in the row``.  The kernel evaluates the last line in
fp32; this module evaluates it in float64.
"""
import hashlib
import os

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF
_MASK64 = 0xFFFFFFFFFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11).  ``ctr``: four 32-bit words, ``key``: two; each an int or an integer numpy
    array (arrays broadcast).  Returns the four output words as uint64 arrays holding 32-bit values (Python ints for
    all-int input)."""
    scalar = all(isinstance(v, (int, np.integer)) for v in tuple(ctr) + tuple(key))
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(_MASK32) for v in ctr]
    k = [np.asarray(v, dtype=np.uint64) & np.uint64(_MASK32) for v in key]
    m0, m1, mask, s32 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1), np.uint64(_MASK32), np.uint64(32)
    for r in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
    return tuple(int(v) for v in c) if scalar else tuple(c)


def check_frame0(frame0, B):
    """The per-row frame offsets of the keyed stream as a list of B ints: each even (an odd offset would pair the Philox
    words of a frame differently than the offset-free stream does) and >= 0, else ``ValueError``."""
    frame0 = [int(v) for v in (frame0.reshape(-1).tolist() if hasattr(frame0, "reshape") else frame0)]
    if len(frame0) != B:
        raise ValueError(f"frame0: {len(frame0)} offsets for {B} rows")
    if any(v < 0 or v % 2 for v in frame0):
        raise ValueError(f"frame0: every offset must be even and >= 0, got {frame0}")
    return frame0


def keyed_noise_reference(keys, seed, F, T, frame0=None):
    """The noise of the stream above in float64: complex128 array [B, 1, F, T] for the B utterance keys ``keys``.
    ``frame0`` (one even offset >= 0 per key): row b holds frames ``frame0[b] .. frame0[b] + T - 1`` of its key's stream."""
    keys = [int(k) & _MASK64 for k in np.asarray(keys, dtype=np.uint64).reshape(-1).tolist()]
    seed = int(seed) & _MASK64
    F, T = int(F), int(T)
    frame0 = [0] * len(keys) if frame0 is None else check_frame0(frame0, len(keys))
    t0 = np.arange(T, dtype=np.uint64)[None, :]
    f = np.arange(F, dtype=np.uint64)[:, None]
    odd = (t0 & np.uint64(1)).astype(bool)                     # the offsets are even: parity is the row's own
    out = np.empty((len(keys), 1, F, T), dtype=np.complex128)
    for b, k in enumerate(keys):
        t = t0 + np.uint64(frame0[b])
        w = philox4x32_10((t >> np.uint64(1), f, k & _MASK32, k >> 32), (seed & _MASK32, seed >> 32))
        wa = np.where(odd, w[2], w[0])
        wb = np.where(odd, w[3], w[1])
        u1 = ((wa >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        u2 = (wb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-np.log(u1))
        out[b, 0] = r * (np.cos(2.0 * np.pi * u2) + 1j * np.sin(2.0 * np.pi * u2))
    return out


def utterance_key(name):
    """64-bit key of an utterance: the 8-byte BLAKE2b digest of the file's base name, little-endian.  Depends on the
    name only -- not on the directory, the listing, or the position in it."""
    return int.from_bytes(hashlib.blake2b(os.path.basename(name).encode(), digest_size=8).digest(), "little")


# ---------------------------------------------------------------------------------------------- flow-matching loss draws
# The objective of ``VFModel._step`` draws a time and a noise tensor per row.  Both come from the stream above, so a loss
# depends on (weights, file name, seed, draw index) only ("Loss draws on the keyed stream").
LOSS_TIME_BIN = 0xFFFFFFFF       # counter word 1 of a time draw: a bin index of the noise stream never reaches it
LOSS_SEED_XOR = 0x6C6F7373       # "loss": the facade's Philox seed of the loss is seed ^ this, apart from the sampler's x_T noise
_DRAW_MUL = 0x9E3779B97F4A7C15


def draw_key(key, k):
    """Row key of draw ``k`` of utterance ``key``: ``key ^ (k * 0x9E3779B97F4A7C15 mod 2**64)``; draw 0 is the key itself."""
    return (int(key) ^ ((int(k) * _DRAW_MUL) & _MASK64)) & _MASK64


def loss_seed(seed):
    """The Philox seed ``VFModel._step`` / ``evaluate --valid_loss`` use for the loss draws of run seed ``seed``."""
    return (int(seed) ^ LOSS_SEED_XOR) & _MASK64


def loss_times(keys, seed, T_rev, t_eps, draws=1):
    """The times of the flow-matching loss, float32 [len(keys), draws].  Draw ``k`` of key ``key`` reads word 0 of
    ``Philox4x32-10(counter = (k, 0xFFFFFFFF, lo32(key), hi32(key)), key = (lo32(seed), hi32(seed)))``,
    ``u01 = (w0 >> 8) * 2**-24``, and then the reference's expression (flowmse/model.py:132-133) in float32:
    ``t = min((1 - u01) * (T_rev - t_eps) + t_eps, T_rev)``.  ``t_eps <= 0`` raises: the field divides by t."""
    if not float(t_eps) > 0.0:
        raise ValueError(f"loss_times: t_eps must be > 0 (the vector field divides by t), got {t_eps}")
    if not float(T_rev) >= float(t_eps):
        raise ValueError(f"loss_times: T_rev must be >= t_eps, got T_rev={T_rev} t_eps={t_eps}")
    keys = np.asarray([int(k) & _MASK64 for k in np.asarray(keys, dtype=np.uint64).reshape(-1).tolist()], dtype=np.uint64)
    seed = int(seed) & _MASK64
    k = np.arange(int(draws), dtype=np.uint64)[None, :]
    w0 = philox4x32_10((k, LOSS_TIME_BIN, keys[:, None] & np.uint64(_MASK32), keys[:, None] >> np.uint64(32)),
                       (seed & _MASK32, seed >> 32))[0]
    w0 = np.broadcast_to(w0, (keys.shape[0], int(draws)))
    u01 = ((w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)      # 24 bits: exact
    span = np.float32(float(T_rev) - float(t_eps))             # the reference subtracts two Python floats
    t = (np.float32(1.0) - u01) * span + np.float32(t_eps)
    return np.minimum(t, np.float32(T_rev)).astype(np.float32)
