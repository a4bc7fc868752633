"""Recordings of any length: one recording as equal, overlapping chunks of ordinary sampler rows.

An opt-in mode, NOT the reference's computation for a long file.  The reference (and every other sampler entry of this
package) treats an utterance as one ``[B,1,256,T]`` tensor: memory grows with the length, and GroupNorm statistics and
the 16-bin attention run over all frames, a context the network -- trained on crops of 256 frames
(flowmse/data_module.py:98,110) -- never saw on a minutes-long file.  Here the spectrogram of ONE recording is cut into
``K`` chunks of ``Tc`` frames that start ``hop = Tc - To`` frames apart; the chunks are sampled as rows of ordinary
``[b,1,256,Tc]`` calls, ``b <= batch``, with a workspace that depends on ``(batch, Tc)`` only; the sampled chunks are
cross-faded over their ``To`` shared frames and ONE inverse STFT makes the waveform.  Every chunk has its own GroupNorm
and attention context, so the result differs from the single-tensor path; it is pinned instead to the oracle
composition -- the oracle sampler per chunk plus the same cross-fade on the host (tests/test_gpu_chunked.py).

Geometry (``plan_chunks``): ``T = L // 128 + 1`` real frames; chunk ``k`` covers the recording's frames
``[k hop, k hop + Tc)``; ``K = 1`` if ``T <= Tc`` else ``ceil((T - To) / hop)``; ``Tg = (K - 1) hop + Tc`` frames in all,
those ``>= T`` zero as with ``pad_spec``.  The tail chunk is zero-padded, not right-aligned: the treatment a short file
gets today, with one hop everywhere.  ``To <= Tc / 2`` guarantees that at most two chunks cover a frame.

Seam rule (``blend_chunks_reference``; ``flowse_istft_decompress_chunks`` on the device): the recording's frame ``t``
belongs to chunk ``k = min(t // hop, K - 1)`` at ``j = t - k hop``; for ``k > 0`` and ``j < To`` its value is
``a + w (b - a)`` with ``a`` = chunk ``k - 1`` at frame ``j + hop``, ``b`` = chunk ``k`` at ``j``, ``w = (j + 0.5) / To``
-- a linear cross-fade of the COMPRESSED complex values, before ``spec_back``.

Noise: all chunks of a recording share its utterance key and address the keyed stream at their absolute frames
(``frame0 = k hop``), so two chunks start from the same ``x_T`` on the frames they share; an explicit ``z`` or the torch
generator gives one ``[1,1,256,Tg]`` draw that is sliced per chunk.

The defaults ``Tc = 256`` (the training crop) and ``To = 32`` are chosen values, not tuned ones: no released checkpoint is
at hand offline, so how the seams sound has not been judged.

A second opt-in geometry, trailing chunks (``plan_trailing``, ``blend_trailing_reference``, ``enhance_trailing``: a chunk that
slides by a small hop and keeps only its tail, for a live latency set by the hop), is described where it begins, below.
"""
import numpy as np
import torch

CHUNK_FRAMES, OVERLAP_FRAMES = 256, 32


def plan_chunks(T, Tc=CHUNK_FRAMES, To=OVERLAP_FRAMES):
    """``(K, hop, Tg)`` for ``T`` real frames cut into chunks of ``Tc`` frames overlapping by ``To`` (module docstring).
    ``ValueError`` unless ``T >= 1``, ``Tc`` a positive multiple of 64, ``To`` even and ``0 <= To <= Tc / 2``."""
    T, Tc, To = int(T), int(Tc), int(To)
    if T < 1:
        raise ValueError(f"plan_chunks: T must be >= 1, got {T}")
    if Tc < 64 or Tc % 64:
        raise ValueError(f"plan_chunks: chunk_frames must be a positive multiple of 64 (the network's frame padding), got {Tc}")
    if To % 2 or not 0 <= To <= Tc // 2:
        raise ValueError(f"plan_chunks: overlap_frames must be even (the keyed noise stream pairs frames) and in "
                         f"0..chunk_frames / 2 = {Tc // 2} (at most two chunks over a frame), got {To}")
    hop = Tc - To
    K = 1 if T <= Tc else -(-(T - To) // hop)
    return K, hop, (K - 1) * hop + Tc


def blend_chunks_reference(chunks, hop):
    """The seam rule in float64: chunks ``[K,1,F,Tc]`` (numpy or torch, complex) that start ``hop`` frames apart ->
    complex128 numpy ``[1,1,F,Tg]``.  Chunks cut from one spectrogram return it exactly (``b - a`` is an exact zero)."""
    c = chunks.detach().cpu().numpy() if torch.is_tensor(chunks) else np.asarray(chunks)
    c = c.astype(np.complex128)
    K, _, F, Tc = c.shape
    hop = int(hop)
    To = Tc - hop
    if not (1 <= hop <= Tc and To <= hop):
        raise ValueError(f"blend_chunks_reference: need Tc / 2 <= hop <= Tc, got Tc={Tc} hop={hop}")
    out = np.empty((1, 1, F, (K - 1) * hop + Tc), dtype=np.complex128)
    for k in range(K):                                   # a later chunk owns the frames it shares with the one before
        out[0, :, :, k * hop:k * hop + Tc] = c[k]
    w = (np.arange(To, dtype=np.float64) + 0.5) / max(To, 1)
    for k in range(1, K):
        a, b = c[k - 1][:, :, hop:], c[k][:, :, :To]
        out[0, :, :, k * hop:k * hop + To] = a + w * (b - a)
    return out


def _recording_noise(z, noise_key, Y_like, frames, who, what=""):
    """The one ``[1,1,F,frames]`` noise tensor of a recording when the noise is not keyed (explicit ``z`` or one draw from
    the process-wide generator), else None.  ``who`` / ``what``: the caller's name and its word for ``frames``."""
    if noise_key is not None:
        return None
    F = Y_like.shape[2]
    if z is None:
        return torch.randn_like(torch.empty(1, 1, F, frames, dtype=torch.complex64, device=Y_like.device))
    if tuple(z.shape) != (1, 1, F, frames):
        raise ValueError(f"{who}: z must be the recording's noise [1,1,{F},{frames}]{what}, got {tuple(z.shape)}")
    return z.to(Y_like.device)


def _enhance_rows(model, y, sched, K, *, who, pad, analyze, synthesize, blend, what="", batch, odesolver, z, noise_key, noise_seed,
                  VF_fn, device, as_tensor, **solver):
    """The body of ``enhance_long`` and ``enhance_trailing``: ``K`` rows of ``sched.Tc`` frames cut at ``sched.noise_frame0(k)``,
    sampled in groups of ``batch`` and put together.  Per geometry: ``analyze(y)`` -> the rows, ``synthesize(sample, norm)`` ->
    the waveform, both one HIP launch; ``blend(sample)`` -> the float64 seam rule; ``pad = (left, frames)``: the zero frames
    before the recording and the length of the stream the oracle path and the noise are cut from; ``solver``: ``N``,
    ``T_rev``, ``t_eps``."""
    from flowmse_amd.evaluate import _analyze, _fused_ok
    from flowmse_amd.sampling import get_white_box_solver
    Tc, L, (left, frames) = sched.Tc, y.size(1), pad
    cut = lambda x, ks: torch.cat([x[..., sched.noise_frame0(k):sched.noise_frame0(k) + Tc] for k in ks], dim=0)  # noqa: E731
    norm_factor = y.abs().max().item()
    y = y.to(device)
    fused = _fused_ok(model, [y], VF_fn)
    if fused:                      # the chunk rows straight from the samples: one HIP kernel, no global spectrogram
        Y = analyze(y / norm_factor)
        with torch.cuda.device(device):
            model.dnn.reserve(batch, Y.shape[2], Tc)     # the workspace of a full group, whatever K is
    else:
        S = _analyze(model, y / norm_factor, False, pad=False)
        Y = cut(torch.nn.functional.pad(S, (left, frames - left - S.size(3), 0, 0)), range(K))
    zg = _recording_noise(z, noise_key, Y, frames, who, what)
    field = VF_fn if VF_fn is not None else model
    rows = []
    for k0 in range(0, K, batch):
        k1 = min(k0 + batch, K)
        Yg = Y[k0:k1].contiguous()
        if zg is None:
            kw = dict(noise_keys=[noise_key] * (k1 - k0), noise_seed=noise_seed,
                      noise_frame0=[sched.noise_frame0(k) for k in range(k0, k1)])
        else:
            kw = dict(z=cut(zg, range(k0, k1)).contiguous())
        rows.append(get_white_box_solver(odesolver, model.ode, field, Y=Yg, Y_prior=Yg, **solver, **kw)()[0])
    sample = torch.cat(rows, dim=0)
    if fused:                      # seam rule + decompression + iSTFT + rescale: one HIP kernel
        x_hat = synthesize(sample, norm_factor).reshape(-1)
    else:
        spec = torch.from_numpy(blend(sample)).to(torch.complex64).to(sample.device)
        x_hat = (model.to_audio(spec.squeeze(), L) * norm_factor).reshape(-1)
    return x_hat if as_tensor else x_hat.cpu().numpy()


def enhance_long(model, y, chunk_frames=CHUNK_FRAMES, overlap_frames=OVERLAP_FRAMES, batch=8, N=5, T_rev=1.0, t_eps=0.03,
                 odesolver="euler", z=None, noise_key=None, noise_seed=0, VF_fn=None, device=None, as_tensor=False):
    """One recording of any length, chunked (module docstring).  y: float tensor [1, samples].  Returns the enhanced
    waveform (numpy), normalised by the recording's global ``max|y|`` like ``enhance_waveform``; with ``as_tensor`` the
    same values as a 1-D tensor left on the compute device (for a step that follows there, ``flowmse_amd.resample``).

    A recording whose padded frame count fits one chunk goes to ``evaluate.enhance_waveform`` unchanged.  Otherwise the
    chunk rows of THIS recording are sampled in groups of ``batch`` (the last group narrower); rows are never pooled
    across recordings, so a file depends on (weights, recording, seed, solver, ``batch``, ``chunk_frames``,
    ``overlap_frames``) only.  ``z``: the recording's noise [1,1,256,Tg], sliced per chunk; ``noise_key`` /
    ``noise_seed``: the keyed stream at absolute frames; neither: one draw of [1,1,256,Tg] from the torch generator.

    With the HIP-backed model on a device tensor the chunk rows come from one ``flowse_stft_compress_chunks`` launch and
    the waveform from one ``flowse_istft_decompress_chunks`` launch; nothing of the recording's length but its samples,
    the chunk rows and the waveform is held.  With ``VF_fn`` or CPU tensors the same steps run as torch ops -- stft,
    spec_fwd, index, sampler, blend (float64, rounded to complex64), spec_back, istft: the oracle composition."""
    from flowmse_amd.evaluate import enhance_waveform
    from flowmse_amd.schedule import OverlapSchedule
    if int(batch) < 1:
        raise ValueError(f"enhance_long: batch must be >= 1, got {batch}")
    if z is not None and noise_key is not None:
        raise ValueError("enhance_long: pass either z or noise_key, not both")
    batch, Tc = int(batch), int(chunk_frames)
    device = torch.device(device) if device is not None else y.device
    if y.dim() != 2 or y.size(0) != 1:
        raise ValueError(f"enhance_long takes one recording [1, samples], got {tuple(y.shape)}")
    dm = model.data_module
    L = y.size(1)
    K, hop, Tg = plan_chunks(L // dm.hop_length + 1, Tc, overlap_frames)
    if K == 1:
        return enhance_waveform(model, y, N=N, T_rev=T_rev, t_eps=t_eps, odesolver=odesolver, z=z, VF_fn=VF_fn,
                                device=device, noise_keys=None if noise_key is None else [noise_key],
                                noise_seed=noise_seed, as_tensor=as_tensor)
    return _enhance_rows(model, y, OverlapSchedule(Tc, overlap_frames), K, who="enhance_long", pad=(0, Tg),
                         analyze=lambda yn: dm.analyze_chunks(yn, Tc, hop),
                         synthesize=lambda s, norm: dm.synthesize_chunks(s, hop, L, norm),
                         blend=lambda s: blend_chunks_reference(s, hop), batch=batch, odesolver=odesolver, z=z,
                         noise_key=noise_key, noise_seed=noise_seed, VF_fn=VF_fn, device=device, as_tensor=as_tensor,
                         T_rev=T_rev, t_eps=t_eps, N=N)


# ---- trailing chunks: latency set by the hop, not the chunk ------------------------------------------------------------
# An opt-in mode of its own, NOT the reference's computation and not ``enhance_long``'s either.  The chunk of ``Tc`` frames
# slides by a small hop ``H``; its older ``P = Tc - H`` frames are context only and only its tail is kept, so a live caller
# (``flowmse_amd.live``, ``hop_frames=``) waits for ``H`` frames and not for ``Tc``: ``128 (H + X) + 382`` samples behind the
# input with a cross-fade of ``X`` frames, 0.184 s at ``(H, X) = (16, 4)``.  The price is ``Tc / H`` network rows per ``H``
# frames of audio.
#
# Geometry (``plan_trailing``): ``T = L // 128 + 1`` real frames, ``K = ceil(T / H)`` chunks, ``Tg = K H >= T`` frames.  Chunk
# ``k`` holds the recording's frames ``[k H - P, k H + H)``; frames ``< 0`` and ``>= T`` are zero -- the first chunks are
# right-aligned against zero frames before the recording, so the latency holds from the first sample on, and a recording
# shorter than one hop is one right-aligned chunk (there is no ``K = 1`` special case).
#
# Noise: the keyed stream of the recording's key is addressed at stream frame ``u = t + P`` (row ``k`` at ``frame0 = k H``,
# which is even), so chunks start from the same ``x_T`` wherever they overlap; an explicit ``z`` is one ``[1,1,256,P + Tg]``
# tensor sliced at ``[k H, k H + Tc)``.
#
# Seam rule (``blend_trailing_reference``; ``flowse_istft_decompress_trailing`` on the device): output frame ``t`` belongs to
# chunk ``k = min((t + X) // H, K - 1)`` at ``j = t - k H + P``; for ``k > 0`` and ``t < k H`` its value is ``a + w (b - a)``,
# ``a`` = chunk ``k - 1`` at ``j + H``, ``b`` = chunk ``k`` at ``j``, ``w = (i + 0.5) / X``, ``i = t - (k H - X)`` -- on the
# compressed complex value, before ``spec_back``, as in the rule above.
#
# The defaults ``(Tc, H, X) = (64, 16, 4)`` are chosen values, not tuned ones: no released checkpoint is at hand offline, so
# neither how little context the network tolerates nor how the seams sound has been judged by listening.
HOP_FRAMES, FADE_FRAMES = 16, 4
NOISE_FRAME_MAX = 2 ** 31 - 2        # the keyed noise stream takes frame0 + T up to this


def plan_trailing(T, Tc=64, H=HOP_FRAMES, X=FADE_FRAMES):
    """``(K, P, Tg)`` for ``T`` real frames as trailing chunks of ``Tc`` frames that slide by ``H`` and cross-fade over ``X``
    (comment above).  ``ValueError`` unless ``T >= 1``, ``Tc`` a positive multiple of 64, ``H`` even and ``4 <= H <= Tc``,
    ``0 <= X <= H`` and ``H + X <= Tc``."""
    T, Tc, H, X = int(T), int(Tc), int(H), int(X)
    if T < 1:
        raise ValueError(f"plan_trailing: T must be >= 1, got {T}")
    if Tc < 64 or Tc % 64:
        raise ValueError(f"plan_trailing: chunk_frames must be a positive multiple of 64 (the network's frame padding), got {Tc}")
    if H % 2 or not 4 <= H <= Tc:
        raise ValueError(f"plan_trailing: hop_frames must be even (the keyed noise stream pairs frames) and in "
                         f"4..chunk_frames = {Tc}, got {H}")
    if not 0 <= X <= H or H + X > Tc:
        raise ValueError(f"plan_trailing: fade_frames must be in 0..hop_frames = {H} with hop_frames + fade_frames <= "
                         f"chunk_frames = {Tc} (the fade reads the chunk before), got {X}")
    K = -(-T // H)
    return K, Tc - H, K * H


def blend_trailing_reference(chunks, H, X):
    """The trailing seam rule in float64: chunks ``[K,1,F,Tc]`` (numpy or torch, complex) that slide by ``H`` frames ->
    complex128 numpy ``[1,1,F,Tg]``, ``Tg = K H``.  Chunks cut from one spectrogram return it exactly (``b - a`` is an exact
    zero)."""
    c = chunks.detach().cpu().numpy() if torch.is_tensor(chunks) else np.asarray(chunks)
    c = c.astype(np.complex128)
    K, _, F, Tc = c.shape
    _, P, Tg = plan_trailing(1, Tc, H, X)
    H, X = int(H), int(X)
    out = np.empty((1, 1, F, K * H), dtype=np.complex128)
    for t in range(K * H):
        k = min((t + X) // H, K - 1)
        j = t - k * H + P
        b = c[k][:, :, j]
        if k > 0 and t < k * H:
            a = c[k - 1][:, :, j + H]
            b = a + (t - (k * H - X) + 0.5) / X * (b - a)
        out[0, :, :, t] = b
    return out


def enhance_trailing(model, y, chunk_frames=64, hop_frames=HOP_FRAMES, fade_frames=FADE_FRAMES, batch=8, N=5, T_rev=1.0,
                     t_eps=0.03, odesolver="euler", z=None, noise_key=None, noise_seed=0, VF_fn=None, device=None,
                     as_tensor=False):
    """One recording of any length as trailing chunks (comment above): what ``LiveEnhancer(hop_frames=...)`` returns for the
    finished recording, as a file call.  y: float tensor [1, samples].  Returns the enhanced waveform (numpy), normalised by
    the recording's global ``max|y|``; with ``as_tensor`` a 1-D tensor left on the compute device.

    The ``K`` rows are sampled in groups of ``batch`` (the last group narrower).  ``z``: the recording's noise
    [1,1,256,P + Tg], sliced per chunk at ``[k H, k H + Tc)``; ``noise_key`` / ``noise_seed``: the keyed stream at
    ``frame0 = k H``; neither: one draw from the torch generator.

    With the HIP-backed model on a device tensor the rows come from one ``flowse_stft_compress_trailing`` launch and the
    waveform from one ``flowse_istft_decompress_trailing`` launch.  With ``VF_fn`` or CPU tensors the same steps run as torch
    ops -- stft, spec_fwd, slice with zero frames, sampler, blend (float64, rounded to complex64), spec_back, istft: the oracle
    composition."""
    from flowmse_amd.schedule import TrailingSchedule
    if int(batch) < 1:
        raise ValueError(f"enhance_trailing: batch must be >= 1, got {batch}")
    if z is not None and noise_key is not None:
        raise ValueError("enhance_trailing: pass either z or noise_key, not both")
    batch, Tc, H, X = int(batch), int(chunk_frames), int(hop_frames), int(fade_frames)
    device = torch.device(device) if device is not None else y.device
    if y.dim() != 2 or y.size(0) != 1:
        raise ValueError(f"enhance_trailing takes one recording [1, samples], got {tuple(y.shape)}")
    dm = model.data_module
    L = y.size(1)
    T = L // dm.hop_length + 1
    K, P, Tg = plan_trailing(T, Tc, H, X)
    if P + Tg > NOISE_FRAME_MAX:
        raise ValueError(f"enhance_trailing: the noise stream is addressed up to frame {NOISE_FRAME_MAX}; this recording's "
                         f"last chunk ends at stream frame (K - 1) hop_frames + chunk_frames = {P + Tg}")
    return _enhance_rows(model, y, TrailingSchedule(Tc, H, X), K, who="enhance_trailing", what=" (P + Tg frames)",
                         pad=(P, P + Tg), analyze=lambda yn: dm.analyze_trailing(yn, Tc, H),
                         synthesize=lambda s, norm: dm.synthesize_trailing(s, H, X, L, norm),
                         blend=lambda s: blend_trailing_reference(s, H, X), batch=batch, odesolver=odesolver, z=z,
                         noise_key=noise_key, noise_seed=noise_seed, VF_fn=VF_fn, device=device, as_tensor=as_tensor,
                         T_rev=T_rev, t_eps=t_eps, N=N)
