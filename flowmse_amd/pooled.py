"""A folder of recordings, and the channels of a recording, as rows that share full sampler calls.

An opt-in mode (``flowmse_amd.enhance --pool``).  ``chunked.enhance_long`` samples the rows of ONE recording per call, so
a folder of short clips runs at batch width 1.  Here every (file, channel, chunk) is one row of the chunk geometry of
``chunked.plan_chunks``; rows of equal width from different files and channels are cut into sampler calls of EXACTLY
``batch`` rows.  A row's result depends neither on its neighbours nor on its position at a fixed batch width
(tests/test_gpu_model.py::test_full_batch_properties), and every call of a run has that one width, so a file's bytes depend
on (weights, the file's samples and name, seed, solver settings, ``batch``, ``Tc``, ``To``) only -- not on what else is in
the folder or on the order.  Channels are enhanced independently (nothing spatial).

Rules (``plan_pool``), all fixed:

* a file of ``L`` samples has ``T = L // 128 + 1`` frames and ``K, hop, Tg = plan_chunks(T, Tc, To)``;
* ``K > 1``: the file's rows have width ``Tc`` and start ``hop`` frames apart; ``K == 1``: the file is a one-chunk stack of its
  ``pad_spec`` width (the multiple of 64 that is ``>= T``), so nothing is zero-padded further than on the unpooled path;
* rows of one width make a bucket (a ``K == 1`` file of width ``Tc`` shares the ``Tc`` bucket); within a bucket files keep
  the order of ``items`` (``enhance.list_inputs``: sorted base name), a file's rows are ordered (channel, chunk);
* the bucket's row list is cut into consecutive calls of ``batch`` rows; the last call is filled up by repeating its own
  first row (same signal, key and ``frame0``), and what the fillers give is discarded: at most ``batch - 1`` wasted rows per
  bucket and run;
* buckets are processed one after another, in ascending width.

Noise is keyed only: row (file, channel c, chunk k) uses ``channel_key(name, c)`` at the absolute frame ``k hop``, so channel 0
of a file draws what the unpooled path draws for it.  A file is normalised by ONE factor, ``max|y|`` over all its channels,
which keeps the level balance between them.

Ensembles (``draws``, ``flowmse_amd.ensemble``; ``enhance --pool --samples D``): the draw is a fourth row coordinate.  A file's
rows are ordered (channel, draw, chunk), row (file, c, draw d, k) uses ``draw_key(channel_key(name, c), d)`` at the same
``frame0``, and the file is finished by ONE ``flowse_istft_decompress_ensemble`` launch that writes the mean of its draws.
``draws=(0,)`` is the plan, the code path and the bytes of a run without the argument.
"""
import collections

import torch

from flowmse_amd._lib import FLOWSE_MAX_SPEC_ROWS as MAX_BATCH    # the rows one flowse_stft_compress_rows launch builds
from flowmse_amd.chunked import CHUNK_FRAMES, OVERLAP_FRAMES, plan_chunks
from flowmse_amd.ensemble import agreements, check_draws, draw_keys
from flowmse_amd.schedule import OverlapSchedule
from flowmse_amd.util.noise import utterance_key

HOP = 128                        # samples per frame the plan counts in; enhance_pooled checks the data module's against it

Row = collections.namedtuple("Row", "item channel chunk frame0 filler draw", defaults=(0,))
Call = collections.namedtuple("Call", "width rows")


def channel_key(name, c):
    """The keyed-noise key of channel ``c`` of file ``name``: the file's ``utterance_key`` for channel 0 (a mono file keeps
    its noise), the key of ``"<name>#ch<c>"`` for the others."""
    c = int(c)
    if c < 0:
        raise ValueError(f"channel_key: channel must be >= 0, got {c}")
    return utterance_key(name) if c == 0 else utterance_key(f"{name}#ch{c}")


def file_geometry(L, Tc=CHUNK_FRAMES, To=OVERLAP_FRAMES):
    """``(K, hop, width)`` of a file of ``L`` samples: ``plan_chunks`` for ``K > 1``; for ``K == 1`` a one-chunk stack of the
    file's ``pad_spec`` width (``hop = width``)."""
    T = int(L) // HOP + 1
    K, hop, _ = plan_chunks(T, Tc, To)
    if K > 1:
        return K, hop, int(Tc)
    width = OverlapSchedule(Tc, To).single_width(T)
    return 1, width, width


def plan_pool(items, batch, Tc=CHUNK_FRAMES, To=OVERLAP_FRAMES, draws=(0,)):
    """The sampler calls of a run, by the rules of the module docstring.  ``items``: list of ``(name, channels, L)``; host
    only.  Returns a list of ``Call(width, rows)`` with ``rows`` a list of exactly ``batch``
    ``Row(item, channel, chunk, frame0, filler, draw)``, ``item`` the index into ``items``.  ``draws``: distinct draw
    indices ``>= 0``; every (channel, chunk) of a file becomes one row per draw, ordered (channel, draw, chunk)."""
    batch = int(batch)
    draws = check_draws(draws)
    if batch < 1:
        raise ValueError(f"plan_pool: batch must be >= 1, got {batch}")
    plan_chunks(1, Tc, To)                               # the geometry's own checks, before any file is looked at
    buckets = {}
    for i, (name, channels, L) in enumerate(items):
        if int(channels) < 1 or int(L) < 2 * HOP:
            raise ValueError(f"plan_pool: {name}: need >= 1 channel and >= {2 * HOP} samples, got {channels} x {L}")
        K, hop, width = file_geometry(L, Tc, To)
        rows = buckets.setdefault(width, [])
        rows.extend(Row(i, c, k, k * hop, False, d) for c in range(int(channels)) for d in draws for k in range(K))
    calls = []
    for width in sorted(buckets):
        rows = buckets[width]
        for r0 in range(0, len(rows), batch):
            group = rows[r0:r0 + batch]
            group += [group[0]._replace(filler=True)] * (batch - len(group))
            calls.append(Call(width, group))
    return calls


def enhance_pooled(model, load, items, write, batch=8, chunk_frames=CHUNK_FRAMES, overlap_frames=OVERLAP_FRAMES, N=5,
                   T_rev=1.0, t_eps=0.03, odesolver="euler", noise_seed=0, draws=(0,), agreement=None):
    """Run ``plan_pool(items, batch, chunk_frames, overlap_frames)`` on the HIP-backed ``model``.

    ``items``: list of ``(name, channels, L)``.  ``load(i)`` -> float32 tensor ``[channels, L]`` on the model's device,
    called when the file's first row comes up; ``write(i, x_hat)`` takes the enhanced ``[channels, L]`` device tensor when
    its last row is in, after which the file's tensors are dropped -- at any call at most ``batch`` files are open.

    Per file: one ``max|y|`` over all channels (one ``.item()``), the division by it on load exactly as the unpooled path
    divides (so the rows carry ``scale_in = 1`` and a file that fills its calls alone gives the bytes ``enhance_long``
    gives).  Per call: one ``flowse_stft_compress_rows`` launch, the unchanged ``get_white_box_solver`` with per-row
    ``noise_keys`` / ``noise_frame0``, copies of the sampled rows into the files' ``[C K,1,256,width]`` stacks.  Per
    finished file: one ``flowse_istft_decompress_stacks`` launch.  ``reserve(batch, 256, width)`` once per bucket.
    Returns ``dict(calls=, rows=, fillers=)``: sampler calls made, real rows and filler rows in them.

    ``draws`` (distinct draw indices, ``flowmse_amd.ensemble``): every row is sampled once per draw under
    ``draw_key(channel_key, d)``, the stack is ``[C D K,1,256,width]`` and ``write`` takes the MEAN of the draws, formed by one
    ``flowse_istft_decompress_ensemble`` launch per finished file.  With two or more draws ``agreement(i, [dB per channel])``
    (optional) is called before ``write(i, ...)``, from one read-back of the file's tracks.  Every call still has exactly
    ``batch`` rows, so by the fixed-width property above the rows of draw ``d`` are bit-identical whatever other draws are
    in the run: ``draws=(0, 1, 2)`` samples exactly the rows of the three runs ``draws=(d,)``, and only the finish differs.
    ``draws=(0,)`` is the run without the argument: same calls, same launches, same bytes."""
    from flowmse_amd.evaluate import _fused_ok
    from flowmse_amd.sampling import get_white_box_solver
    batch = int(batch)
    if not 1 <= batch <= MAX_BATCH:
        raise ValueError(f"enhance_pooled: batch must be 1..{MAX_BATCH} (the rows of one spectrogram launch), got {batch}")
    draws = check_draws(draws)
    D, dpos = len(draws), {d: j for j, d in enumerate(draws)}
    calls = plan_pool(items, batch, chunk_frames, overlap_frames, draws)
    geometry = [file_geometry(L, chunk_frames, overlap_frames) for _, _, L in items]
    keys = [[draw_keys(channel_key(name, c), draws) for c in range(int(C))] for name, C, _ in items]
    left = [int(C) * D * g[0] for (_, C, _), g in zip(items, geometry)]         # rows still to come, per file
    n_rows = sum(left)
    dm = model.data_module
    if getattr(dm, "hop_length", None) != HOP:
        raise RuntimeError(f"enhance_pooled plans in frames of {HOP} samples, the model's transform has hop_length "
                           f"{getattr(dm, 'hop_length', None)}")
    opened = {}                                                            # item -> (samples [C, L], peak, stack)
    width = None
    for call in calls:
        for row in call.rows:
            if row.item in opened:
                continue
            name, C, L = items[row.item]
            y = load(row.item)
            if tuple(y.shape) != (int(C), int(L)) or y.dtype != torch.float32:
                raise ValueError(f"enhance_pooled: {name}: load() returned {y.dtype} {tuple(y.shape)}, the plan has "
                                 f"float32 {(int(C), int(L))}")
            if not _fused_ok(model, [y]):
                raise RuntimeError("enhance_pooled needs the HIP spectrogram kernels: device tensors and the released STFT "
                                   "configuration (n_fft 510, hop 128, hann, 'exponent')")
            peak = y.abs().max().item()
            K = geometry[row.item][0]
            stack = torch.empty(int(C) * D * K, 1, 256, call.width, dtype=torch.complex64, device=y.device)
            opened[row.item] = ((y / peak).contiguous(), peak, stack)
        device = opened[call.rows[0].item][0].device
        if call.width != width:
            width = call.width
            with torch.cuda.device(device):
                model.dnn.reserve(batch, 256, width)
        Y = dm.analyze_rows([(opened[r.item][0][r.channel], r.frame0, 1.0) for r in call.rows], width)
        sample = get_white_box_solver(odesolver, model.ode, model, Y=Y, Y_prior=Y, T_rev=T_rev, t_eps=t_eps, N=N,
                                      noise_keys=[keys[r.item][r.channel][dpos[r.draw]] for r in call.rows], noise_seed=noise_seed,
                                      noise_frame0=[r.frame0 for r in call.rows])()[0]
        real = [r for r in call.rows if not r.filler]
        r0 = 0
        while r0 < len(real):                                               # one copy per file in the call
            i = real[r0].item
            r1 = r0
            while r1 < len(real) and real[r1].item == i:
                r1 += 1
            K = geometry[i][0]
            # (channel, draw, chunk) order: consecutive in the stack
            s0 = (real[r0].channel * D + dpos[real[r0].draw]) * K + real[r0].chunk
            opened[i][2][s0:s0 + r1 - r0].copy_(sample[r0:r1])
            left[i] -= r1 - r0
            if left[i] == 0:
                _, peak, stack = opened.pop(i)
                _, C, L = items[i]
                if D == 1:
                    write(i, dm.synthesize_stacks(stack, int(C), geometry[i][1], int(L), peak))
                else:
                    x_hat, tracks = dm.synthesize_ensemble(stack, int(C), D, geometry[i][1], int(L), peak, tracks=True)
                    if agreement is not None:
                        agreement(i, agreements(tracks, int(L)))
                    write(i, x_hat)
            r0 = r1
    return dict(calls=len(calls), rows=n_rows, fillers=len(calls) * batch - n_rows)
