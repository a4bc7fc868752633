#!/usr/bin/env python3
"""Inference CLI: counterpart of the reference's ``evaluate.py`` (evaluate.py:27-194) on the HIP sampler.

    python -m flowmse_amd.evaluate --test_dir DATA --folder_destination OUT --ckpt MODEL.ckpt [--N 5]

Same arguments and outputs (``files/*.wav``, ``_results.csv``, ``_avg_results.txt``, ``_settings.txt``).  Per
utterance it follows evaluate.py:101-136: load wav -> normalise by max|y| -> STFT -> magnitude compression
(spec_fwd) -> pad frames to a multiple of 64 -> white-box Euler sampler -> spec_back -> iSTFT -> rescale.
Wave I/O uses scipy (torchaudio / soundfile are optional), PESQ / ESTOI are reported when the ``pesq`` / ``pystoi``
packages are importable, SI-SDR / SI-SIR / SI-SAR always (utils.py:10-35); ``--metrics device`` takes ESTOI and the three
energy ratios from the library instead (``flowmse_amd.metrics``: float64 on the GPU, no optional package, one read-back
per sampler call), PESQ stays a host import.  ``--synthetic`` runs with synthetic
weights and synthetic noisy/clean pairs (no checkpoint or dataset needed) as an end-to-end smoke demo.

``--noise keyed`` draws the prior noise from the keyed stream of ``flowmse_amd.util.noise`` (addressed by seed, file name,
bin and frame) instead of the process-wide generator, and ``--gpus N`` shards the set over N GPUs of this node, one
process each; in keyed mode the wavs and the CSV are byte-identical for any ``--gpus``, any ``--streams`` and any file
order (they depend on weights, utterance, seed, solver settings and ``--batch`` only).

``--valid_loss K`` (keyed noise only) adds a ``valid_loss`` column: the flow-matching loss the model is trained on
(reference ``VFModel._step``, model.py:130-143), on each file's 256-frame validation item, mean over K keyed draws.

``--samples D`` (keyed noise only; ``flowmse_amd.ensemble``) samples every file ``D`` times and writes and scores the MEAN of
the draws; an ``agreement_db`` column says how far the draws agree.  NOT the reference's computation, which draws once.

Layout: the per-utterance recipe lives once, in ``_enhance`` (``enhance_waveform`` / ``enhance_batch`` / ``enhance_concurrent``
are it with one group, one group of all, and lanes); ``plan_calls`` lists a run's sampler calls for either noise mode and
``run_calls`` is the one loop that turns them into wavs and rows.
"""
import argparse
import csv
import glob
import os
import re
import time

import numpy as np
import torch

from flowmse_amd.ensemble import samples_arg
from flowmse_amd.sampling import get_white_box_solver, get_white_box_solver_multi
from flowmse_amd.util.other import pad_spec, read_wav as _read_wav


def energy_ratios(s_hat, s, n):
    """SI-SDR, SI-SIR, SI-SAR in dB (reference utils.py:10-35)."""
    alpha_s = np.dot(s_hat, s) / np.linalg.norm(s) ** 2
    s_target = alpha_s * s
    alpha_n = np.dot(s_hat, n) / np.linalg.norm(n) ** 2
    e_noise = alpha_n * n
    e_art = s_hat - s_target - e_noise
    si_sdr = 10 * np.log10(np.linalg.norm(s_target) ** 2 / np.linalg.norm(e_noise + e_art) ** 2)
    si_sir = 10 * np.log10(np.linalg.norm(s_target) ** 2 / np.linalg.norm(e_noise) ** 2)
    si_sar = 10 * np.log10(np.linalg.norm(s_target) ** 2 / np.linalg.norm(e_art) ** 2)
    return si_sdr, si_sir, si_sar


def mean_std(data):
    a = np.asarray([d for d in data if np.isfinite(d)], dtype=np.float64)
    return f"{a.mean():.2f} ± {a.std():.2f}" if a.size else "nan"


def _fused_ok(model, ys, VF_fn=None):
    """True when analysis and synthesis of the waveforms ``ys`` run as the library's spectrogram kernels: the model's own
    field (no ``VF_fn``), device tensors, the released STFT configuration (``SpecTransform.fused_ok``)."""
    dm = model.data_module
    return VF_fn is None and hasattr(dm, "fused_ok") and all(dm.fused_ok(y) for y in ys)


def _analyze(model, y, fused, pad=True):
    """Normalised waveform [1, samples] -> compressed spectrogram [1,1,F,T]: STFT + compression + frame padding as one HIP
    kernel, or the same as torch ops (``pad=False``: the real frames only)."""
    if fused:
        return model.data_module.analyze(y)
    Y = torch.unsqueeze(model._forward_transform(model._stft(y)), 0)
    return pad_spec(Y) if pad else Y


def _synthesize(model, sample, T_orig, norm_factor, fused):
    """Sampled spectrogram [1,1,F,T] -> 1-D waveform of ``T_orig`` samples, rescaled: decompression + iSTFT + rescale as one
    HIP kernel, or the same as torch ops."""
    if fused:
        return model.data_module.synthesize(sample, T_orig, norm_factor).reshape(-1)
    return (model.to_audio(sample.squeeze(), T_orig) * norm_factor).reshape(-1)


def _enhance(model, ys, groups, lanes=None, N=5, T_rev=1.0, t_eps=0.03, odesolver="euler", z=None, VF_fn=None, device=None,
             noise_keys=None, noise_seed=0, as_tensor=False, samples=1, agreement=None):
    """The per-utterance recipe (evaluate.py:107-136) for a list of utterances ``ys`` (float tensors [1, samples_i]):
    normalise by max|y| (one ``.item()`` each) -> analysis -> sampler -> synthesis.  ``groups``: lists of indices into
    ``ys``, each an equal-padded-length batch that is sampled as one item.  ``lanes`` None: one ``get_white_box_solver`` call
    per group, in order; an integer: ONE ``get_white_box_solver_multi`` call on that many lanes.  Either way the priors are
    drawn in the order of ``groups``.  ``noise_keys``: one key per utterance, in the order of ``ys``.  Returns the waveforms in
    the order of ``ys``: numpy, or with ``as_tensor`` 1-D tensors left on the compute device.

    ``samples`` D > 1 (``flowmse_amd.ensemble``): a group of g utterances is sampled as ONE item of g D rows ordered (draw,
    utterance) -- the same ``Y`` rows repeated, keys ``draw_key(key_i, d)`` -- and every utterance is finished by one
    ``synthesize_ensemble`` call over its D rows (``draw_stride = g``): the waveform returned is the mean of the draws.
    ``agreement``: a list that receives ``(index into ys, agreement in dB)`` per utterance.  Keyed noise and the HIP
    spectrogram kernels only."""
    from flowmse_amd.ensemble import agreements
    from flowmse_amd.util.noise import draw_key
    D = int(samples)
    ys = [y.to(device or y.device) for y in ys]
    norms = [y.abs().max().item() for y in ys]
    fused = _fused_ok(model, ys, VF_fn)
    if D > 1 and (noise_keys is None or z is not None or not fused):
        raise ValueError("samples > 1 needs keyed noise (noise_keys, no explicit z) and the HIP spectrogram kernels")
    specs = [_analyze(model, y / n, fused) for y, n in zip(ys, norms)]     # y / max|y| as the reference computes it (evaluate.py:111)
    Ys = [specs[g[0]] if len(g) * D == 1 else torch.cat([specs[i] for i in g] * D, dim=0) for g in groups]
    keys = [None if noise_keys is None else [draw_key(noise_keys[i], d) for d in range(D) for i in g] for g in groups]
    field = VF_fn if VF_fn is not None else model
    kw = dict(T_rev=T_rev, t_eps=t_eps, N=N, noise_seed=noise_seed)
    if lanes is None:
        samples = [get_white_box_solver(odesolver, model.ode, field, Y=Y, Y_prior=Y, z=z, noise_keys=k, **kw)()[0]
                   for Y, k in zip(Ys, keys)]
    else:
        samples = get_white_box_solver_multi(odesolver, model.ode, field, Ys, lanes=lanes,
                                             noise_keys=None if noise_keys is None else keys, **kw)()[0]
    out = [None] * len(ys)
    for g, sample in zip(groups, samples):
        for j, i in enumerate(g):
            if D == 1:
                x_hat = _synthesize(model, sample[j:j + 1], ys[i].size(1), norms[i], fused)
            else:                  # rows j, j + g, ...: the D draws of utterance i, a one-chunk stack each
                x_hat, tracks = model.data_module.synthesize_ensemble(
                    sample[j:j + (D - 1) * len(g) + 1], 1, D, sample.shape[3], ys[i].size(1), norms[i], draw_stride=len(g),
                    K=1, tracks=True)
                x_hat = x_hat.reshape(-1)
                if agreement is not None:
                    agreement.append((i, agreements(tracks, ys[i].size(1))[0]))
            out[i] = x_hat if as_tensor else x_hat.cpu().numpy()
    return out


def enhance_waveform(model, y, N=5, T_rev=1.0, t_eps=0.03, odesolver="euler", z=None, VF_fn=None, device=None,
                     noise_keys=None, noise_seed=0, as_tensor=False):
    """One utterance, evaluate.py:107-136.  y: float tensor [1, samples].  Returns the enhanced waveform (numpy; with
    ``as_tensor`` the same values as a 1-D tensor left on the compute device).
    ``noise_keys`` ([key], see ``flowmse_amd.util.noise.utterance_key``) / ``noise_seed``: keyed prior noise."""
    return _enhance(model, [y], [[0]], None, N, T_rev, t_eps, odesolver, z, VF_fn, device, noise_keys, noise_seed,
                    as_tensor)[0]


def enhance_batch(model, ys, N=5, T_rev=1.0, t_eps=0.03, odesolver="euler", noise_keys=None, noise_seed=0, as_tensor=False):
    """Several utterances whose padded frame counts agree, as ONE sampler call (the reference enhances one file at
    a time, evaluate.py:97; trajectories are independent, so batching changes nothing but throughput).
    ys: list of float tensors [1, samples_i] on the target device.  Returns a list of numpy waveforms (with ``as_tensor``
    the same values as 1-D tensors left on the device).
    ``noise_keys`` (one key per utterance) / ``noise_seed``: keyed prior noise, which follows the utterance and not its
    row or batch."""
    return _enhance(model, ys, [list(range(len(ys)))], None, N, T_rev, t_eps, odesolver, noise_keys=noise_keys,
                    noise_seed=noise_seed, as_tensor=as_tensor)


def enhance_concurrent(model, ys, lanes, N=5, T_rev=1.0, t_eps=0.03, odesolver="euler", groups=None, noise_keys=None,
                       noise_seed=0, as_tensor=False):
    """Several utterances of ANY lengths as one multi-lane sampler call: up to ``lanes`` (1..4) of them are in flight on
    the GPU at a time, on streams that share one copy of the weights (``get_white_box_solver_multi``).  Analysis and
    synthesis run per utterance as in ``enhance_batch``.  ``groups`` (optional): lists of indices into ``ys``, each an
    equal-padded-length batch that is sampled as ONE item; default every utterance is its own item, and then every
    waveform equals ``enhance_waveform``'s for the same prior noise, bit for bit.  A throughput option: a single
    utterance's latency goes up.  ys: list of float tensors [1, samples_i] on the target device.  Returns the list of
    numpy waveforms (with ``as_tensor``: 1-D device tensors), in the order of ``ys``.  ``noise_keys`` (one key per
    utterance, in the order of ``ys``) / ``noise_seed``: keyed prior noise."""
    groups = [[i] for i in range(len(ys))] if groups is None else [list(g) for g in groups]
    return _enhance(model, ys, groups, lanes, N, T_rev, t_eps, odesolver, noise_keys=noise_keys, noise_seed=noise_seed,
                    as_tensor=as_tensor)


def _write_wav(path, x, sr=16000):
    """16-bit PCM WAV like the reference's ``soundfile.write(path, x_hat, 16000)`` (evaluate.py:147; libsndfile's
    default subtype for .wav is PCM_16, float samples scaled by 0x7FFF and rounded to nearest).  soundfile itself is
    used when importable, so output trees diff cleanly against the reference's.  Without it scipy writes samples formed
    the way libsndfile forms them: the product ``x * 32767`` in float32 (libsndfile scales in the sample's own type
    before ``lrintf``), round half to even, and -- libsndfile does NOT clip by default (SFC_SET_CLIPPING off) -- a
    sample with |x| > 1, possible after the rescale by max|y|, keeps the low 16 bits of its rounded value instead of
    saturating.  Non-finite samples (undefined in libsndfile's float -> int conversion) are written as 0.  The fallback
    aims at the same file for finite input; it has not been diffed against libsndfile here (soundfile is not in
    this image)."""
    x = np.asarray(x, dtype=np.float32)
    try:
        import soundfile
        soundfile.write(path, x, sr)
        return
    except ImportError:
        pass
    from scipy.io import wavfile
    scaled = np.rint(x * np.float32(32767.0))                      # float32 product, like libsndfile
    scaled = np.where(np.isfinite(scaled), scaled, np.float32(0.0))
    pcm = scaled.astype(np.int64).astype(np.uint16).astype(np.int16)
    wavfile.write(path, sr, pcm)


def _synthetic_pairs(n, seconds=2.0, sr=16000, seed=0):
    """``seconds``: one duration, or a sequence that is cycled over the pairs."""
    g = np.random.default_rng(seed)
    secs = [float(v) for v in seconds] if isinstance(seconds, (list, tuple)) else [float(seconds)]
    out = []
    for i in range(n):
        t = np.arange(int(secs[i % len(secs)] * sr)) / sr
        clean = 0.3 * np.sin(2 * np.pi * (200 + 60 * i) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t))
        noisy = clean + 0.05 * g.standard_normal(t.shape)
        out.append((f"synthetic_{i:02d}.wav", clean.astype(np.float32), noisy.astype(np.float32)))
    return out


MAX_ROWS = 64                    # rows of one sampler call that --batch x --samples may ask for
MAX_STREAMS = 4                  # FLOWSE_MAX_LANES of the library: one stream per lane, four hardware queues per process
_ITEMS_PER_LANE = 4              # sampler items per lane and multi-lane call (bounds the spectrograms held on the device)


def _streams_arg(v):
    k = int(v)
    if not 1 <= k <= MAX_STREAMS:
        raise argparse.ArgumentTypeError(f"--streams must be 1..{MAX_STREAMS}, got {v}")
    return k


def _seconds_arg(v):
    try:
        secs = [float(x) for x in v.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--synthetic_seconds takes a comma list of durations, got {v!r}")
    if not secs or min(secs) <= 0:
        raise argparse.ArgumentTypeError(f"--synthetic_seconds takes positive durations, got {v!r}")
    return secs


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--test_dir", type=str, default=None, help="directory with test/clean and test/noisy")
    ap.add_argument("--odesolver_type", type=str, choices=("white",), default="white")
    ap.add_argument("--odesolver", type=str, default="euler")
    ap.add_argument("--reverse_starting_point", type=float, default=1.0)
    ap.add_argument("--last_eval_point", type=float, default=0.03)
    ap.add_argument("--folder_destination", type=str, required=True)
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--N_mid", type=int, default=0, help="accepted for command-line compatibility (evaluate.py:42: "
                                                         "'not related to FlowSE'); must be 0")
    ap.add_argument("--synthetic", type=int, default=0, help="run on this many synthetic pairs with synthetic weights")
    ap.add_argument("--synthetic_seconds", type=_seconds_arg, default=[2.0],
                    help="durations of the synthetic pairs in seconds, a comma list cycled over them (default 2.0)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16x3", "bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=1,
                    help="enhance up to this many utterances of equal padded length per sampler call (1 = reference "
                         "behaviour). Batch widths select different kernels: across --batch values the keyed NOISE of an "
                         "utterance is identical, its enhanced samples agree to fp32 tolerance (about 1e-5 relative), not "
                         "byte for byte")
    ap.add_argument("--streams", type=_streams_arg, default=1,
                    help="sample up to this many utterances (or --batch groups) concurrently on one GPU, on streams that "
                         "share the weights (1..4; 1 = one sampler call at a time). Same output files; more throughput "
                         "at small batch, longer latency per utterance")
    ap.add_argument("--seed", type=int, default=None,
                    help="--noise torch: torch.manual_seed before the first prior sample, so that two runs draw the same "
                         "noise and write the same files (default: unseeded, like the reference). --noise keyed: the "
                         "64-bit seed of the keyed stream (default: drawn from os.urandom and recorded in _settings.txt)")
    ap.add_argument("--noise", choices=("torch", "keyed"), default=None,
                    help="prior noise. torch: the process-wide generator, consumed in processing order (the reference's "
                         "behaviour). keyed: a counter-based stream addressed by (seed, file name, bin, frame), so an "
                         "utterance's files do not depend on --gpus, --streams, the processing order or what else is in "
                         "the directory. Default: torch with --gpus 1, keyed with --gpus > 1")
    ap.add_argument("--metrics", choices=("host", "device"), default="host",
                    help="host: ESTOI from pystoi where importable (nan otherwise), the energy ratios in numpy. device: ESTOI "
                         "and SI-SDR / SI-SIR / SI-SAR in float64 on the GPU (flowmse_amd.metrics), read back once per "
                         "sampler call; PESQ stays on the host either way")
    ap.add_argument("--valid_loss", type=int, default=0, metavar="K",
                    help="also score every file's validation item (centre crop / pad to 256 frames, as the reference's "
                         "validation set builds it) with the flow-matching loss the model is trained on: a valid_loss column "
                         "with the mean over K keyed draws of (t, z). Needs --noise keyed. 0 = off")
    ap.add_argument("--samples", type=samples_arg, default=1, metavar="D",
                    help="sample every file D times under independent keyed streams (draw d of a file uses draw_key(key, d)) "
                         "and write and score the MEAN of the draws; the CSV gains an agreement_db column (the mean's power "
                         "over the draws' deviation from it: high = the draws agree). Needs keyed noise (selected when --noise "
                         "is not given) and --batch x D <= 64. Not the reference's computation (it draws once). D > 1 makes "
                         "the sampler call D times as wide, and widths select different kernels: draw 0 inside an ensemble "
                         "equals the single-draw output to rounding only here (bit for bit under enhance --pool). 1 = off")
    ap.add_argument("--gpus", type=int, default=1,
                    help="shard the test set over this many GPUs of this node, one process each (keyed noise only)")
    return ap


def parse_args(argv=None, ap=None):
    """Parse and resolve the command line: ``--noise`` defaults to ``torch`` at ``--gpus 1`` and ``keyed`` above."""
    ap = ap or build_parser()
    args = ap.parse_args(argv)
    if args.gpus < 1:
        ap.error(f"--gpus must be >= 1, got {args.gpus}")
    if args.batch < 1:
        ap.error(f"--batch must be >= 1, got {args.batch}")
    if args.gpus > 1 and args.noise == "torch":
        ap.error("--gpus > 1 needs --noise keyed: a single host random stream has no meaning across ranks")
    if args.samples > 1 and args.noise == "torch":
        ap.error(f"--samples {args.samples} needs --noise keyed: the draws are independent streams of the keyed noise")
    if args.samples > 1 and args.batch * args.samples > MAX_ROWS:    # one draw: --batch is as free as it always was
        ap.error(f"--batch x --samples must be <= {MAX_ROWS} (the rows of one sampler call), got {args.batch} x {args.samples}")
    if args.noise is None:
        args.noise = "keyed" if args.gpus > 1 or args.samples > 1 else "torch"
    if args.valid_loss < 0:
        ap.error(f"--valid_loss must be >= 0, got {args.valid_loss}")
    if args.valid_loss and args.noise != "keyed":
        ap.error("--valid_loss needs --noise keyed: its times and noise are draws of the keyed stream")
    return args


def _padded_frames(n_samples):
    return (((n_samples // 128 + 1) + 63) // 64) * 64


def _num_samples(path):
    """Samples per channel of a wav file, from its header where the reader allows it."""
    try:
        import soundfile
        return int(soundfile.info(path).frames)
    except ImportError:
        pass
    from scipy.io import wavfile
    try:
        return int(wavfile.read(path, mmap=True)[1].shape[0])
    except ValueError:                                             # a sample format scipy cannot map
        return int(wavfile.read(path)[1].shape[0])


def _load_model(args, ap):
    """(model, epoch) on the current device, in eval mode at --precision."""
    from flowmse_amd.model import VFModel
    if args.synthetic:
        from flowmse_amd.util import synth
        model = VFModel(backbone="ncsnpp", ode="flowmatching")
        model.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape)))
                                   for n, p in model.dnn.named_parameters()})
    else:
        if not args.ckpt or not args.test_dir:
            ap.error("--ckpt and --test_dir are required unless --synthetic is given")
        model = VFModel.load_from_checkpoint(args.ckpt, base_dir="", batch_size=8, num_workers=4,
                                             kwargs=dict(gpu=False))
    model.eval(no_ema=False)
    model.cuda()
    model.dnn.set_precision(args.precision)
    m = re.search(r"epoch=(\d+)", args.ckpt or "")
    return model, (m.group(1) if m else "n/a")


def _metric_fns():
    try:
        from pesq import pesq
    except Exception:
        pesq = None
    try:
        from pystoi import stoi
    except Exception:
        stoi = None
    return pesq, stoi


def _metrics(pesq, stoi, x, y, x_hat, sr=16000):
    """(pesq, estoi, si_sdr, si_sir, si_sar) of one utterance: clean x, noisy y, enhanced x_hat."""
    try:
        p = pesq(sr, x, x_hat, "wb") if pesq else float("nan")
    except Exception:
        p = float("nan")
    e = stoi(x, x_hat, sr, extended=True) if stoi else float("nan")
    return (p, e) + tuple(energy_ratios(x_hat, x, y - x))


def _metrics_device(pesq, triples, sr=16000):
    """The rows of ``_metrics`` for the utterances of ONE sampler call with ``--metrics device``: ``triples`` is a list of
    (clean x: numpy, noisy y: numpy or device tensor, enhanced x_hat: 1-D device tensor).  ESTOI and the energy ratios of
    all of them are queued on the device and read back once; PESQ as in ``_metrics``.  Returns the rows and the enhanced
    waveforms as numpy arrays."""
    from flowmse_amd.metrics import metrics_device
    dev = triples[0][2].device
    table = torch.empty(len(triples), 4, dtype=torch.float64, device=dev)
    for row, (x, y, x_hat) in zip(table, triples):
        metrics_device(x, y.reshape(-1) if isinstance(y, torch.Tensor) else y, x_hat, out=row, sr=sr)
    table = table.cpu().numpy()                                    # the one read-back
    rows, waves = [], []
    for vals, (x, _, x_hat) in zip(table, triples):
        w = x_hat.cpu().numpy()
        try:
            p = pesq(sr, x, w, "wb") if pesq else float("nan")
        except Exception:
            p = float("nan")
        rows.append((p,) + tuple(float(v) for v in vals))
        waves.append(w)
    return rows, waves


def _write_reports(target_dir, data, args, model, epoch, noise_seed):
    with open(os.path.join(target_dir, "_results.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(list(data.keys()))
        for i in range(len(data["filename"])):
            w.writerow([data[k][i] for k in data])
    with open(os.path.join(target_dir, "_avg_results.txt"), "w") as f:
        f.write("PESQ: {} \n".format(mean_std(data["pesq"])))
        f.write("ESTOI: {} \n".format(mean_std(data["estoi"])))
        f.write("SI-SDR: {} \n".format(mean_std(data["si_sdr"])))
        f.write("SI-SIR: {} \n".format(mean_std(data["si_sir"])))
        f.write("SI-SAR: {} \n".format(mean_std(data["si_sar"])))
        if "valid_loss" in data:                                   # --valid_loss only: the other files are unchanged
            a = np.asarray(data["valid_loss"], dtype=np.float64)
            f.write(f"valid_loss: {a.mean():.6g} ± {a.std():.6g} \n")
        if "agreement_db" in data:                                 # --samples D > 1 only
            f.write("Agreement: {} \n".format(mean_std(data["agreement_db"])))
    with open(os.path.join(target_dir, "_settings.txt"), "w") as f:
        f.write(f"epoch: {epoch}\ncheckpoint file: {args.ckpt}\nodesolver_type: {args.odesolver_type}\n")
        f.write(f"odesolver: {args.odesolver}\nReverse starting point: {args.reverse_starting_point}\n")
        f.write(f"Last evaluated point: {args.last_eval_point}\ndata: {args.test_dir}\node: FLOWMATCHING\n")
        f.write(f"sigma_min: {model.ode.sigma_min}\nsigma_max: {model.ode.sigma_max}\nN: {args.N}\n")
        f.write(f"precision: {args.precision}\n")
        f.write(f"batch: {args.batch}\nstreams: {args.streams}\nseed: {args.seed}\n")
        f.write(f"noise: {args.noise}\nnoise seed: {noise_seed}\ngpus: {args.gpus}\n")
        if getattr(args, "metrics", "host") == "device":           # a host run's file is unchanged
            f.write("metrics: device\n")
        if getattr(args, "valid_loss", 0):
            f.write(f"valid_loss draws: {args.valid_loss}\n")
        if getattr(args, "samples", 1) > 1:
            f.write(f"samples: {args.samples}\n")


_COLUMNS = ("filename", "pesq", "estoi", "si_sdr", "si_sir", "si_sar")


def _spawn_ranks(args, argv):
    """Run this module as ``args.gpus`` ranks on this node, one per GPU, and return their exit status.  The parent holds
    no GPU state: the ranks are fresh child processes.  An unseeded run gets its seed here, so every rank has the same."""
    import signal
    import socket
    import subprocess
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    if args.seed is None:
        argv += ["--seed", str(int.from_bytes(os.urandom(8), "little"))]
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "flowmse_amd.evaluate"] + argv
    proc = subprocess.Popen(cmd, env=env)
    try:
        signal.signal(signal.SIGTERM, lambda *_: sys.exit(143))    # a terminated parent takes its ranks with it
    except ValueError:                                             # not the main thread: no handler, the ranks run on
        pass
    try:
        return proc.wait()
    finally:
        if proc.poll() is None:
            proc.terminate()                                       # the launcher ends its workers on SIGTERM
            try:
                proc.wait(30)
            except subprocess.TimeoutExpired:
                proc.kill()


def _enter_rank(args):
    """(rank, world) of this process after binding it to its device and joining the process group (world > 1)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}: refusing to run on a different GPU count")
    if world == 1:
        return 0, 1
    if os.environ.get("FLOWSE_EVAL_SHARE_GPU"):                    # test hook: every rank on device 0
        local_rank = 0
    elif torch.cuda.device_count() < world:
        raise SystemExit(f"--gpus {world} needs {world} visible devices, found {torch.cuda.device_count()} "
                         "(FLOWSE_EVAL_SHARE_GPU=1 FLOWSE_EVAL_BACKEND=gloo runs the ranks on one device for testing)")
    torch.cuda.set_device(local_rank)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("FLOWSE_EVAL_BACKEND", "nccl")        # "gloo": ranks that share one GPU (RCCL cannot)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group(backend)
    return rank, world


def plan_calls(noise, batch, streams, lens, world=1, rank=0):
    """The sampler calls of rank ``rank`` of ``world`` in processing order; host only.  ``lens``: every file's padded frame
    count.  A call is a list of groups, a group a list of file indices that are sampled as one equal-padded-length batch.
    keyed: the batches of the WHOLE set, dealt to the ranks unsplit (batch composition does not depend on the world size).
    torch: at ``batch > 1`` the files grouped by padded frame count, largest first; else the files in order.
    ``streams > 1``: ``streams * _ITEMS_PER_LANE`` groups per (multi-lane) call; else one group per call."""
    from flowmse_amd.parallel import batches_by_length, plan_shards
    if noise == "keyed":
        groups = [list(ids) for _, ids in plan_shards(lens, world, batch, level=False)[rank]]
    elif batch > 1:
        groups = [list(ids) for _, ids in batches_by_length(range(len(lens)), lens, batch)]
    else:
        groups = [[i] for i in range(len(lens))]
    per_call = streams * _ITEMS_PER_LANE if streams > 1 else 1
    return [groups[k:k + per_call] for k in range(0, len(groups), per_call)]


def _sources(args):
    """``(names, n_samples, load)`` of the run's files in sorted-filename order; ``load(i)`` -> (clean, noisy) as numpy.  The
    lengths of files on disk come from their headers: the plan needs every length, a file is read when its call comes up."""
    if args.synthetic:
        pairs = _synthetic_pairs(args.synthetic, seconds=args.synthetic_seconds)
        return [p[0] for p in pairs], [p[2].shape[0] for p in pairs], lambda i: (pairs[i][1], pairs[i][2])
    clean_dir = os.path.join(args.test_dir, "test", "clean")
    noisy_dir = os.path.join(args.test_dir, "test", "noisy")
    names = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(noisy_dir, "*.wav")))]

    def load(i):
        return (_read_wav(os.path.join(clean_dir, names[i]))[0][0].numpy(),
                _read_wav(os.path.join(noisy_dir, names[i]))[0][0].numpy())

    return names, [_num_samples(os.path.join(noisy_dir, n)) for n in names], load


def _valid_losses(model, waves, names, seed, draws, batch, device):
    """``--valid_loss`` of the files of one planned batch: ``waves`` their (clean, noisy) numpy pairs."""
    from flowmse_amd.util.inference import keyed_valid_losses, validation_item
    items = [validation_item(model, torch.from_numpy(x)[None].to(device), torch.from_numpy(y)[None].to(device))
             for x, y in waves]
    return keyed_valid_losses(model, items, names, seed=seed, draws=draws, batch=batch)


def run_calls(args, model, epoch, names, n_samples, load, seed=None, rank=0, world=1, device="cuda"):
    """The driver loop of both noise modes: ``plan_calls`` -> per call load, ``_enhance`` (utterance keys in keyed mode only),
    metrics, ``--valid_loss``, one wav per file as its call completes -> rows gathered on rank 0, sorted by file index,
    ``_write_reports``.  ``seed``: the keyed stream's seed, None in torch mode.  Returns the seconds the loop took."""
    from flowmse_amd.parallel import gather_rows
    from flowmse_amd.util.noise import utterance_key
    keyed = args.noise == "keyed"
    target_dir = args.folder_destination.rstrip("/") + "/"
    os.makedirs(target_dir + "files/", exist_ok=True)
    pesq, stoi = _metric_fns()
    on_device = args.metrics == "device"
    lanes = args.streams if args.streams > 1 else None
    calls = plan_calls(args.noise, args.batch, args.streams, [_padded_frames(n) for n in n_samples], world, rank)
    rows, t0 = [], time.time()
    for call in calls:
        flat = [i for g in call for i in g]
        pos = {i: j for j, i in enumerate(flat)}
        waves = [load(i) for i in flat]
        ys = [torch.from_numpy(y)[None].to(device) for _, y in waves]
        agree = []
        outs = _enhance(model, ys, [[pos[i] for i in g] for g in call], lanes, N=args.N, T_rev=args.reverse_starting_point,
                        t_eps=args.last_eval_point, odesolver=args.odesolver,
                        noise_keys=[utterance_key(names[i]) for i in flat] if keyed else None,
                        noise_seed=seed if keyed else 0, as_tensor=on_device,
                        **(dict(samples=args.samples, agreement=agree) if args.samples > 1 else {}))
        if on_device:
            metric_rows, outs = _metrics_device(pesq, [(x, yd, x_hat) for (x, _), yd, x_hat in zip(waves, ys, outs)])
        else:
            metric_rows = [_metrics(pesq, stoi, x, y, x_hat) for (x, y), x_hat in zip(waves, outs)]
        if args.valid_loss:            # per planned batch, so that the rows of a call do not depend on --gpus or --streams
            for g in call:
                vl = _valid_losses(model, [waves[pos[i]] for i in g], [names[i] for i in g], seed, args.valid_loss,
                                   args.batch, device)
                for i, v in zip(g, vl):
                    metric_rows[pos[i]] = tuple(metric_rows[pos[i]]) + (float(v),)
        for j, db in agree:                                        # --samples D > 1: the last column
            metric_rows[j] = tuple(metric_rows[j]) + (float(db),)
        for i, (_, y), x_hat, m in zip(flat, waves, outs, metric_rows):
            _write_wav(target_dir + "files/" + names[i], x_hat, 16000)
            rows.append((i, names[i]) + tuple(m) + (y.shape[0] // 128 + 1,))
    rows = gather_rows(rows)
    dt = time.time() - t0
    if rank == 0:
        rows.sort(key=lambda r: r[0])                              # the global sorted-filename order
        assert [r[0] for r in rows] == list(range(len(names))), "every utterance exactly once"
        columns = _COLUMNS + (("valid_loss",) if args.valid_loss else ()) + (("agreement_db",) if args.samples > 1 else ())
        data = {c: [r[1 + j] for r in rows] for j, c in enumerate(columns)}
        _write_reports(target_dir, data, args, model, epoch, seed)
        where = f" on {world} GPU(s), keyed noise seed {seed}" if keyed else ""
        print(f"enhanced {len(names)} utterances ({sum(r[-1] for r in rows)} frames) in {dt:.2f} s{where} -> {target_dir}")
    return dt


def main(argv=None):
    ap = build_parser()
    args = parse_args(argv, ap)
    if args.N_mid != 0:
        raise ValueError("N_mid should be 0.")          # evaluate.py:124-125
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:           # plain `python -m flowmse_amd.evaluate --gpus N`
        return _spawn_ranks(args, argv)
    keyed = args.noise == "keyed"      # as one rank of ``--gpus N`` or in-process at ``--gpus 1``: the same plan, the same calls
    rank, world = _enter_rank(args) if keyed else (0, 1)
    seed = None
    if keyed:
        seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(8), "little")
    model, epoch = _load_model(args, ap)
    names, n_samples, load = _sources(args)
    if not keyed and args.seed is not None:
        torch.manual_seed(args.seed)
    run_calls(args, model, epoch, names, n_samples, load, seed, rank, world)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
