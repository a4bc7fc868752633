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
"""
import argparse
import csv
import glob
import os
import re
import time

import numpy as np
import torch

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


def enhance_waveform(model, y, N=5, T_rev=1.0, t_eps=0.03, odesolver="euler", z=None, VF_fn=None, device=None,
                     noise_keys=None, noise_seed=0, as_tensor=False):
    """One utterance, evaluate.py:107-136.  y: float tensor [1, samples].  Returns the enhanced waveform (numpy; with
    ``as_tensor`` the same values as a 1-D tensor left on the compute device).
    ``noise_keys`` ([key], see ``flowmse_amd.util.noise.utterance_key``) / ``noise_seed``: keyed prior noise."""
    device = device or y.device
    T_orig = y.size(1)
    norm_factor = y.abs().max().item()
    dm = model.data_module
    fused = VF_fn is None and hasattr(dm, "fused_ok") and dm.fused_ok(y.to(device))
    if fused:                      # STFT + compression + frame padding as one HIP kernel
        Y = dm.analyze(y.to(device) / norm_factor)       # y / max|y| as the reference computes it (evaluate.py:111)
    else:
        y = y / norm_factor
        Y = torch.unsqueeze(model._forward_transform(model._stft(y.to(device))), 0)
        Y = pad_spec(Y)
    sampler = get_white_box_solver(odesolver, model.ode, VF_fn if VF_fn is not None else model, Y=Y, Y_prior=Y,
                                   T_rev=T_rev, t_eps=t_eps, N=N, z=z, noise_keys=noise_keys,
                                   noise_seed=noise_seed)
    sample, _ = sampler()
    if fused:                      # decompression + iSTFT + rescale as one HIP kernel
        x_hat = dm.synthesize(sample, T_orig, norm_factor).reshape(-1)
    else:
        x_hat = (model.to_audio(sample.squeeze(), T_orig) * norm_factor).reshape(-1)
    return x_hat if as_tensor else x_hat.cpu().numpy()


def enhance_batch(model, ys, N=5, T_rev=1.0, t_eps=0.03, odesolver="euler", noise_keys=None, noise_seed=0, as_tensor=False):
    """Several utterances whose padded frame counts agree, as ONE sampler call (the reference enhances one file at
    a time, evaluate.py:97; trajectories are independent, so batching changes nothing but throughput).
    ys: list of float tensors [1, samples_i] on the target device.  Returns a list of numpy waveforms (with ``as_tensor``
    the same values as 1-D tensors left on the device).
    ``noise_keys`` (one key per utterance) / ``noise_seed``: keyed prior noise, which follows the utterance and not its
    row or batch."""
    host = (lambda t: t.reshape(-1)) if as_tensor else (lambda t: t.squeeze().cpu().numpy())
    norms = [y.abs().max().item() for y in ys]
    dm = model.data_module
    fused = hasattr(dm, "fused_ok") and all(dm.fused_ok(y) for y in ys)
    if fused:                      # STFT + compression + frame padding: one HIP kernel per utterance
        specs = [dm.analyze(y / n) for y, n in zip(ys, norms)]
    else:
        specs = [pad_spec(torch.unsqueeze(model._forward_transform(model._stft(y / n)), 0)) for y, n in zip(ys, norms)]
    Y = torch.cat(specs, dim=0)
    sample, _ = get_white_box_solver(odesolver, model.ode, model, Y=Y, Y_prior=Y, T_rev=T_rev, t_eps=t_eps, N=N,
                                     noise_keys=noise_keys, noise_seed=noise_seed)()
    if fused:                      # decompression + iSTFT + rescale: one HIP kernel per utterance
        return [host(dm.synthesize(sample[i:i + 1], y.size(1), n)) for i, (y, n) in enumerate(zip(ys, norms))]
    return [host(model.to_audio(sample[i, 0], y.size(1)) * n) for i, (y, n) in enumerate(zip(ys, norms))]


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
    host = (lambda t: t.reshape(-1)) if as_tensor else (lambda t: t.squeeze().cpu().numpy())
    norms = [y.abs().max().item() for y in ys]
    dm = model.data_module
    fused = hasattr(dm, "fused_ok") and all(dm.fused_ok(y) for y in ys)
    if fused:                      # STFT + compression + frame padding: one HIP kernel per utterance
        specs = [dm.analyze(y / n) for y, n in zip(ys, norms)]
    else:
        specs = [pad_spec(torch.unsqueeze(model._forward_transform(model._stft(y / n)), 0)) for y, n in zip(ys, norms)]
    groups = [[i] for i in range(len(ys))] if groups is None else [list(g) for g in groups]
    Ys = [specs[g[0]] if len(g) == 1 else torch.cat([specs[i] for i in g], dim=0) for g in groups]
    item_keys = None if noise_keys is None else [[noise_keys[i] for i in g] for g in groups]
    samples, _ = get_white_box_solver_multi(odesolver, model.ode, model, Ys, T_rev=T_rev, t_eps=t_eps, N=N, lanes=lanes,
                                            noise_keys=item_keys, noise_seed=noise_seed)()
    out = [None] * len(ys)
    for g, sample in zip(groups, samples):
        for j, i in enumerate(g):
            if fused:              # decompression + iSTFT + rescale: one HIP kernel per utterance
                out[i] = host(dm.synthesize(sample[j:j + 1], ys[i].size(1), norms[i]))
            else:
                out[i] = host(model.to_audio(sample[j, 0], ys[i].size(1)) * norms[i])
    return out


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
    if args.noise is None:
        args.noise = "keyed" if args.gpus > 1 else "torch"
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


def _main_keyed(args, ap):
    """Keyed-noise run, as one rank of ``--gpus N`` or in-process at ``--gpus 1``: the same plan and the same calls."""
    import torch.distributed as dist
    from flowmse_amd.parallel import gather_rows, plan_shards
    from flowmse_amd.util.inference import keyed_valid_losses, validation_item
    from flowmse_amd.util.noise import utterance_key
    rank, world = _enter_rank(args)
    seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(8), "little")
    model, epoch = _load_model(args, ap)
    if args.synthetic:
        pairs = _synthetic_pairs(args.synthetic, seconds=args.synthetic_seconds)
        names = [p[0] for p in pairs]
        n_samples = [p[2].shape[0] for p in pairs]

        def load(i):
            return pairs[i][1], pairs[i][2]
    else:
        clean_dir = os.path.join(args.test_dir, "test", "clean")
        noisy_dir = os.path.join(args.test_dir, "test", "noisy")
        names = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(noisy_dir, "*.wav")))]
        n_samples = [_num_samples(os.path.join(noisy_dir, n)) for n in names]     # headers only: the plan needs every length

        def load(i):
            return (_read_wav(os.path.join(clean_dir, names[i]))[0][0].numpy(),
                    _read_wav(os.path.join(noisy_dir, names[i]))[0][0].numpy())

    target_dir = args.folder_destination.rstrip("/") + "/"
    os.makedirs(target_dir + "files/", exist_ok=True)
    pesq, stoi = _metric_fns()
    kw = dict(N=args.N, T_rev=args.reverse_starting_point, t_eps=args.last_eval_point, odesolver=args.odesolver,
              noise_seed=seed)
    # the batches of the WHOLE set, dealt to the ranks unsplit: batch composition does not depend on the world size
    batches = [ids for _, ids in plan_shards([_padded_frames(n) for n in n_samples], world, args.batch, level=False)[rank]]
    per_call = args.streams * _ITEMS_PER_LANE if args.streams > 1 else 1
    on_device = args.metrics == "device"
    rows, t0 = [], time.time()
    for k in range(0, len(batches), per_call):
        chunk = batches[k:k + per_call]
        flat = [i for g in chunk for i in g]
        waves = {i: load(i) for i in flat}
        ys = [torch.from_numpy(waves[i][1])[None].cuda() for i in flat]
        keys = [utterance_key(names[i]) for i in flat]
        if args.streams > 1:
            pos = {i: j for j, i in enumerate(flat)}
            outs = enhance_concurrent(model, ys, args.streams, groups=[[pos[i] for i in g] for g in chunk],
                                      noise_keys=keys, as_tensor=on_device, **kw)
        else:
            outs = enhance_batch(model, ys, noise_keys=keys, as_tensor=on_device, **kw)
        if on_device:
            metric_rows, outs = _metrics_device(pesq, [(waves[i][0], yd, x_hat) for i, yd, x_hat in zip(flat, ys, outs)])
        else:
            metric_rows = [_metrics(pesq, stoi, waves[i][0], waves[i][1], x_hat) for i, x_hat in zip(flat, outs)]
        if args.valid_loss:            # per planned batch, so that the rows of a call do not depend on --gpus or --streams
            at = {i: j for j, i in enumerate(flat)}
            for g in chunk:
                items = [validation_item(model, torch.from_numpy(waves[i][0])[None].cuda(),
                                         torch.from_numpy(waves[i][1])[None].cuda()) for i in g]
                vl = keyed_valid_losses(model, items, [names[i] for i in g], seed=seed, draws=args.valid_loss,
                                        batch=args.batch)
                for i, v in zip(g, vl):
                    metric_rows[at[i]] = tuple(metric_rows[at[i]]) + (float(v),)
        for i, x_hat, m in zip(flat, outs, metric_rows):
            y = waves[i][1]
            _write_wav(target_dir + "files/" + names[i], x_hat, 16000)
            rows.append((i, names[i]) + m + (y.shape[0] // 128 + 1,))
    rows = gather_rows(rows)
    dt = time.time() - t0
    if rank == 0:
        rows.sort(key=lambda r: r[0])                              # the global sorted-filename order
        assert [r[0] for r in rows] == list(range(len(names))), "every utterance exactly once"
        columns = _COLUMNS + (("valid_loss",) if args.valid_loss else ())
        data = {c: [r[1 + j] for r in rows] for j, c in enumerate(columns)}
        _write_reports(target_dir, data, args, model, epoch, seed)
        print(f"enhanced {len(names)} utterances ({sum(r[-1] for r in rows)} frames) in {dt:.2f} s on {world} GPU(s), "
              f"keyed noise seed {seed} -> {target_dir}")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main(argv=None):
    ap = build_parser()
    args = parse_args(argv, ap)
    if args.N_mid != 0:
        raise ValueError("N_mid should be 0.")          # evaluate.py:124-125
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:           # plain `python -m flowmse_amd.evaluate --gpus N`
        return _spawn_ranks(args, argv)
    if args.noise == "keyed":
        return _main_keyed(args, ap)

    model, epoch = _load_model(args, ap)
    if args.synthetic:
        pairs = _synthetic_pairs(args.synthetic, seconds=args.synthetic_seconds)
    else:
        clean_dir = os.path.join(args.test_dir, "test", "clean")
        noisy_dir = os.path.join(args.test_dir, "test", "noisy")
        pairs = []
        for f in sorted(glob.glob(os.path.join(noisy_dir, "*.wav"))):
            name = os.path.basename(f)
            pairs.append((name, _read_wav(os.path.join(clean_dir, name))[0][0].numpy(), _read_wav(f)[0][0].numpy()))

    target_dir = args.folder_destination.rstrip("/") + "/"
    os.makedirs(target_dir + "files/", exist_ok=True)
    pesq, stoi = _metric_fns()
    data = {c: [] for c in _COLUMNS}
    sr = 16000
    frames, t0 = 0, time.time()
    from flowmse_amd.parallel import batches_by_length
    enhanced = {}
    on_device = args.metrics == "device"
    metric_rows = {}                   # --metrics device: idx -> row, filled after each sampler call

    def keep(ids, ys, outs):
        if on_device:
            rows, outs = _metrics_device(pesq, [(pairs[i][1], y, o) for i, y, o in zip(ids, ys, outs)], sr)
            metric_rows.update(dict(zip(ids, rows)))
        enhanced.update(dict(zip(ids, outs)))

    if args.seed is not None:
        torch.manual_seed(args.seed)
    if args.streams > 1:               # utterances (or equal-length batches of them) dealt to concurrent lanes
        lens = [_padded_frames(p[2].shape[0]) for p in pairs]
        items = [ids for _, ids in batches_by_length(range(len(pairs)), lens, args.batch)] if args.batch > 1 \
            else [[i] for i in range(len(pairs))]
        per_call = args.streams * _ITEMS_PER_LANE
        for k in range(0, len(items), per_call):
            chunk = items[k:k + per_call]
            flat = [i for g in chunk for i in g]
            pos = {i: j for j, i in enumerate(flat)}
            ys = [torch.from_numpy(pairs[i][2])[None].cuda() for i in flat]
            outs = enhance_concurrent(model, ys, args.streams,
                                      N=args.N, T_rev=args.reverse_starting_point, t_eps=args.last_eval_point,
                                      odesolver=args.odesolver, groups=[[pos[i] for i in g] for g in chunk],
                                      as_tensor=on_device)
            keep(flat, ys, outs)
    elif args.batch > 1:               # group by padded frame count, largest first
        lens = [_padded_frames(p[2].shape[0]) for p in pairs]
        for _, ids in batches_by_length(range(len(pairs)), lens, args.batch):
            ys = [torch.from_numpy(pairs[i][2])[None].cuda() for i in ids]
            outs = enhance_batch(model, ys, N=args.N,
                                 T_rev=args.reverse_starting_point, t_eps=args.last_eval_point,
                                 odesolver=args.odesolver, as_tensor=on_device)
            keep(ids, ys, outs)
    for idx, (name, x, y) in enumerate(pairs):
        if idx not in enhanced:
            yd = torch.from_numpy(y)[None].cuda()
            keep([idx], [yd], [enhance_waveform(model, yd, N=args.N,
                                                T_rev=args.reverse_starting_point, t_eps=args.last_eval_point,
                                                odesolver=args.odesolver, as_tensor=on_device)])
        x_hat = enhanced.pop(idx)
        frames += y.shape[0] // 128 + 1
        _write_wav(target_dir + "files/" + name, x_hat, sr)
        for c, v in zip(_COLUMNS, (name,) + (metric_rows[idx] if on_device else _metrics(pesq, stoi, x, y, x_hat, sr))):
            data[c].append(v)
    dt = time.time() - t0

    _write_reports(target_dir, data, args, model, epoch, None)
    print(f"enhanced {len(pairs)} utterances ({frames} frames) in {dt:.2f} s -> {target_dir}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
