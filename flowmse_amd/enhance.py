#!/usr/bin/env python3
"""Enhancement CLI: noisy recordings of any length in, enhanced recordings out.

    python -m flowmse_amd.enhance --input WAV_OR_DIR --output DIR --ckpt MODEL.ckpt [--N 5] [--batch 8]
                                  [--chunk_frames 256] [--overlap_frames 32] [--noise keyed|torch] [--seed S]
                                  [--resample [--output_rate 16000|input]]

Unlike ``flowmse_amd.evaluate`` it needs no clean files and reports no metrics.  Every recording goes through
``flowmse_amd.chunked.enhance_long``: one that fits a single chunk is enhanced exactly as ``evaluate`` would; a longer
one is cut into overlapping chunks of ``--chunk_frames`` frames that are sampled ``--batch`` rows at a time and
cross-faded, so device memory does not grow with the recording.  The chunked mode is NOT the reference's computation
for a long file (each chunk has its own GroupNorm and attention context), and its defaults -- 256 frames, the training
crop, overlapping by 32 -- are chosen values, not tuned ones: no released checkpoint was at hand to listen to the seams.

Output: ``DIR/<name>.wav`` (16-bit PCM; 16 kHz unless ``--output_rate input``) for every input and ``DIR/_settings.txt``
with the arguments and the noise seed.  ``--noise keyed`` (default) addresses the prior noise by (seed, file name, bin, absolute frame): a file's bytes do
not depend on what else is in the folder or on the processing order.  ``--synthetic n`` runs on synthetic weights and
synthetic noisy signals (no checkpoint or input needed).

Sample rates.  The network works at 16 kHz.  Without ``--resample`` nothing here resamples: input that is not 16 kHz is
refused by name before anything is enhanced.  With ``--resample`` a file at any supported rate (``flowmse_amd.resample``:
8 .. 192 kHz, the ratio to 16 kHz at most 1024 after reduction) is moved to the device, brought to 16 kHz there by the
library's polyphase resampler and enhanced as a 16 kHz recording; a 16 kHz file gives the bytes it gives without the flag,
and files at unsupported rates (16 001 Hz, say) are still refused by name first.  The keyed noise stays addressed by (seed, file name, bin,
absolute 16 kHz frame).  ``--output_rate 16000`` (default) writes the enhanced signal at the network's rate;
``--output_rate input`` resamples it back on the device to the file's own rate, trimmed to the input's sample count.  Such a
file carries NOTHING above 8 kHz: the network never saw that band, and the way back only interpolates.
``--synthetic_rate HZ`` generates the synthetic signals at another rate, to exercise all this without a checkpoint.
"""
import argparse
import glob
import os
import time
import types

import torch

from flowmse_amd.chunked import CHUNK_FRAMES, OVERLAP_FRAMES, enhance_long, plan_chunks
from flowmse_amd.evaluate import _load_model, _seconds_arg, _synthetic_pairs, _write_wav
from flowmse_amd.resample import rational, resample
from flowmse_amd.util.noise import utterance_key
from flowmse_amd.util.other import read_wav

SAMPLE_RATE = 16000


def build_parser():
    ap = argparse.ArgumentParser(description="Enhance noisy 16 kHz recordings of any length (no clean files, no metrics); "
                                             "with --resample, recordings at other sample rates too.")
    ap.add_argument("--input", type=str, default=None, help="a wav file, or a directory whose *.wav are enhanced")
    ap.add_argument("--output", type=str, required=True, help="directory for the enhanced wavs and _settings.txt")
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--synthetic", type=int, default=0, help="run on this many synthetic signals with synthetic weights")
    ap.add_argument("--synthetic_seconds", type=_seconds_arg, default=[2.0],
                    help="durations of the synthetic signals in seconds, a comma list cycled over them (default 2.0)")
    ap.add_argument("--N", type=int, default=5)
    ap.add_argument("--odesolver", type=str, default="euler")
    ap.add_argument("--reverse_starting_point", type=float, default=1.0)
    ap.add_argument("--last_eval_point", type=float, default=0.03)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16x3", "bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=8,
                    help="chunk rows of ONE recording per sampler call (rows are never pooled across recordings). Batch "
                         "widths select different kernels: across --batch values a file agrees to fp32 tolerance (about "
                         "1e-5 relative), not byte for byte")
    ap.add_argument("--chunk_frames", type=int, default=CHUNK_FRAMES,
                    help="frames per chunk, a multiple of 64 (default 256, the training crop)")
    ap.add_argument("--overlap_frames", type=int, default=OVERLAP_FRAMES,
                    help="frames two neighbouring chunks share and cross-fade over: even, at most chunk_frames / 2")
    ap.add_argument("--noise", choices=("keyed", "torch"), default="keyed",
                    help="prior noise. keyed: the counter-based stream addressed by (seed, file name, bin, absolute "
                         "frame). torch: the process-wide generator, consumed in processing order")
    ap.add_argument("--seed", type=int, default=None,
                    help="keyed: the 64-bit seed of the stream (default: drawn from os.urandom and recorded in "
                         "_settings.txt). torch: torch.manual_seed before the first draw (default: unseeded)")
    ap.add_argument("--resample", action="store_true",
                    help="accept input at other sample rates (8 .. 192 kHz; the ratio to 16 kHz at most 1024 after reduction) "
                         "and resample it to 16 kHz on the device before it is enhanced. Without it such files are refused")
    ap.add_argument("--output_rate", choices=("16000", "input"), default="16000",
                    help="needs --resample. 16000: write the enhanced signal at the network's rate. input: resample it back "
                         "on the device to the file's own rate, trimmed to the input's sample count; such a file carries "
                         "nothing above 8 kHz (the network never saw that band)")
    ap.add_argument("--synthetic_rate", type=int, default=SAMPLE_RATE, metavar="HZ",
                    help="sample rate of the --synthetic signals (default 16000); any other value needs --resample")
    return ap


def parse_args(argv=None, ap=None):
    ap = ap or build_parser()
    args = ap.parse_args(argv)
    if args.synthetic < 0:
        ap.error(f"--synthetic must be >= 0, got {args.synthetic}")
    if not args.synthetic and not (args.input and args.ckpt):
        ap.error("--input and --ckpt are required unless --synthetic is given")
    if args.batch < 1:
        ap.error(f"--batch must be >= 1, got {args.batch}")
    if args.N < 1:
        ap.error(f"--N must be >= 1, got {args.N}")
    try:
        plan_chunks(1, args.chunk_frames, args.overlap_frames)
    except ValueError as e:
        ap.error(str(e))
    if args.output_rate != "16000" and not args.resample:
        ap.error("--output_rate input needs --resample")
    if args.synthetic_rate != SAMPLE_RATE and not args.resample:
        ap.error(f"--synthetic_rate {args.synthetic_rate} needs --resample")
    try:
        rational(args.synthetic_rate, SAMPLE_RATE)
    except ValueError as e:
        ap.error(f"--synthetic_rate: {e}")
    return args


def list_inputs(path):
    """The wav files ``--input`` names, sorted by base name: the file itself, or the *.wav of a directory."""
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "*.wav")), key=os.path.basename)
        if not files:
            raise SystemExit(f"no *.wav in {path}")
        return files
    if not os.path.isfile(path):
        raise SystemExit(f"--input {path}: no such file or directory")
    return [path]


def sample_rate(path):
    """Sample rate of a wav file, from its header."""
    from scipy.io import wavfile
    try:
        return int(wavfile.read(path, mmap=True)[0])
    except ValueError:                                             # a sample format scipy cannot map
        return int(wavfile.read(path)[0])


def refuse_other_rates(files):
    """Exit, naming them, if any file is not 16 kHz: the network was trained on 16 kHz speech and, without ``--resample``
    (the only case this is called in), nothing here resamples."""
    bad = [(os.path.basename(f), sr) for f, sr in ((f, sample_rate(f)) for f in files) if sr != SAMPLE_RATE]
    if bad:
        raise SystemExit("not 16 kHz (resample first): " + ", ".join(f"{n} ({sr} Hz)" for n, sr in bad))


def resampling_rates(files):
    """The sample rate of every file under ``--resample``.  Exits, naming the files and both rates, if one cannot be
    brought to 16 kHz by a ratio the resampler supports (``flowmse_amd.resample.rational``)."""
    rates = [sample_rate(f) for f in files]
    bad = []
    for f, sr in zip(files, rates):
        try:
            rational(sr, SAMPLE_RATE)
        except ValueError:
            bad.append(f"{os.path.basename(f)} ({sr} Hz)")
    if bad:
        raise SystemExit(f"cannot resample to {SAMPLE_RATE} Hz (the reduced ratio exceeds 1024): " + ", ".join(bad))
    return rates


def enhance_recording(model, y, sr, output_rate="16000", **kw):
    """One recording ``y`` [1, samples] on the device at ``sr`` Hz through resample -> ``enhance_long(**kw)`` [-> resample
    back].  Returns (waveform as numpy, its sample rate, frames of the 16 kHz signal).  At 16 kHz this is ``enhance_long``
    and nothing else.  ``output_rate="input"``: the enhanced waveform stays on the device, is resampled to ``sr`` there and
    trimmed to the input's sample count."""
    y16 = resample(y, sr, SAMPLE_RATE)
    frames = y16.size(1) // 128 + 1
    if output_rate != "input" or sr == SAMPLE_RATE:
        return enhance_long(model, y16, **kw), SAMPLE_RATE, frames
    x_hat = enhance_long(model, y16, as_tensor=True, **kw)
    return resample(x_hat[None], SAMPLE_RATE, sr)[0, :y.size(1)].cpu().numpy(), sr, frames


def write_settings(out_dir, args, model, epoch, noise_seed, resampled=()):
    with open(os.path.join(out_dir, "_settings.txt"), "w") as f:
        f.write(f"epoch: {epoch}\ncheckpoint file: {args.ckpt}\ninput: {args.input}\nsynthetic: {args.synthetic}\n")
        f.write(f"odesolver: {args.odesolver}\nReverse starting point: {args.reverse_starting_point}\n")
        f.write(f"Last evaluated point: {args.last_eval_point}\node: FLOWMATCHING\n")
        f.write(f"sigma_min: {model.ode.sigma_min}\nsigma_max: {model.ode.sigma_max}\nN: {args.N}\n")
        f.write(f"precision: {args.precision}\nbatch: {args.batch}\n")
        f.write(f"chunk_frames: {args.chunk_frames}\noverlap_frames: {args.overlap_frames}\n")
        f.write(f"resample: {args.resample}\noutput_rate: {args.output_rate}\n")
        for name, sr in resampled:
            f.write(f"resampled {name}: {sr} Hz\n")
        f.write(f"seed: {args.seed}\nnoise: {args.noise}\nnoise seed: {noise_seed}\n")


def main(argv=None):
    ap = build_parser()
    args = parse_args(argv, ap)
    if args.synthetic:
        pairs = _synthetic_pairs(args.synthetic, seconds=args.synthetic_seconds, sr=args.synthetic_rate)
        names = [p[0] for p in pairs]
        rates = [args.synthetic_rate] * len(pairs)

        def load(i):
            return torch.from_numpy(pairs[i][2])[None]
    else:
        files = list_inputs(args.input)
        if args.resample:
            rates = resampling_rates(files)
        else:
            refuse_other_rates(files)
            rates = [SAMPLE_RATE] * len(files)
        names = [os.path.basename(f) for f in files]

        def load(i):
            return read_wav(files[i])[0]

    model, epoch = _load_model(types.SimpleNamespace(synthetic=args.synthetic, ckpt=args.ckpt, test_dir=args.input,
                                                     precision=args.precision), ap)
    os.makedirs(args.output, exist_ok=True)
    keyed = args.noise == "keyed"
    seed = None
    if keyed:
        seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(8), "little")
    elif args.seed is not None:
        torch.manual_seed(args.seed)
    frames, t0 = 0, time.time()
    for i, name in enumerate(names):
        y = load(i).cuda()
        x_hat, sr_out, n_frames = enhance_recording(
            model, y, rates[i], args.output_rate, chunk_frames=args.chunk_frames, overlap_frames=args.overlap_frames,
            batch=args.batch, N=args.N, T_rev=args.reverse_starting_point, t_eps=args.last_eval_point,
            odesolver=args.odesolver, noise_key=utterance_key(name) if keyed else None, noise_seed=seed if keyed else 0)
        _write_wav(os.path.join(args.output, name), x_hat, sr_out)
        frames += n_frames
    write_settings(args.output, args, model, epoch, seed,
                   [(n, sr) for n, sr in zip(names, rates) if sr != SAMPLE_RATE])
    print(f"enhanced {len(names)} recordings ({frames} frames) in {time.time() - t0:.2f} s -> {args.output}"
          + (f", keyed noise seed {seed}" if keyed else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
