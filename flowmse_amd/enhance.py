#!/usr/bin/env python3
"""Enhancement CLI: noisy recordings of any length in, enhanced recordings out.

    python -m flowmse_amd.enhance --input WAV_OR_DIR --output DIR --ckpt MODEL.ckpt [--N 5] [--batch 8]
                                  [--chunk_frames 256] [--overlap_frames 32] [--noise keyed|torch] [--seed S]
                                  [--resample [--output_rate 16000|input]] [--pool [--channels first|all] [--samples D]]
    ... | python -m flowmse_amd.enhance --live --ckpt MODEL.ckpt [--live_rate HZ [--output_rate input]] | ...
    ... | python -m flowmse_amd.enhance --live --ckpt MODEL.ckpt --live_channels C [--live_rate HZ --live_resample] | ...

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

Pooling.  Without ``--pool`` a sampler call holds rows of ONE recording, so a folder of short clips runs at batch width 1.
``--pool`` (``flowmse_amd.pooled``) cuts the rows of all files -- one per (file, channel, chunk) -- into calls of exactly
``--batch`` rows; a file's bytes still depend on the file, its name, the seed and the settings only, not on the folder.  At
``--batch 1`` a mono file gets the bytes it gets without the flag; at wider batches it agrees to fp32 tolerance.  Keyed noise
only.  ``--channels all`` (needs ``--pool``) enhances every channel of a multi-channel file independently, normalised by one
factor per file, and writes a file with the input's channel count; ``--channels first`` (default) reads channel 0, as ever.
``--synthetic_channels 1,2,...`` gives the synthetic signals that many channels (channel c > 0: an independent signal at
half the level of channel 0).

Ensembles.  ``--samples D`` (1..64, needs ``--pool``; ``flowmse_amd.ensemble``) samples every row ``D`` times under the keys
``draw_key(channel_key, d)`` and writes the MEAN of the ``D`` draws, taken on the linear spectra on the device before the one
inverse STFT (and before ``--output_rate input`` resamples back).  This is NOT the reference's computation, which draws once.
``_ensemble.csv`` (``filename,channel,samples,agreement_db``) says per file and channel how far the draws agree -- the mean's
power over the draws' deviation from it, in dB: high means the model is sure, around 0 dB or below the output is mostly the
draw.  Draw 0 is the draw of a run without the flag, bit for bit, and ``--samples 1`` is that run.  A file's stack of sampled
rows is ``D`` times as large (512 KB per chunk and draw at 256 frames).

Live.  ``--live --ckpt MODEL.ckpt`` (``flowmse_amd.live``) reads raw mono 16 kHz PCM from stdin (``--live_pcm s16le|f32le``),
``--live_block`` samples at a time, and writes the enhanced PCM to stdout in the same format as soon as it is final, flushed
after every block: ``arecord -t raw -f S16_LE -r 16000 | python -m flowmse_amd.enhance --live --ckpt m.ckpt | aplay ...``.  The
bytes are those of the chunked file mode at ``--batch 1`` for the finished recording under the noise key of the name
``live``, when ``--live_norm`` is the recording's peak; ``--live_norm first`` (default) takes the peak of the samples that
make the first chunk ready.  The output trails the input by at most ``128 chunk_frames + 382`` samples (2.07 s at the default
256 frames, 0.54 s at 64) plus the sampler's compute time.  Nothing but PCM goes to stdout; messages go to stderr.  The
file-mode options that make no sense on one open stream (``--input``, ``--output``, ``--pool``, ``--resample``, ``--samples``
> 1, ``--channels all``, ``--noise torch``) are refused by name.  ``--synthetic 1`` stands in for a checkpoint (synthetic
weights); stdin is still the signal.  ``--live_rate HZ`` (default 16000) names the rate of stdin: the stream is resampled to
16 kHz on the device as it arrives (``flowmse_amd.resample.StreamResampler``, the file mode's filter sample for sample), and
with ``--output_rate input`` the enhanced stream is resampled back, as many samples out as came in: ``arecord -t raw -f S16_LE
-r 48000 | python -m flowmse_amd.enhance --live --live_rate 48000 --output_rate input --ckpt m.ckpt | aplay -t raw -f S16_LE
-r 48000``.  The bytes are then those of the file mode under ``--resample`` with the same ``--output_rate`` (at ``--batch 1``,
``--live_norm`` the peak of the resampled recording).  ``--live_block`` and the latency count samples at ``--live_rate``;
a rate whose ratio to 16 kHz the resampler does not support is refused by name.  ``--resample`` itself stays a file-mode flag.
``--live_channels C`` (default 1; ``flowmse_amd.livepool``) reads and writes interleaved frames of ``C`` channels: ``arecord -t
raw -f S16_LE -r 16000 -c 2 | python -m flowmse_amd.enhance --live --live_channels 2 --ckpt m.ckpt | aplay -t raw -f S16_LE -r
16000 -c 2``.  The stream is one session of a ``LivePool`` of width ``C`` under the keys ``channel_key("live", c)``, normalised by
one factor over all channels, and the bytes are those of ``--pool --channels all --batch C`` on the finished recording alone.
``C = 1`` is the path above, byte for byte.  ``C > 1`` runs at 16 kHz only: with another ``--live_rate`` it is refused by name,
unless ``--live_resample`` is given.  ``--live_resample`` (needs ``--live``, ``C > 1`` and a ``--live_rate`` other than 16000)
opens the session at ``--live_rate``: stdin is interleaved PCM at that rate, the pool resamples all channels to 16 kHz in one
launch per step, and with ``--output_rate input`` back again in a second one, as many frames out as came in: ``arecord -t raw
-f S16_LE -r 48000 -c 2 | python -m flowmse_amd.enhance --live --live_channels 2 --live_rate 48000 --live_resample --output_rate
input --ckpt m.ckpt | aplay -t raw -f S16_LE -r 48000 -c 2``.  ``--live_norm`` applies to the 16 kHz signal; ``--live_block``
and the latency line count frames at ``--live_rate``.

Trailing chunks.  ``--hop_frames H [--fade_frames X]`` (``flowmse_amd.chunked.enhance_trailing``; opt-in and NOT the
reference's computation) slides the chunk of ``--chunk_frames`` frames by ``H`` frames (even, 4 .. chunk_frames), uses its
older ``chunk_frames - H`` frames as context only and keeps its tail, cross-faded over the ``X`` frames (default 0; at most
``H``, ``H + X <= chunk_frames``) before each hop.  With ``--live`` the output then trails the input by ``128 (H + X) + 382``
samples instead of ``128 chunk_frames + 382`` -- 0.184 s at ``--chunk_frames 64 --hop_frames 16 --fade_frames 4`` -- at
``chunk_frames / H`` network rows per ``H`` frames: ``arecord -t raw -f S16_LE -r 16000 | python -m flowmse_amd.enhance --live
--chunk_frames 64 --hop_frames 16 --fade_frames 4 --ckpt m.ckpt | aplay ...``.  In file mode every recording goes through
``enhance_trailing`` (``--resample`` works around it as around ``enhance_long``), and the bytes of ``--batch 1`` are those of
``--live`` with the same flags when ``--live_norm`` is the recording's peak.  One mono recording or stream under keyed noise:
with ``--pool``, ``--samples`` > 1, ``--channels all``, ``--live_channels`` > 1, ``--noise torch`` or an explicit
``--overlap_frames`` the flags are refused by name before anything is enhanced, as is ``--fade_frames`` without
``--hop_frames``.  ``H`` and ``X`` have not been chosen by listening: no released checkpoint was at hand.
"""
import argparse
import csv
import glob
import os
import time
import types

import torch

from flowmse_amd.chunked import CHUNK_FRAMES, OVERLAP_FRAMES, enhance_long, enhance_trailing, plan_chunks, plan_trailing
from flowmse_amd.ensemble import samples_arg
from flowmse_amd.evaluate import _load_model, _seconds_arg, _synthetic_pairs, _write_wav
from flowmse_amd.live import PCM_FORMATS, pcm_decode, pcm_deinterleave, pcm_encode, pcm_interleave
from flowmse_amd.livepool import MAX_WIDTH
from flowmse_amd.pooled import MAX_BATCH, channel_key, enhance_pooled
from flowmse_amd.resample import out_len, rational, resample
from flowmse_amd.util.noise import utterance_key
from flowmse_amd.util.other import read_wav, read_wav_channels

SAMPLE_RATE = 16000


def _channels_arg(v):
    try:
        chans = [int(x) for x in v.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--synthetic_channels takes a comma list of channel counts, got {v!r}")
    if not chans or min(chans) < 1:
        raise argparse.ArgumentTypeError(f"--synthetic_channels takes counts >= 1, got {v!r}")
    return chans


def build_parser():
    ap = argparse.ArgumentParser(description="Enhance noisy 16 kHz recordings of any length (no clean files, no metrics); "
                                             "with --resample, recordings at other sample rates too.")
    ap.add_argument("--input", type=str, default=None, help="a wav file, or a directory whose *.wav are enhanced")
    ap.add_argument("--output", type=str, default=None,
                    help="directory for the enhanced wavs and _settings.txt (required unless --live)")
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
                    help="chunk rows of ONE recording per sampler call (rows are pooled across recordings only with --pool, "
                         f"which makes every call exactly this wide and takes at most {MAX_BATCH}). Batch widths select different kernels: across --batch "
                         "values a file agrees to fp32 tolerance (about 1e-5 relative), not byte for byte")
    ap.add_argument("--chunk_frames", type=int, default=CHUNK_FRAMES,
                    help="frames per chunk, a multiple of 64 (default 256, the training crop)")
    ap.add_argument("--overlap_frames", type=int, default=None,
                    help=f"frames two neighbouring chunks share and cross-fade over: even, at most chunk_frames / 2 (default "
                         f"{OVERLAP_FRAMES})")
    ap.add_argument("--hop_frames", type=int, default=None, metavar="H",
                    help="trailing chunks (flowmse_amd.chunked.enhance_trailing; not the reference's computation): slide the "
                         "chunk by H frames (even, 4..chunk_frames), use its older chunk_frames - H frames as context only and "
                         "keep its tail. With --live the output trails the input by 128 (H + X) + 382 samples instead of 128 "
                         "chunk_frames + 382, at chunk_frames / H network rows per H frames. One mono recording or stream, keyed "
                         "noise; not with --overlap_frames, --pool, --samples > 1, --channels all or --live_channels > 1")
    ap.add_argument("--fade_frames", type=int, default=0, metavar="X",
                    help="needs --hop_frames. Frames before each hop that are cross-faded from the chunk before (0..H, H + X "
                         "<= chunk_frames; default 0)")
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
                    help="needs --resample (or --live --live_rate). 16000: write the enhanced signal at the network's rate. input: resample it back "
                         "on the device to the file's own rate, trimmed to the input's sample count; such a file carries "
                         "nothing above 8 kHz (the network never saw that band)")
    ap.add_argument("--synthetic_rate", type=int, default=SAMPLE_RATE, metavar="HZ",
                    help="sample rate of the --synthetic signals (default 16000); any other value needs --resample")
    ap.add_argument("--pool", action="store_true",
                    help="fill every sampler call with --batch rows taken across recordings and channels "
                         "(flowmse_amd.pooled); needs --noise keyed. A file's bytes do not depend on the rest of the folder")
    ap.add_argument("--channels", choices=("first", "all"), default="first",
                    help="first: enhance channel 0 of a multi-channel file (default). all: needs --pool; enhance every "
                         "channel independently and write a file with the input's channel count")
    ap.add_argument("--samples", type=samples_arg, default=1, metavar="D",
                    help="needs --pool. Sample every row D times (1..64) under independent keyed streams and write the mean of "
                         "the draws, with _ensemble.csv: per file and channel the agreement of the draws in dB. Not the "
                         "reference's computation (it draws once). 1 (default): one draw, the files written without the flag")
    ap.add_argument("--synthetic_channels", type=_channels_arg, default=[1],
                    help="channel counts of the --synthetic signals, a comma list cycled over them (default 1); channel "
                         "c > 0 is an independent signal at half the level of channel 0")
    ap.add_argument("--live", action="store_true",
                    help="enhance raw mono PCM (16 kHz, or --live_rate) from stdin to stdout as it arrives (flowmse_amd.live): the bytes of the "
                         "chunked file mode at --batch 1, at most 128 chunk_frames + 382 samples behind the input")
    ap.add_argument("--live_pcm", choices=tuple(PCM_FORMATS), default="s16le",
                    help="needs --live. Sample format of stdin and stdout (default s16le; output rounded to nearest, saturated)")
    ap.add_argument("--live_block", type=int, default=2048, metavar="N",
                    help="needs --live. Samples read from stdin per push (default 2048); stdout is flushed after each")
    ap.add_argument("--live_norm", type=_live_norm_arg, default="first", metavar="FLOAT|first",
                    help="needs --live. The peak the signal is normalised by: a positive number (the recording's max|y| gives "
                         "the file mode's bytes), or 'first' (default): the peak of the samples that make the first chunk ready")
    ap.add_argument("--live_rate", type=int, default=SAMPLE_RATE, metavar="HZ",
                    help="needs --live. Sample rate of stdin (default 16000): the stream is resampled to 16 kHz on the device "
                         "as it arrives (the ratio to 16 kHz at most 1024 after reduction). stdout is at 16 kHz, or with "
                         "--output_rate input at this rate, as many samples as were read")
    ap.add_argument("--live_channels", type=int, default=1, metavar="C",
                    help="needs --live. Channels of stdin and stdout, interleaved frame after frame (default 1). C > 1 enhances "
                         "the channels independently in sampler calls of C rows (flowmse_amd.livepool), one normalisation "
                         "for all of them; 16 kHz only, unless --live_resample is given")
    ap.add_argument("--live_resample", action="store_true",
                    help="needs --live, --live_channels C > 1 and a --live_rate other than 16000. stdin is interleaved PCM at "
                         "--live_rate: the live pool resamples all channels to 16 kHz in one launch per step, and with "
                         "--output_rate input back again, as many frames out as came in")
    return ap


def _live_norm_arg(v):
    if v == "first":
        return v
    try:
        f = float(v)
    except ValueError:
        f = -1.0
    if not 0.0 < f < float("inf"):
        raise argparse.ArgumentTypeError(f"--live_norm takes a positive number or 'first', got {v!r}")
    return f


def _check_solver(args, ap):
    """``--N`` and the chunk geometry.  ``--live`` and the file mode each call this where they always checked them, so that an
    argv that breaks several rules is still told the same one first."""
    if args.N < 1:
        ap.error(f"--N must be >= 1, got {args.N}")
    try:
        plan_chunks(1, args.chunk_frames, args.overlap_frames)
    except ValueError as e:
        ap.error(str(e))


def _solver_kw(args):
    """The geometry and solver keywords that every sampler entry takes."""
    return dict(chunk_frames=args.chunk_frames, overlap_frames=args.overlap_frames, N=args.N,
                T_rev=args.reverse_starting_point, t_eps=args.last_eval_point, odesolver=args.odesolver)


def _check_live(args, ap):
    """``--live`` reads one open stream: every option that names files, pools rows or draws unkeyed noise is refused."""
    for given, name in ((args.input is not None, "--input"), (args.output is not None, "--output"), (args.pool, "--pool"),
                        (args.resample, "--resample"), (args.samples > 1, f"--samples {args.samples}"),
                        (args.channels == "all", "--channels all"), (args.noise != "keyed", f"--noise {args.noise}")):
        if given:
            ap.error(f"--live does not take {name}: it enhances one mono 16 kHz stream from stdin to stdout with keyed noise")
    if args.live_block < 1:
        ap.error(f"--live_block must be >= 1, got {args.live_block}")
    try:
        rational(args.live_rate, SAMPLE_RATE)
    except ValueError as e:
        ap.error(f"--live_rate: {e}")
    if not 1 <= args.live_channels <= MAX_WIDTH:
        ap.error(f"--live_channels must be 1..{MAX_WIDTH}, got {args.live_channels}")
    if args.live_resample and args.live_rate == SAMPLE_RATE:
        ap.error(f"--live_resample needs a --live_rate other than {SAMPLE_RATE}: at {SAMPLE_RATE} Hz there is nothing to resample")
    if args.live_resample and args.live_channels == 1:
        ap.error("--live_resample needs --live_channels C > 1 (the live pool's resamplers); one channel at another "
                 "--live_rate takes no flag")
    if args.live_channels > 1 and args.live_rate != SAMPLE_RATE and not args.live_resample:
        ap.error(f"--live_channels {args.live_channels} does not take --live_rate {args.live_rate}: the live pool runs at "
                 f"{SAMPLE_RATE} Hz only (--live_resample puts its resamplers around it)")
    if not args.synthetic and not args.ckpt:
        ap.error("--live needs --ckpt (or --synthetic 1 for synthetic weights)")
    _check_solver(args, ap)
    return args


def _check_trailing(args, ap):
    """``--hop_frames`` / ``--fade_frames``: one mono recording or stream under keyed noise, in the geometry of
    ``plan_trailing``; everything that pools rows, draws several times or names the other geometry is refused by name."""
    if args.hop_frames is None:
        if args.fade_frames:
            ap.error(f"--fade_frames {args.fade_frames} needs --hop_frames")
        return
    for given, name in ((args.pool, "--pool"), (args.samples > 1, f"--samples {args.samples}"),
                        (args.channels == "all", "--channels all"),
                        (args.live_channels > 1, f"--live_channels {args.live_channels}"),
                        (args.noise != "keyed", f"--noise {args.noise}"),
                        (args.overlap_frames is not None, f"--overlap_frames {args.overlap_frames}")):
        if given:
            ap.error(f"--hop_frames does not take {name}: trailing chunks enhance one mono recording or stream with keyed "
                     "noise, and their overlap is chunk_frames - hop_frames")
    try:
        plan_trailing(1, args.chunk_frames, args.hop_frames, args.fade_frames)
    except ValueError as e:
        ap.error(str(e))


def parse_args(argv=None, ap=None):
    ap = ap or build_parser()
    args = ap.parse_args(argv)
    _check_trailing(args, ap)
    if args.overlap_frames is None:
        args.overlap_frames = OVERLAP_FRAMES
    if args.live:
        return _check_live(args, ap)
    if args.live_rate != SAMPLE_RATE:
        ap.error(f"--live_rate {args.live_rate} needs --live (files at other rates take --resample)")
    if args.live_channels != 1:
        ap.error(f"--live_channels {args.live_channels} needs --live (files with several channels take --pool --channels all)")
    if args.live_resample:
        ap.error("--live_resample needs --live (files at other rates take --resample)")
    if args.output is None:
        ap.error("the following arguments are required: --output")
    if args.synthetic < 0:
        ap.error(f"--synthetic must be >= 0, got {args.synthetic}")
    if not args.synthetic and not (args.input and args.ckpt):
        ap.error("--input and --ckpt are required unless --synthetic is given")
    if args.batch < 1:
        ap.error(f"--batch must be >= 1, got {args.batch}")
    _check_solver(args, ap)
    if args.channels == "all" and not args.pool:
        ap.error("--channels all needs --pool")
    if args.samples > 1 and not args.pool:
        ap.error(f"--samples {args.samples} needs --pool (the unpooled path draws once)")
    if args.pool and args.noise != "keyed":
        ap.error("--pool --noise torch: pooling needs --noise keyed (the generator's draw order would depend on the folder)")
    if args.pool and args.batch > MAX_BATCH:
        ap.error(f"--pool takes --batch up to {MAX_BATCH}, got {args.batch}")
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


def wav_shape(path):
    """(samples per channel, channels) of a wav file, which the ``--pool`` plan needs before any file is loaded.  From the
    header where scipy can map the samples; a sample format it cannot map (24-bit, say) is read in full here, so a
    pooled run reads such a file twice."""
    from scipy.io import wavfile
    try:
        data = wavfile.read(path, mmap=True)[1]
    except ValueError:                                             # a sample format scipy cannot map
        data = wavfile.read(path)[1]
    return int(data.shape[0]), (1 if data.ndim == 1 else int(data.shape[1]))


def synthetic_signals(n, seconds, channels, sr):
    """``[(name, float32 [C, samples])]``: channel 0 is the noisy signal of ``evaluate._synthetic_pairs``; channel c > 0 an
    independent tone-plus-noise signal at half that level.  ``channels``: counts cycled over the signals."""
    import numpy as np
    out = []
    for i, (name, _, noisy) in enumerate(_synthetic_pairs(n, seconds=seconds, sr=sr)):
        rows = [noisy]
        t = np.arange(noisy.shape[0]) / sr
        for c in range(1, channels[i % len(channels)]):
            g = np.random.default_rng([1, i, c])
            tone = 0.3 * np.sin(2 * np.pi * (230 + 60 * i + 45 * c) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t + c))
            rows.append((0.5 * (tone + 0.05 * g.standard_normal(t.shape))).astype(np.float32))
        out.append((name, np.stack(rows)))
    return out


def run_pooled(model, args, names, rates, shapes, read, seed):
    """The ``--pool`` run: ``read(i)`` -> float32 [C, samples] on the host at ``rates[i]`` Hz, ``shapes[i]`` its (samples,
    channels).  Every file is moved to the device, brought to 16 kHz there (all channels in one launch), enhanced by
    ``enhance_pooled`` and written as it completes (``--output_rate input``: resampled back and trimmed first).  Returns
    the real 16 kHz frames enhanced, channels counted.  ``--samples D > 1``: the mean of D draws, and ``_ensemble.csv``."""
    every = args.channels == "all"
    items = []
    for name, sr, (n, C) in zip(names, rates, shapes):
        up, down = rational(sr, SAMPLE_RATE)
        items.append((name, C if every else 1, out_len(n, up, down)))

    def load(i):
        y = read(i)
        return resample((y if every else y[:1]).cuda(), rates[i], SAMPLE_RATE)

    def write(i, x_hat):
        sr = SAMPLE_RATE
        if args.output_rate == "input" and rates[i] != SAMPLE_RATE:
            sr = rates[i]
            x_hat = resample(x_hat, SAMPLE_RATE, sr)[:, :shapes[i][0]]
        x = x_hat.cpu().numpy()
        _write_wav(os.path.join(args.output, names[i]), x[0] if x.shape[0] == 1 else x.T, sr)

    agree = {}
    enhance_pooled(model, load, items, write, batch=args.batch, **_solver_kw(args), noise_seed=seed,
                   draws=tuple(range(args.samples)), agreement=agree.__setitem__)
    if args.samples > 1:
        with open(os.path.join(args.output, "_ensemble.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["filename", "channel", "samples", "agreement_db"])
            for i, name in enumerate(names):
                for c, db in enumerate(agree[i]):
                    w.writerow([name, c, args.samples, db])
    return sum(C * (L // 128 + 1) for _, C, L in items)


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


def enhance_recording(model, y, sr, output_rate="16000", hop_frames=None, fade_frames=0, **kw):
    """One recording ``y`` [1, samples] on the device at ``sr`` Hz through resample -> ``enhance_long(**kw)`` [-> resample
    back].  Returns (waveform as numpy, its sample rate, frames of the 16 kHz signal).  At 16 kHz this is ``enhance_long``
    and nothing else.  ``output_rate="input"``: the enhanced waveform stays on the device, is resampled to ``sr`` there and
    trimmed to the input's sample count.  With ``hop_frames`` the core is ``enhance_trailing(hop_frames, fade_frames, **kw)``
    (``overlap_frames`` is not read)."""
    core = enhance_long
    if hop_frames is not None:
        kw.pop("overlap_frames", None)

        def core(model, y16, **kw):
            return enhance_trailing(model, y16, hop_frames=hop_frames, fade_frames=fade_frames, **kw)
    y16 = resample(y, sr, SAMPLE_RATE)
    frames = y16.size(1) // 128 + 1
    if output_rate != "input" or sr == SAMPLE_RATE:
        return core(model, y16, **kw), SAMPLE_RATE, frames
    x_hat = core(model, y16, as_tensor=True, **kw)
    return resample(x_hat[None], SAMPLE_RATE, sr)[0, :y.size(1)].cpu().numpy(), sr, frames


def write_settings(out_dir, args, model, epoch, noise_seed, resampled=()):
    with open(os.path.join(out_dir, "_settings.txt"), "w") as f:
        f.write(f"epoch: {epoch}\ncheckpoint file: {args.ckpt}\ninput: {args.input}\nsynthetic: {args.synthetic}\n")
        f.write(f"odesolver: {args.odesolver}\nReverse starting point: {args.reverse_starting_point}\n")
        f.write(f"Last evaluated point: {args.last_eval_point}\node: FLOWMATCHING\n")
        f.write(f"sigma_min: {model.ode.sigma_min}\nsigma_max: {model.ode.sigma_max}\nN: {args.N}\n")
        f.write(f"precision: {args.precision}\nbatch: {args.batch}\n")
        f.write(f"chunk_frames: {args.chunk_frames}\noverlap_frames: {args.overlap_frames}\n")
        if getattr(args, "hop_frames", None) is not None:          # without the flag the file is what it always was
            f.write(f"hop_frames: {args.hop_frames}\nfade_frames: {args.fade_frames}\n")
        f.write(f"resample: {args.resample}\noutput_rate: {args.output_rate}\n")
        if args.pool:                                              # without the flag the file is what it always was
            f.write(f"pool: {args.pool}\nchannels: {args.channels}\n")
        if getattr(args, "samples", 1) > 1:
            f.write(f"samples: {args.samples}\n")
        for name, sr in resampled:
            f.write(f"resampled {name}: {sr} Hz\n")
        f.write(f"seed: {args.seed}\nnoise: {args.noise}\nnoise seed: {noise_seed}\n")


def run_live(args, ap):
    """The ``--live`` run: PCM blocks from stdin through one ``LiveEnhancer`` to stdout, flushed after every push.  Returns
    the samples written."""
    import sys
    from flowmse_amd.live import LiveEnhancer
    stdin, stdout = sys.stdin.buffer, sys.stdout.buffer
    text_out, sys.stdout = sys.stdout, sys.stderr                  # nothing but PCM may reach stdout
    try:
        model, _ = _load_model(types.SimpleNamespace(synthetic=args.synthetic, ckpt=args.ckpt, test_dir="stdin",
                                                     precision=args.precision), ap)
        seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(8), "little")
        if args.live_channels > 1:
            return _run_live_channels(args, model, seed, stdin, stdout)
        live = LiveEnhancer(model, norm=args.live_norm, key=utterance_key("live"), seed=seed, **_solver_kw(args),
                            input_rate=args.live_rate, output_rate=args.output_rate, hop_frames=args.hop_frames,
                            fade_frames=args.fade_frames)
        if args.live_rate != SAMPLE_RATE:
            print(f"live: {args.live_rate} Hz in, {args.live_rate if args.output_rate == 'input' else SAMPLE_RATE} Hz out",
                  file=sys.stderr)
        print(f"live: keyed noise seed {seed}, {args.live_pcm}, blocks of {args.live_block}, at most "
              f"{live.latency_samples} samples ({live.latency_samples / args.live_rate:.2f} s) behind the input", file=sys.stderr)
        width, t0 = PCM_FORMATS[args.live_pcm], time.time()
        while True:
            data = stdin.read(args.live_block * width)
            if not data:
                break
            stdout.write(pcm_encode(live.push(pcm_decode(data, args.live_pcm)), args.live_pcm))
            stdout.flush()
        stdout.write(pcm_encode(live.finish(), args.live_pcm))
        stdout.flush()
        print(f"live: enhanced {live.samples_out} samples in {time.time() - t0:.2f} s", file=sys.stderr)
        return live.samples_out
    finally:
        sys.stdout = text_out


def _run_live_channels(args, model, seed, stdin, stdout):
    """``--live --live_channels C``, ``C > 1``: interleaved frames through one session of a ``LivePool`` of width ``C``, one
    ``step()`` per block.  Returns the frames written."""
    import sys
    from flowmse_amd.live import latency_samples
    from flowmse_amd.livepool import LivePool
    C = args.live_channels
    pool = LivePool(model, width=C, seed=seed, **_solver_kw(args))
    if args.live_resample:                                         # frames at --live_rate in, and with --output_rate input out
        session = pool.open([channel_key("live", c) for c in range(C)], args.live_norm, input_rate=args.live_rate,
                            output_rate=args.output_rate)
        latency = session.latency_samples
        print(f"live: {args.live_rate} Hz in, {args.live_rate if args.output_rate == 'input' else SAMPLE_RATE} Hz out",
              file=sys.stderr)
    else:
        session = pool.open([channel_key("live", c) for c in range(C)], args.live_norm)
        latency = latency_samples(args.chunk_frames)
    print(f"live: {C} channels, keyed noise seed {seed}, {args.live_pcm}, blocks of {args.live_block} frames, at most "
          f"{latency} samples ({latency / args.live_rate:.2f} s) behind the input", file=sys.stderr)
    width, t0 = PCM_FORMATS[args.live_pcm], time.time()

    def deliver():
        for _, x in pool.step():
            stdout.write(pcm_encode(pcm_interleave(x), args.live_pcm))
        stdout.flush()

    while True:
        data = stdin.read(args.live_block * width * C)
        if not data:
            break
        session.push(pcm_deinterleave(pcm_decode(data, args.live_pcm), C))
        deliver()
    session.finish()
    deliver()
    print(f"live: enhanced {session.samples_out} frames of {C} channels in {time.time() - t0:.2f} s", file=sys.stderr)
    return session.samples_out


def main(argv=None):
    ap = build_parser()
    args = parse_args(argv, ap)
    if args.live:
        run_live(args, ap)
        return 0
    if args.synthetic:
        signals = synthetic_signals(args.synthetic, args.synthetic_seconds, args.synthetic_channels, args.synthetic_rate)
        names = [p[0] for p in signals]
        rates = [args.synthetic_rate] * len(signals)
        shapes = [(p[1].shape[1], p[1].shape[0]) for p in signals]

        def read(i):
            return torch.from_numpy(signals[i][1])

        def load(i):
            return read(i)[:1]
    else:
        files = list_inputs(args.input)
        if args.resample:
            rates = resampling_rates(files)
        else:
            refuse_other_rates(files)
            rates = [SAMPLE_RATE] * len(files)
        names = [os.path.basename(f) for f in files]
        shapes = [wav_shape(f) for f in files] if args.pool else None

        def load(i):
            return read_wav(files[i])[0]

        def read(i):
            return read_wav_channels(files[i])[0]

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
    if args.pool:
        frames = run_pooled(model, args, names, rates, shapes, read, seed)
    else:
        for i, name in enumerate(names):
            y = load(i).cuda()
            x_hat, sr_out, n_frames = enhance_recording(
                model, y, rates[i], args.output_rate, batch=args.batch, **_solver_kw(args),
                noise_key=utterance_key(name) if keyed else None, noise_seed=seed if keyed else 0,
                hop_frames=args.hop_frames, fade_frames=args.fade_frames)
            _write_wav(os.path.join(args.output, name), x_hat, sr_out)
            frames += n_frames
    write_settings(args.output, args, model, epoch, seed,
                   [(n, sr) for n, sr in zip(names, rates) if sr != SAMPLE_RATE])
    print(f"enhanced {len(names)} recordings ({frames} frames) in {time.time() - t0:.2f} s -> {args.output}"
          + (f", keyed noise seed {seed}" if keyed else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
