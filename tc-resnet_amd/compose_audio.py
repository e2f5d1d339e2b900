"""Labelled test recordings from a dataset directory: the split's clips pasted at known times onto its looping background noise, on
the device (`composing.Composer`, tcr_compose), written as WAV files with the events a sweep scores against.

    python compose_audio.py --dataset_path D --dataset_split_name valid --output_dir OUT --num_recordings N --seconds S
                            [--frames_per_step k] [--window_stride_ms MS] [--sample_rate HZ] | [--step_samples M]
                            [--min_gap_ms MS] [--max_gap_ms MS] [--keywords l0,l1,...] [--foreground_gain G] [--background_volume V]
                            [--snr_db X | LO:HI] [--seed SEED] [--prefix NAME]
                            [--rir_dir DIR | --rir_rt60 X | LO:HI [--rir_count N]] [--rir_probability P] [--rir_tail_ms MS] [--rir_seed S]

D/<split>/<label>/*.wav and D/<split>/_background_noise_/*.wav are read as training reads them (`SingleLabelAudioDataWrapper`: every
clip decoded once into an int16 pool on the device).  Every recording is --seconds long, rounded down to whole steps of
--frames_per_step x --window_stride_ms (or --step_samples), the scanner's k x hop, so sweep_audio.py drops nothing.  The draws are
`Composer.plan`'s, from one generator seeded with --seed: per recording a background recording and its phase, then clip, gap, clip,
gap .. with gaps of --min_gap_ms .. --max_gap_ms, clips from the --keywords (default: every label), each at --foreground_gain or at
--snr_db over the background (a number, or LO:HI drawn per clip).  --min_gap_ms has to exceed the --tolerance_ms of the sweep.

Reverberation (`Composer.reverberated`, tcr_reverb): with --rir_dir (every *.wav of DIR is a room impulse response, sorted by name,
resampled to --sample_rate where needed) or --rir_rt60 (--rir_count synthetic responses, default 16, RT60 in seconds: a number, or
LO:HI drawn per response) every clip is convolved on the device with a response drawn from the bank, or left dry at probability
1 - --rir_probability; --rir_tail_ms caps the tail a wet clip -- and with it its event -- is lengthened by (default: the whole
response); --rir_seed seeds the bank and the draws.  --snr_db then counts the wet clips' power.

Files: OUT/<prefix>_<n>.wav (16-bit mono) and OUT/events.csv (file,start_ms,end_ms,label with label names), directly usable as
    python sweep_audio.py --frozen M --wav OUT/*.wav --events OUT/events.csv --ragged --labels <the dataset's label names>
stdout: one line per written file.  stderr: one JSON line with the recordings, the seconds of audio and the events per label."""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace
from typing import List, Optional

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.composing import Composer
    from tcresnet_amd.reverberation import ImpulseResponses
    from tcresnet_amd.datasets.audio_data_wrapper import SingleLabelAudioDataWrapper
else:
    from .composing import Composer
    from .reverberation import ImpulseResponses
    from .datasets.audio_data_wrapper import SingleLabelAudioDataWrapper


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--dataset_path", required=True, help="the dataset's root: <split>/<label>/*.wav")
    p.add_argument("--dataset_split_name", default="valid")
    p.add_argument("--output_dir", required=True, help="where the recordings and events.csv are written")
    p.add_argument("--num_recordings", type=int, required=True)
    p.add_argument("--seconds", type=float, required=True, help="the length of every recording")
    p.add_argument("--sample_rate", type=int, default=16000)
    p.add_argument("--frames_per_step", type=int, default=1, help="the scanner's new front-end frames per step (k)")
    p.add_argument("--window_stride_ms", type=float, default=20.0, help="the front-end's hop")
    p.add_argument("--step_samples", type=int, default=None, help="k x hop in samples, instead of the two flags above")
    p.add_argument("--min_gap_ms", type=float, default=1500.0, help="the shortest gap after a clip (above the sweep's --tolerance_ms)")
    p.add_argument("--max_gap_ms", type=float, default=4000.0)
    p.add_argument("--keywords", default=None, help="comma-separated labels to draw clips from (default: every label)")
    p.add_argument("--foreground_gain", type=float, default=1.0)
    p.add_argument("--background_volume", type=float, default=0.1)
    p.add_argument("--snr_db", default=None, help="X or LO:HI: the clips' gain from their power over the background's")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--prefix", default="rec", help="the files are <prefix>_<n>.wav")
    p.add_argument("--rir_dir", default=None, help="a directory of room impulse responses (*.wav): the clips are reverberated")
    p.add_argument("--rir_rt60", default=None, help="X or LO:HI seconds: synthetic impulse responses instead of --rir_dir")
    p.add_argument("--rir_count", type=int, default=None, help="the number of synthetic responses (default 16; with --rir_rt60)")
    p.add_argument("--rir_probability", type=float, default=None, help="the share of clips that get a response (default 1)")
    p.add_argument("--rir_tail_ms", type=float, default=None, help="the longest tail a clip is lengthened by (default: the response's)")
    p.add_argument("--rir_seed", type=int, default=None, help="seeds the synthetic bank and the draws per clip (default 0)")
    return p.parse_args(arguments)


def check_arguments(args):
    """The refusals that need no dataset; --snr_db becomes None, a number or (lo, hi), --step_samples is resolved."""
    if args.num_recordings < 1:
        raise SystemExit(f"--num_recordings must be >= 1 (got {args.num_recordings})")
    if not args.seconds >= 0:
        raise SystemExit(f"--seconds must be >= 0 (got {args.seconds})")
    if not args.min_gap_ms > 0 or args.max_gap_ms < args.min_gap_ms:
        raise SystemExit(f"--min_gap_ms {args.min_gap_ms:g} and --max_gap_ms {args.max_gap_ms:g}: 0 < min <= max")
    if args.step_samples is None:
        args.step_samples = args.frames_per_step * int(args.sample_rate * args.window_stride_ms / 1000)
    if args.step_samples < 1:
        raise SystemExit(f"a step of {args.step_samples} samples: --frames_per_step, --window_stride_ms or --step_samples must be positive")
    if args.snr_db is not None:
        try:
            parts = [float(x) for x in str(args.snr_db).split(":")]
        except ValueError:
            parts = []
        if len(parts) not in (1, 2) or (len(parts) == 2 and parts[1] < parts[0]):
            raise SystemExit(f"--snr_db {args.snr_db}: expected X or LO:HI with HI >= LO")
        args.snr_db = parts[0] if len(parts) == 1 else (parts[0], parts[1])
    if args.rir_dir is not None and args.rir_rt60 is not None:
        raise SystemExit("--rir_dir and --rir_rt60 exclude each other: measured responses or synthetic ones")
    if args.rir_dir is None and args.rir_rt60 is None:
        for flag in ("rir_count", "rir_probability", "rir_tail_ms", "rir_seed"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} needs --rir_dir or --rir_rt60: there is nothing to reverberate with")
    if args.rir_count is not None and args.rir_rt60 is None:
        raise SystemExit("--rir_count counts synthetic responses: it needs --rir_rt60 (--rir_dir takes every file)")
    if args.rir_count is not None and args.rir_count < 1:
        raise SystemExit(f"--rir_count must be >= 1 (got {args.rir_count})")
    if args.rir_probability is not None and not 0.0 <= args.rir_probability <= 1.0:
        raise SystemExit(f"--rir_probability must be in [0, 1] (got {args.rir_probability})")
    if args.rir_tail_ms is not None and not args.rir_tail_ms >= 0:
        raise SystemExit(f"--rir_tail_ms must be >= 0 (got {args.rir_tail_ms})")
    if args.rir_rt60 is not None:
        try:
            parts = [float(x) for x in str(args.rir_rt60).split(":")]
        except ValueError:
            parts = []
        if len(parts) not in (1, 2) or not parts[0] > 0 or (len(parts) == 2 and parts[1] < parts[0]):
            raise SystemExit(f"--rir_rt60 {args.rir_rt60}: expected X or LO:HI seconds with 0 < LO <= HI")
        args.rir_rt60 = parts[0] if len(parts) == 1 else (parts[0], parts[1])
    return args


def open_responses(args, device):
    """The bank --rir_dir or --rir_rt60 asks for on `device`, or None."""
    if args.rir_dir is None and args.rir_rt60 is None:
        return None
    seed = args.rir_seed or 0
    if args.rir_dir is not None:
        if not os.path.isdir(args.rir_dir):
            raise SystemExit(f"--rir_dir {args.rir_dir}: no such directory")
        paths = sorted(os.path.join(args.rir_dir, f) for f in os.listdir(args.rir_dir) if f.lower().endswith(".wav"))
        if not paths:
            raise SystemExit(f"--rir_dir {args.rir_dir}: no *.wav files")
        return ImpulseResponses.from_files(paths, args.sample_rate, device=device)
    return ImpulseResponses.synthetic(args.rir_count or 16, args.rir_rt60, args.sample_rate, seed=seed, device=device)


def open_dataset(args) -> SingleLabelAudioDataWrapper:
    """The split as training opens it, without silent samples; the class count is the split's own."""
    root = os.path.join(args.dataset_path, args.dataset_split_name)
    if not os.path.isdir(root):
        raise SystemExit(f"{root}: no such dataset split directory")
    labels = [d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)) and not d.startswith("_")]
    cfg = SimpleNamespace(dataset_path=args.dataset_path, batch_size=1, shuffle=False, add_null_class=True, num_classes=len(labels) + 1,
                          num_silent=0, sample_rate=args.sample_rate, clip_duration_ms=1000, augmentation_method="no_augmentation_audio",
                          seed=args.seed)
    return SingleLabelAudioDataWrapper(cfg, dataset_split_name=args.dataset_split_name, is_training=False)


def main(args) -> int:
    args = check_arguments(args)
    composer = Composer.from_dataset(open_dataset(args))
    irs = open_responses(args, composer.device)
    if irs is not None:
        composer = composer.reverberated(irs, 1.0 if args.rir_probability is None else args.rir_probability, args.rir_tail_ms, args.rir_seed or 0)
    names = composer.label_names
    classes = None
    if args.keywords:
        keywords = args.keywords.split(",")
        unknown = [k for k in keywords if k not in names]
        if unknown:
            raise SystemExit(f"--keywords {unknown} are not labels of the split ({names})")
        classes = [names.index(k) for k in keywords]
    plan = composer.plan(args.num_recordings, args.seconds, args.step_samples, min_gap_ms=args.min_gap_ms, max_gap_ms=args.max_gap_ms,
                         classes=classes, foreground_gain=args.foreground_gain, background_volume=args.background_volume,
                         snr_db=args.snr_db, seed=args.seed)
    rec = composer.compose(plan, floats=False, pcm=True)
    paths = rec.write_wavs(args.output_dir, args.prefix)
    for path in paths + [os.path.join(args.output_dir, "events.csv")]:
        print(path)
    sys.stdout.flush()
    counts = {}
    for evs in rec.events:
        for _, _, label in evs:
            counts[names[label]] = counts.get(names[label], 0) + 1
    info = {"recordings": len(paths), "seconds": float(plan.total_samples) / plan.sample_rate, "events": counts, "output_dir": args.output_dir}
    if irs is not None:
        info.update(responses=len(irs), wet_clips=int((composer.ir_index >= 0).sum()))
    print(json.dumps(info), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
