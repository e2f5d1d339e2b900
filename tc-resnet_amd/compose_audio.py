"""Labelled test recordings from a dataset directory: the split's clips pasted at known times onto its looping background noise, on
the device (`composing.Composer`, tcr_compose), written as WAV files with the events a sweep scores against.

    python compose_audio.py --dataset_path D --dataset_split_name valid --output_dir OUT --num_recordings N --seconds S
                            [--frames_per_step k] [--window_stride_ms MS] [--sample_rate HZ] | [--step_samples M]
                            [--min_gap_ms MS] [--max_gap_ms MS] [--keywords l0,l1,...] [--foreground_gain G] [--background_volume V]
                            [--snr_db X | LO:HI] [--seed SEED] [--prefix NAME]

D/<split>/<label>/*.wav and D/<split>/_background_noise_/*.wav are read as training reads them (`SingleLabelAudioDataWrapper`: every
clip decoded once into an int16 pool on the device).  Every recording is --seconds long, rounded down to whole steps of
--frames_per_step x --window_stride_ms (or --step_samples), the scanner's k x hop, so sweep_audio.py drops nothing.  The draws are
`Composer.plan`'s, from one generator seeded with --seed: per recording a background recording and its phase, then clip, gap, clip,
gap .. with gaps of --min_gap_ms .. --max_gap_ms, clips from the --keywords (default: every label), each at --foreground_gain or at
--snr_db over the background (a number, or LO:HI drawn per clip).  --min_gap_ms has to exceed the --tolerance_ms of the sweep.

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
    from tcresnet_amd.datasets.audio_data_wrapper import SingleLabelAudioDataWrapper
else:
    from .composing import Composer
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
    return args


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
    print(json.dumps({"recordings": len(paths), "seconds": float(plan.total_samples) / plan.sample_rate, "events": counts,
                      "output_dir": args.output_dir}), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
