"""Hard examples of a frozen artifact over labelled WAV files, as clips a training run can read: the windows that fired outside any
event, the events never hit, the windows that came close (`KeywordScanner.mine`, tcr_mine_*).

    python mine_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] --out_dir DIR [--events EVENTS.csv] [--top K]
                         [--source detections|peaks] [--kinds false_accept,hit,duplicate,miss] [--floor P] [--radius_ms MS]
                         [--lead_ms MS] [--as_label NAME] [--tolerance_ms MS] [--keywords l0,l1,...] [--detection_threshold T]
                         [--frames_per_step k] [--labels l0,l1,...] [--average_window_ms MS] [--suppression_ms MS] [--min_count N]
                         [--max_windows B]
                         [--second_frozen MODEL2.npz --enter_threshold P [--cascade_pad_ms MS] [--cascade_pad_before_ms MS] [--second_frames_per_step K]]

The model, input, detector and cascade flags are sweep_audio.py's, and so is EVENTS.csv (optional here: without it every detection
is a false accept).  The files are always scanned at their own lengths in one `KeywordScanner.scan_ragged` call (--ragged is implied);
--chunk_seconds and --ragged_chunk_seconds are refused: mining needs the whole scan and the whole audio on the device.
--source detections (the default) takes the scan's detections at --detection_threshold, classified by the sweep's rule, and keeps
the --top K of the --kinds with the highest score ("miss": one clip per event no detection hit, on top of K); --source peaks takes
the K highest local maxima of the keyword posteriors (--keywords; default: every label that does not start with '_') that reach
--floor, within --radius_ms (default: the suppression time), outside every window that overlaps an event.  A clip is the model's
input length and ends --lead_ms after the step's window.

Files: DIR/<label>/<source file stem>_<time_ms>.wav, 16-bit mono at the model's rate -- <label> is --as_label (default _unknown_),
and for misses and hits the event's label -- the layout the dataset loader reads.  stdout: a CSV manifest
path,file,time_ms,label,kind,value,event_start_ms  (label: the detection's or peak's, a miss: the event's; value: empty for a miss).
stderr: one JSON line with the clips written and the counts per kind."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
from typing import List, Optional

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd import sweep_audio
    from tcresnet_amd.audio_input import (Recordings, add_detector_flags, cascade_argv, format_time_ms, label_names, open_cascade, open_detector,
                                          write_wav)
    from tcresnet_amd.deploy import FrozenModel
else:
    from . import sweep_audio
    from .audio_input import Recordings, add_detector_flags, cascade_argv, format_time_ms, label_names, open_cascade, open_detector, write_wav
    from .deploy import FrozenModel

COLUMNS = ("path", "file", "time_ms", "label", "kind", "value", "event_start_ms")
KINDS = ("false_accept", "hit", "duplicate", "miss")
CHUNK_REFUSAL = ("mine_audio.py mines one whole scan and gathers the clips from the whole audio on the device: {flag} is not supported "
                 "(the files are scanned at their own lengths in one call)")


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_detector_flags(p)
    p.add_argument("--out_dir", required=True, help="where the clips are written")
    p.add_argument("--events", default=None, help="CSV of labelled keyword events: file,start_ms,end_ms,label (sweep_audio.py's)")
    p.add_argument("--tolerance_ms", type=float, default=1000.0, help="a detection up to this long after an event's end still hits it")
    p.add_argument("--top", type=int, default=1000, help="K: the clips kept (misses come on top)")
    p.add_argument("--source", default="detections", choices=("detections", "peaks"))
    p.add_argument("--kinds", default="false_accept", help="comma-separated, of " + ",".join(KINDS) + " (--source detections)")
    p.add_argument("--keywords", default=None, help="comma-separated labels mined (default: labels not starting with '_')")
    p.add_argument("--floor", type=float, default=0.0, help="--source peaks: the lowest posterior that counts")
    p.add_argument("--radius_ms", type=float, default=None, help="--source peaks: a peak is the largest within this time on both sides")
    p.add_argument("--lead_ms", type=float, default=0.0, help="the clip ends this long after the step's window")
    p.add_argument("--as_label", default="_unknown_", help="the folder (label) of the clips that are no event's")
    return p.parse_args(cascade_argv(arguments))


def check_arguments(args):
    """The refusals that need no model; --kinds becomes a list."""
    if args.chunk_seconds is not None:
        raise SystemExit(CHUNK_REFUSAL.format(flag="--chunk_seconds"))
    if args.ragged_chunk_seconds is not None:
        raise SystemExit(CHUNK_REFUSAL.format(flag="--ragged_chunk_seconds"))
    if args.top < 0:
        raise SystemExit(f"--top must be >= 0 (got {args.top})")
    kinds = [x for x in str(args.kinds).split(",") if x]
    bad = [x for x in kinds if x not in KINDS]
    if bad:
        raise SystemExit(f"--kinds: unknown kind {bad} (known: {','.join(KINDS)})")
    if args.source == "peaks" and kinds != ["false_accept"]:
        raise SystemExit("--kinds belongs to --source detections (peaks have no kind)")
    args.kinds, args.ragged = kinds, True
    return args


def main(args) -> int:
    args = check_arguments(args)
    cascade = open_cascade(args)
    scanner = cascade.second if cascade is not None else open_detector(FrozenModel.load(args.frozen), args)[0]
    names = label_names(args, scanner)
    keywords = args.keywords.split(",") if args.keywords else [x for x in names if not x.startswith("_")]
    unknown = [k for k in keywords if k not in names]
    if unknown:
        raise SystemExit(f"--keywords {unknown} are not labels")
    rec = Recordings(args.wav, scanner)
    if rec.n_steps == 0:
        raise SystemExit("no whole step of audio in the files")
    events = sweep_audio.read_events(args.events, args.wav) if args.events else None
    signals = rec.packed()
    out = (cascade or scanner).scan_ragged(signals)
    classes = [names.index(k) for k in keywords] if (args.keywords or args.source == "peaks") else None
    mined = scanner.mine(out, signals, events, k=args.top, source=args.source, kinds=args.kinds, classes=classes, floor=args.floor,
                         radius_ms=args.radius_ms, tolerance_ms=args.tolerance_ms, labels=names, lead_ms=args.lead_ms, pcm=True)
    pcm = mined.pcm.cpu().numpy()
    w = csv.writer(sys.stdout, lineterminator="\n")
    w.writerow(COLUMNS)
    counts = {}
    for i, kind in enumerate(mined.kind_names()):
        label = names[int(mined.label[i])]
        folder = label if kind in ("miss", "hit") else args.as_label
        src = args.wav[int(mined.signal[i])]
        os.makedirs(os.path.join(args.out_dir, folder), exist_ok=True)
        path = os.path.join(args.out_dir, folder, f"{os.path.splitext(os.path.basename(src))[0]}_{format_time_ms(float(mined.time_ms[i]))}.wav")
        write_wav(path, pcm[i], rec.rate)
        counts[kind] = counts.get(kind, 0) + 1
        start = mined.event_start_ms[i]
        w.writerow([path, src, format_time_ms(float(mined.time_ms[i])), label, kind, "" if kind == "miss" else f"{float(mined.value[i]):.6f}",
                    "" if start != start else format_time_ms(float(start))])
    sys.stdout.flush()
    print(json.dumps({"clips": len(mined), "kinds": counts, "source": args.source, "out_dir": args.out_dir}), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
