"""Detector tuning of a frozen artifact over labelled WAV files: the averaging window, min_count, the suppression time and the
threshold from ONE scan (`KeywordScanner.tune`, tcr_detect_grid).

    python tune_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] --events EVENTS.csv
                         [--average_window_ms W0,W1,...] [--min_count M0,M1,...] [--suppression_ms S0,S1,...]
                         [--thresholds LO:HI:STEP | t0,t1,...] [--tolerance_ms MS] [--keywords l0,l1,...] [--per_label]
                         [--target_fa_per_hour F] [--frames_per_step k] [--labels l0,l1,...] [--max_windows B] [--ragged]

The flags, the files and EVENTS.csv are sweep_audio.py's; the three detector flags take comma lists, and their Cartesian grid (in
the order window, min_count, suppression) is evaluated at every threshold from the probabilities of one scan -- the front-end and
the network run once.  Combinations with min_count above the window's steps are dropped.  --ragged scans the files at their own
lengths.  --chunk_seconds and --ragged_chunk_seconds are refused: the grid needs the whole scan's probabilities on the device.

stdout: sweep_audio.py's CSV with the leading columns average_window_ms,min_count,suppression_ms (--per_label: then its label
column), the points in grid order; for a grid of one point the columns behind them are sweep_audio.py's rows for those detector
flags, byte for byte.  stderr: one JSON line: the hours scanned, the points dropped and `best`, the point and threshold of the lowest
FRR with fa_per_hour <= --target_fa_per_hour (null when none is)."""
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
    from tcresnet_amd.audio_input import Recordings, label_names, open_detector
    from tcresnet_amd.deploy import FrozenModel
else:
    from . import sweep_audio
    from .audio_input import Recordings, label_names, open_detector
    from .deploy import FrozenModel

GRID_COLUMNS = ("average_window_ms", "min_count", "suppression_ms")
CHUNK_REFUSAL = ("tune_audio.py tunes the detector from one whole scan's probabilities: --chunk_seconds and --ragged_chunk_seconds are "
                 "not supported (use the one-call run or --ragged)")


def _floats(spec: str) -> List[float]:
    return [float(x) for x in str(spec).split(",")]


def parse_arguments(arguments: Optional[List[str]] = None):
    """sweep_audio.py's arguments; the three detector flags are comma lists here."""
    argv = list(sys.argv[1:] if arguments is None else arguments)
    lists = {}
    rest, i = [], 0
    while i < len(argv):                # the list flags are taken out before sweep_audio's parser sees its scalar flags
        key = argv[i].split("=", 1)[0]
        if key in ("--average_window_ms", "--min_count", "--suppression_ms"):
            if "=" in argv[i]:
                lists[key[2:]] = argv[i].split("=", 1)[1]
                i += 1
            else:
                if i + 1 >= len(argv):
                    raise SystemExit(f"{key} expects a comma-separated list")
                lists[key[2:]] = argv[i + 1]
                i += 2
        else:
            rest.append(argv[i])
            i += 1
    args = sweep_audio.parse_arguments(rest)
    if args.chunk_seconds is not None or args.ragged_chunk_seconds is not None:
        raise SystemExit(CHUNK_REFUSAL)
    if args.phrases is not None:
        raise SystemExit("--phrases is sweep_audio.py's and scan_audio.py's: this tool tunes the word detector (a phrase detector's grid: "
                         "scanning.PhraseDetector.tune)")
    if args.templates is not None:
        raise SystemExit("--templates is sweep_audio.py's and scan_audio.py's: this tool tunes the word detector (a template detector's "
                         "grid: scanning.TemplateDetector.tune)")
    try:
        args.grid_window_ms = _floats(lists.get("average_window_ms", args.average_window_ms))
        args.grid_min_count = [int(x) for x in str(lists.get("min_count", args.min_count)).split(",")]
        args.grid_suppression_ms = _floats(lists.get("suppression_ms", args.suppression_ms))
    except ValueError as e:
        raise SystemExit(f"--average_window_ms, --min_count and --suppression_ms take comma-separated numbers: {e}")
    # the scanner itself is built with the grid's first values (its own settings only matter to the scan's unused detector tail)
    args.average_window_ms, args.suppression_ms = args.grid_window_ms[0], args.grid_suppression_ms[0]
    args.min_count = 1
    return args


def main(args) -> int:
    scanner, run = open_detector(FrozenModel.load(args.frozen), args)
    names = label_names(args, scanner)
    keywords = args.keywords.split(",") if args.keywords else [x for x in names if not x.startswith("_")]
    unknown = [k for k in keywords if k not in names]
    if unknown:
        raise SystemExit(f"--keywords {unknown} are not labels")
    classes = [names.index(k) for k in keywords]
    thresholds = sweep_audio.parse_thresholds(args.thresholds)
    rec = Recordings(args.wav, scanner)
    if rec.n_steps == 0:
        raise SystemExit("no whole step of audio in the files")
    events = sweep_audio.read_events(args.events, args.wav)
    grid = dict(average_window_ms=args.grid_window_ms, min_count=args.grid_min_count, suppression_ms=args.grid_suppression_ms,
                events=events, tolerance_ms=args.tolerance_ms, labels=names)
    if args.ragged:
        res = scanner.tune(scanner.scan_ragged(rec.packed()), thresholds, **grid)
    else:
        outs = [run(samples) for _, samples in rec.chunks(None)]
        res = scanner.tune(outs[0], thresholds, lengths=rec.lengths, **grid)
    w = csv.writer(sys.stdout, lineterminator="\n")
    w.writerow(GRID_COLUMNS + (("label",) if args.per_label else ()) + sweep_audio.COLUMNS)
    for j, pt in enumerate(res.points):
        lead = [f"{pt.average_window_ms:g}", pt.min_count, f"{pt.suppression_ms:g}"]
        r = res.result(j)
        if args.per_label:
            for k, c in zip(keywords, classes):
                cv = r.curve([c])
                for t in range(len(thresholds)):
                    w.writerow(lead + [k] + sweep_audio.format_row(cv, t))
        else:
            cv = r.curve(classes)
            for t in range(len(thresholds)):
                w.writerow(lead + sweep_audio.format_row(cv, t))
    sys.stdout.flush()
    best = res.best(args.target_fa_per_hour, classes)
    if best is not None:
        pt = best.pop("point")
        best = {"average_window_ms": pt.average_window_ms, "min_count": pt.min_count, "suppression_ms": pt.suppression_ms, **best}
    print(json.dumps({"hours": float(res.hours.sum()), "keywords": keywords, "target_fa_per_hour": args.target_fa_per_hour,
                      "dropped": [[p.average_window_ms, p.min_count, p.suppression_ms] for p in res.dropped], "best": best}),
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
