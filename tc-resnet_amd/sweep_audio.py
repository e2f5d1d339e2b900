"""Detection-threshold sweep of a frozen artifact (TC-ResNet, DS-CNN or 2-D graph; deploy.FrozenModel, include_preprocess) over labelled WAV files: a DET
curve (false rejects against false accepts per hour) from one scan.

    python sweep_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] --events EVENTS.csv [--thresholds LO:HI:STEP | t0,t1,...]
                          [--tolerance_ms MS] [--keywords l0,l1,...] [--per_label] [--target_fa_per_hour F]
                          [--frames_per_step k] [--labels l0,l1,...] [--average_window_ms MS] [--suppression_ms MS]
                          [--min_count N] [--max_windows B] [--chunk_seconds X | --ragged | --ragged_chunk_seconds X]
                          [--second_frozen MODEL2.npz --enter_threshold P [--cascade_pad_ms MS] [--cascade_pad_before_ms MS] [--second_frames_per_step K]]
                          [--phrases "w1 w2;w3 w4" | @FILE [--phrase_window_ms MS] [--phrase_unordered] [--phrase_combine product|min]]
                          [--templates TEMPLATES.npz [--template_max_stretch X]]

The files are read as scan_audio.py reads them (`audio_input.Recordings`: 16-bit PCM, converted to the model's sample rate on the
device where it differs, only whole steps), zero-padded to the longest and scanned in one call; one `KeywordScanner.sweep` then
walks the detector's suppression rule at every threshold over each file's true length (--detection_threshold is not an input: the
thresholds are).  With --chunk_seconds the files are read and scanned chunk by chunk (scan_audio.py's --chunk_seconds:
`StreamingDetector.push_many`); either way the chunks' top / score are concatenated on the device and swept once: the output is the
one-call output, byte for byte.  With --ragged (not together with --chunk_seconds) the files are scanned at their own lengths in
one `KeywordScanner.scan_ragged` call and swept over its packed rows: the same curve without the padding; --ragged_chunk_seconds X
(on its own) reads the files X seconds at a time at their own lengths (`StreamingDetector.push_ragged`), keeps every file's top /
score rows on the device, puts them back into the packed layout and sweeps once: --ragged's output, byte for byte.  A cascade
(--ragged with --second_frozen and --enter_threshold, scan_audio.py's flags: `scanning.CascadeScanner`) sweeps the second stage's
detector over the merged posteriors; the JSON line then gains selected_steps and total_steps.  EVENTS.csv has a header and the columns
file,start_ms,end_ms,label  (file as given to --wav, label one of --labels or a class index).  A detection at time t (the end of
the window that fired, scan_audio.py's time) hits an event of its label when  start_ms <= t <= end_ms + tolerance_ms; the first
hit of an event counts as a hit, later ones as duplicates, every other detection as a false accept.

stdout: CSV with a header, one row per threshold over the --keywords (default: every label that does not start with '_'):
threshold,hits,events,false_accepts,duplicates,frr,fa_per_hour  (frr = 1 - hits / events); --per_label: one row per keyword and
threshold, with a leading label column.  stderr: one JSON line, the hours scanned and the operating point: the threshold of the
lowest FRR with fa_per_hour <= --target_fa_per_hour (null when none is).

With --phrases (scan_audio.py's flags: `scanning.PhraseDetector`) the curve is the phrase detector's over the scan: the events' labels
and the --keywords are phrase names (the words joined by a space; default: every phrase, never _background_), on the one-call run,
--ragged and a cascade; not with --chunk_seconds / --ragged_chunk_seconds.  With --templates (scan_audio.py's flags:
`scanning.TemplateDetector` over an enroll_audio.py file; not with --phrases) it is the template detector's: the events' labels and the
--keywords are the enrolled keywords' names, on the same runs."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
from typing import List, Optional

import numpy as np

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.audio_input import (Recordings, add_detector_flags, cascade_argv, check_phrase_flags, label_names, open_cascade,
                                          open_detector, open_phrases)
    from tcresnet_amd.deploy import FrozenModel
    from tcresnet_amd.scanning import RaggedScanOutput, ScanOutput
else:
    from .audio_input import (Recordings, add_detector_flags, cascade_argv, check_phrase_flags, label_names, open_cascade, open_detector,
                              open_phrases)
    from .deploy import FrozenModel
    from .scanning import RaggedScanOutput, ScanOutput

COLUMNS = ("threshold", "hits", "events", "false_accepts", "duplicates", "frr", "fa_per_hour")


def parse_thresholds(spec: str) -> np.ndarray:
    """LO:HI:STEP (LO, LO + STEP, ... up to HI inclusive) or a comma list."""
    if ":" in spec:
        lo, hi, step = (float(x) for x in spec.split(":"))
        if not step > 0 or hi < lo:
            raise ValueError(f"--thresholds {spec}: expected LO:HI:STEP with STEP > 0 and HI >= LO")
        return np.arange(lo, hi + step * 1e-6, step)
    return np.array([float(x) for x in spec.split(",")])


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_detector_flags(p, threshold=False, phrases=True)
    p.add_argument("--events", required=True, help="CSV of labelled keyword events: file,start_ms,end_ms,label")
    p.add_argument("--thresholds", default="0:0.99:0.01", help="LO:HI:STEP or a comma-separated list")
    p.add_argument("--tolerance_ms", type=float, default=1000.0, help="a detection up to this long after an event's end still hits it")
    p.add_argument("--keywords", default=None, help="comma-separated labels scored (default: labels not starting with '_')")
    p.add_argument("--per_label", action="store_true", help="one row per keyword and threshold")
    p.add_argument("--target_fa_per_hour", type=float, default=0.5, help="false-accept budget of the operating point")
    return p.parse_args(cascade_argv(arguments))


def format_row(cv, t: int) -> list:
    """Row t of a `SweepResult.curve` as the CSV's fields (COLUMNS)."""
    return [f"{cv['threshold'][t]:.6g}", *(int(cv[k][t]) for k in COLUMNS[1:5]), f"{cv['frr'][t]:.6g}", f"{cv['fa_per_hour'][t]:.9g}"]


def read_events(path: str, wavs: List[str]):
    out = [[] for _ in wavs]
    index = {w: n for n, w in enumerate(wavs)}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            f = row["file"]
            if f not in index:
                raise SystemExit(f"{path}: event of {f!r}, which is not one of --wav")
            lab = row["label"].strip()
            out[index[f]].append((float(row["start_ms"]), float(row["end_ms"]), lab))
    return out


def main(args) -> int:
    import torch
    check_phrase_flags(args)
    cascade, extra = open_cascade(args), {}
    if cascade is not None:
        scanner, run = cascade.second, None
    else:
        scanner, run = open_detector(FrozenModel.load(args.frozen), args)
    phrases = open_phrases(args, scanner)
    names = label_names(args, scanner) if phrases is None else phrases.labels
    keywords = args.keywords.split(",") if args.keywords else [x for x in names if not x.startswith("_")]
    unknown = [k for k in keywords if k not in names]
    if unknown:
        raise SystemExit(f"--keywords {unknown} are not labels")
    classes = [names.index(k) for k in keywords]
    thresholds = parse_thresholds(args.thresholds)
    rec = Recordings(args.wav, scanner)
    if rec.n_steps == 0:
        raise SystemExit("no whole step of audio in the files")
    events = read_events(args.events, args.wav)
    if phrases is not None:                             # (the one-call runs only: `open_phrases` refuses the chunked ones)
        if cascade is not None:
            out = cascade.scan_ragged(rec.packed())
            extra = {"selected_steps": int(out.selected.numel()), "total_steps": int(out.top.shape[0])}
            res = phrases.sweep(out, thresholds, events=events, tolerance_ms=args.tolerance_ms)
        elif args.ragged:
            res = phrases.sweep(scanner.scan_ragged(rec.packed()), thresholds, events=events, tolerance_ms=args.tolerance_ms)
        else:
            _, samples = next(iter(rec.chunks(None)))
            res = phrases.sweep(run(samples), thresholds, events=events, lengths=rec.lengths, tolerance_ms=args.tolerance_ms)
    elif cascade is not None:
        out = cascade.scan_ragged(rec.packed())
        extra = {"selected_steps": int(out.selected.numel()), "total_steps": int(out.top.shape[0])}
        res = scanner.sweep(out, thresholds, events=events, tolerance_ms=args.tolerance_ms, labels=names)
    elif args.ragged_chunk_seconds is not None:
        tops, scores = [[] for _ in args.wav], [[] for _ in args.wav]      # per file, its rows chunk by chunk
        for _, packed, lengths in rec.ragged_chunks(args.ragged_chunk_seconds):
            o = run((packed, lengths))
            for n in range(len(args.wav)):
                a, b = int(o.offsets[n]), int(o.offsets[n + 1])
                if b > a:
                    tops[n].append(o.top[a:b])
                    scores[n].append(o.score[a:b])
        offsets = np.concatenate([[0], np.cumsum([x // rec.step for x in rec.lengths])])
        out = RaggedScanOutput(None, None, None, torch.cat([t for f in tops for t in f]), torch.cat([t for f in scores for t in f]), None,
                               offsets)
        res = scanner.sweep(out, thresholds, events=events, tolerance_ms=args.tolerance_ms, labels=names)
    elif args.ragged:
        res = scanner.sweep(scanner.scan_ragged(rec.packed()), thresholds, events=events, tolerance_ms=args.tolerance_ms, labels=names)
    else:
        tops, scores = [], []                           # (only what the sweep reads stays on the device)
        for _, samples in rec.chunks(args.chunk_seconds):
            o = run(samples)
            tops.append(o.top)
            scores.append(o.score)
        out = ScanOutput(None, None, None, torch.cat(tops, dim=1), torch.cat(scores, dim=1), None)
        res = scanner.sweep(out, thresholds, events=events, lengths=rec.lengths, tolerance_ms=args.tolerance_ms, labels=names)
    w = csv.writer(sys.stdout, lineterminator="\n")
    fmt = format_row
    if args.per_label:
        w.writerow(("label",) + COLUMNS)
        for k, c in zip(keywords, classes):
            cv = res.curve([c])
            for t in range(len(thresholds)):
                w.writerow([k] + fmt(cv, t))
    else:
        w.writerow(COLUMNS)
        cv = res.curve(classes)
        for t in range(len(thresholds)):
            w.writerow(fmt(cv, t))
    sys.stdout.flush()
    print(json.dumps({"hours": float(res.hours.sum()), "keywords": keywords, "target_fa_per_hour": args.target_fa_per_hour,
                      "operating_point": res.operating_point(args.target_fa_per_hour, classes), **extra}), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
