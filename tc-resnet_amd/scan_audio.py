"""Offline keyword scanning of long WAV files with a frozen artifact (TC-ResNet, DS-CNN or 2-D graph; deploy.FrozenModel, include_preprocess):

    python scan_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] [--frames_per_step k] [--labels l0,l1,...]
                         [--average_window_ms MS] [--detection_threshold P] [--suppression_ms MS] [--min_count N]
                         [--max_windows B] [--summary] [--chunk_seconds X | --ragged | --ragged_chunk_seconds X]
                         [--second_frozen MODEL2.npz --enter_threshold P [--cascade_pad_ms MS] [--cascade_pad_before_ms MS] [--second_frames_per_step K]]
                         [--phrases "w1 w2;w3 w4" | @FILE [--phrase_window_ms MS] [--phrase_unordered] [--phrase_combine product|min]]
                         [--templates TEMPLATES.npz [--template_max_stretch X]]

The files (16-bit PCM) come from `audio_input.Recordings`, zero-padded to the longest, and are scanned in one
`scanning.KeywordScanner` call; samples that do not fill a whole step are dropped (noted on stderr).  A file at another sample rate
than the model's (its `fmt ` chunk) is converted on the device (`resampling.Resampler`: the int16 PCM is uploaded, one stderr line
a.wav: 48000 Hz -> 16000 Hz), its length is the converted signal's, and time_ms is real time; files at the model's rate are decoded
on the host.  With --chunk_seconds, the files are read X seconds at a time (rounded down to whole steps) and fed to one
`streaming.StreamingDetector` by `push_many`, so host memory holds one chunk per file; a file that has ended reads as zeros until the
longest ends, and the output is the one-call output, byte for byte.  The output is stream_audio.py's, line for line: one line per
detection on stdout,  file,time_ms,label,score,  in step order and, within a step, in file order -- time_ms is the end of the
window that fired (every file starts as if it had heard one clip of silence).  --summary adds one JSON line on stderr: the hours
of audio scanned (each file's whole steps), the detections per label and the detections per hour.  With --ragged (not together with
--chunk_seconds) every file is scanned at its own whole-step length in one `KeywordScanner.scan_ragged` call: nothing is padded, the
lines have the same format and order, and no file has steps (or detections) past its own end.  --ragged_chunk_seconds X (on its own:
not with --chunk_seconds or --ragged) is that run in bounded host memory: every file is read X seconds at a time at its own length --
its next whole steps, none once it has ended -- and the chunks go to one `StreamingDetector.push_ragged`; stdout and the --summary
line are those of --ragged, byte for byte.  A cascade (--ragged with --second_frozen MODEL2.npz and --enter_threshold P): --frozen scans
every step, the steps where one of its keyword classes (every class from 2 on) reaches P, and --cascade_pad_ms of audio on both sides
of them (default: the averaging window minus one step; --cascade_pad_before_ms MS: another amount in front of them, 0 being the
causal cascade stream_audio.py computes on live streams), are computed again by MODEL2 at --second_frames_per_step, and the detector
-- the detector flags are the second stage's -- runs on the merged posteriors (`scanning.CascadeScanner`); both models must have the
same sample rate, classes and step (frames per step x hop).  --summary then gains selected_steps and total_steps.  With
--enter_threshold -inf every step is MODEL2's and stdout is MODEL2's own --ragged run, byte for byte.  With --phrases "go left;stop no"
(or @FILE, one phrase per line; words are --labels names or class indices) the lines and the summary are those of a
`scanning.PhraseDetector` over the scan: label is the phrase, score its posterior -- the best product (--phrase_combine min: minimum)
of its words' smoothed posteriors within --phrase_window_ms, in the given order unless --phrase_unordered -- with the detector
flags' threshold and suppression; on the one-call run, --ragged and a cascade, not with --chunk_seconds / --ragged_chunk_seconds.
With --templates TEMPLATES.npz (written by enroll_audio.py; not with --phrases) they are those of a `scanning.TemplateDetector` instead:
label is an enrolled keyword, score 1 - the cost of the best match of one of its templates that ends at the step, 0 for a match of
more than --template_max_stretch (default 3) times the longest template's steps; on the same runs as --phrases."""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.audio_input import (Recordings, add_detector_flags, cascade_argv, check_phrase_flags, label_names, open_cascade,
                                          open_detector, open_phrases, print_detections, print_detections_ragged, summary_line)
    from tcresnet_amd.deploy import FrozenModel
else:
    from .audio_input import (Recordings, add_detector_flags, cascade_argv, check_phrase_flags, label_names, open_cascade, open_detector,
                              open_phrases, print_detections, print_detections_ragged, summary_line)
    from .deploy import FrozenModel


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_detector_flags(p, phrases=True)
    p.add_argument("--summary", action="store_true", help="one JSON line of totals on stderr")
    return p.parse_args(cascade_argv(arguments))


def main_cascade(args, cascade) -> int:
    rec = Recordings(args.wav, cascade.second)
    names, counts, extra = label_names(args, cascade.second), {}, {"selected_steps": 0, "total_steps": 0}
    phrases = open_phrases(args, cascade.second)
    if rec.n_steps > 0:
        out = cascade.scan_ragged(rec.packed())
        if phrases is not None:
            out, names = phrases.detect(out), phrases.labels
        print_detections_ragged(rec, out, names, counts)
        extra = {"selected_steps": int(out.selected.numel()), "total_steps": int(out.top.shape[0])}
    if args.summary:
        print(summary_line(rec, counts, extra), file=sys.stderr)
    return 0


def main(args) -> int:
    check_phrase_flags(args)
    cascade = open_cascade(args)
    if cascade is not None:
        return main_cascade(args, cascade)
    det, run = open_detector(FrozenModel.load(args.frozen), args)
    rec = Recordings(args.wav, det)
    names, counts = label_names(args, det), {}
    phrases = open_phrases(args, det)
    if phrases is not None:                             # (the one-call runs only: `open_phrases` refuses the chunked ones)
        if args.ragged:
            if rec.n_steps > 0:
                print_detections_ragged(rec, phrases.detect(det.scan_ragged(rec.packed())), phrases.labels, counts)
        else:
            for i0, samples in rec.chunks(None):
                print_detections(rec, phrases.detect(run(samples)), i0, phrases.labels, counts)
    elif args.ragged_chunk_seconds is not None:
        for i0, packed, lengths in rec.ragged_chunks(args.ragged_chunk_seconds):
            print_detections_ragged(rec, run((packed, lengths)), names, counts, i0)
    elif args.ragged:
        if rec.n_steps > 0:
            print_detections_ragged(rec, det.scan_ragged(rec.packed()), names, counts)
    else:
        for i0, samples in rec.chunks(args.chunk_seconds):
            print_detections(rec, run(samples), i0, names, counts)
    if args.summary:
        print(summary_line(rec, counts), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
