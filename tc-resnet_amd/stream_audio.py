"""Streaming keyword detection over long WAV files with a frozen artifact (TC-ResNet, DS-CNN or 2-D graph; deploy.FrozenModel, include_preprocess):

    python stream_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] [--frames_per_step k] [--labels l0,l1,...]
                           [--average_window_ms MS] [--detection_threshold P] [--suppression_ms MS] [--min_count N]
                           [--phrases "w1 w2;w3 w4" | @FILE [--phrase_window_ms MS] [--phrase_unordered] [--phrase_combine product|min]]
                           [--second_frozen MODEL2.npz --enter_threshold P [--cascade_pad_ms MS] [--second_frames_per_step K]]

Each file is one stream of a `streaming.StreamingDetector`.  The recordings are scan_audio.py's (`audio_input.Recordings`: 16-bit
PCM, whole on the device; a file at another sample rate than the model's is converted there, `resampling.Resampler`, and noted on
stderr); they are fed in lockstep, one `push` of k * hop samples per step, and a file that has ended is fed zeros until every file
is done.  Samples that do not fill a whole step are dropped (noted on stderr).  One line per detection on stdout:
file,time_ms,label,score  -- time_ms is the end of the window that fired (every stream starts as if it had heard one clip of
silence).  With --phrases "go left;stop no" (or @FILE, one phrase per line; words are --labels names or class indices) every step's
output goes on through a `scanning.StreamingPhraseDetector` and the lines are its detections -- label is the phrase, score its
posterior -- exactly those scan_audio.py --phrases prints for the same files and flags.  A streaming cascade (--second_frozen
MODEL2.npz and --enter_threshold P; `streaming.StreamingCascade`): --frozen steps every stream, and MODEL2's network runs only on the
streams where one of --frozen's keyword classes (every class from 2 on) reaches P at this step or did within --cascade_pad_ms of audio
before it (default: --average_window_ms minus one step); the other streams' posteriors are --frozen's, and the detector flags
configure the final detector, which is MODEL2's.  The two models' steps must be equal (k1 * hop1 == k2 * hop2).  Up to each
file's own end the lines are those of scan_audio.py --ragged with the same cascade flags and --cascade_pad_before_ms 0, byte for byte
(past it a file is fed zeros here, as without a cascade, and a ragged scan has no steps); --phrases composes with it."""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.audio_input import (Recordings, add_detector_flags, cascade_argv, detector_settings, format_time_ms, label_names,
                                          open_phrases, open_streaming_cascade, print_detections)
    from tcresnet_amd.deploy import FrozenModel
else:
    from .audio_input import (Recordings, add_detector_flags, cascade_argv, detector_settings, format_time_ms, label_names, open_phrases,
                              open_streaming_cascade, print_detections)
    from .deploy import FrozenModel
# (format_time_ms is not used here: it stays importable from this module, where it was first defined)


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_detector_flags(p, each="stream", offline=False, phrases=True)
    return p.parse_args(cascade_argv(arguments))


def main(args) -> int:
    import torch
    cascade = open_streaming_cascade(args, len(args.wav))
    det = cascade.second if cascade is not None else FrozenModel.load(args.frozen).streaming(len(args.wav), **detector_settings(args))
    push = det.push if cascade is None else cascade.push
    rec = Recordings(args.wav, det)
    names, step = label_names(args, det), det.step_samples
    phrases = open_phrases(args, det)
    live = None if phrases is None else phrases.streaming(len(args.wav))
    if phrases is not None:
        names = phrases.labels
    buf = torch.zeros((len(args.wav), step), dtype=torch.float32, device=det.device)
    for _, audio in rec.chunks():                   # the whole recordings, once
        for i in range(rec.n_steps):
            buf.copy_(audio[:, i * step:(i + 1) * step])
            out = push(buf)
            print_detections(rec, out if live is None else live.push(out), i, names, {})
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
