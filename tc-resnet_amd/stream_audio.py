"""Streaming keyword detection over long WAV files with a frozen artifact (TC-ResNet, DS-CNN or 2-D graph; deploy.FrozenModel, include_preprocess):

    python stream_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] [--frames_per_step k] [--labels l0,l1,...]
                           [--average_window_ms MS] [--detection_threshold P] [--suppression_ms MS] [--min_count N]
                           [--phrases "w1 w2;w3 w4" | @FILE [--phrase_window_ms MS] [--phrase_unordered] [--phrase_combine product|min]]
                           [--templates TEMPLATES.npz [--template_max_stretch X]]
                           [--second_frozen MODEL2.npz --enter_threshold P [--cascade_pad_ms MS] [--second_frames_per_step K]]
                           [--capture_dir DIR [--capture_lead_ms MS]]

Each file is one stream of a `streaming.StreamingDetector`.  The recordings are scan_audio.py's (`audio_input.Recordings`: 16-bit
PCM, whole on the device; a file at another sample rate than the model's is converted there, `resampling.Resampler`, and noted on
stderr); they are fed in lockstep, one `push` of k * hop samples per step, and a file that has ended is fed zeros until every file
is done.  Samples that do not fill a whole step are dropped (noted on stderr).  One line per detection on stdout:
file,time_ms,label,score  -- time_ms is the end of the window that fired (every stream starts as if it had heard one clip of
silence).  With --phrases "go left;stop no" (or @FILE, one phrase per line; words are --labels names or class indices) every step's
output goes on through a `scanning.StreamingPhraseDetector` and the lines are its detections -- label is the phrase, score its
posterior -- exactly those scan_audio.py --phrases prints for the same files and flags; with --templates TEMPLATES.npz (written by
enroll_audio.py; not with --phrases) through a `scanning.StreamingTemplateDetector`, and the lines are exactly those scan_audio.py
--templates prints: label is an enrolled keyword.  A streaming cascade (--second_frozen
MODEL2.npz and --enter_threshold P; `streaming.StreamingCascade`): --frozen steps every stream, and MODEL2's network runs only on the
streams where one of --frozen's keyword classes (every class from 2 on) reaches P at this step or did within --cascade_pad_ms of audio
before it (default: --average_window_ms minus one step); the other streams' posteriors are --frozen's, and the detector flags
configure the final detector, which is MODEL2's.  The two models' steps must be equal (k1 * hop1 == k2 * hop2).  Up to each
file's own end the lines are those of scan_audio.py --ragged with the same cascade flags and --cascade_pad_before_ms 0, byte for byte
(past it a file is fed zeros here, as without a cascade, and a ragged scan has no steps); --phrases composes with it.
--capture_dir DIR writes the audio behind every printed detection of a keyword class (every class from 2 on; with --phrases every
phrase) to DIR/<label>/<file stem>_<time_ms>.wav, mine_audio.py's layout: the model's clip length ending --capture_lead_ms (default 0)
after the detection's step, 16-bit mono at the model's rate, cut on the device by a `scanning.StreamingRecorder` next to the detector
(what the stream has not been fed by the end reads as zeros).  The lines on stdout do not change."""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.audio_input import (Recordings, add_detector_flags, cascade_argv, detector_settings, format_time_ms, label_names,
                                          open_phrases, open_streaming_cascade, print_detections, write_wav)
    from tcresnet_amd.capturing import StreamingRecorder
    from tcresnet_amd.deploy import FrozenModel
else:
    from .audio_input import (Recordings, add_detector_flags, cascade_argv, detector_settings, format_time_ms, label_names, open_phrases,
                              open_streaming_cascade, print_detections, write_wav)
    from .capturing import StreamingRecorder
    from .deploy import FrozenModel
# (format_time_ms stays importable from this module, where it was first defined)


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_detector_flags(p, each="stream", offline=False, phrases=True)
    p.add_argument("--capture_dir", default=None, help="write the audio behind every detection to DIR/<label>/<file stem>_<time_ms>.wav")
    p.add_argument("--capture_lead_ms", type=float, default=0.0, help="the clips end this long after the detection's step (default 0)")
    return p.parse_args(cascade_argv(arguments))


def write_captured(args, rec: Recordings, names: List[str], clips) -> None:
    """The clips of one recorder call as WAV files in mine_audio.py's layout."""
    h = clips.host()
    for i in range(len(h.stream)):
        folder = os.path.join(args.capture_dir, names[int(h.label[i])])
        os.makedirs(folder, exist_ok=True)
        stem = os.path.splitext(os.path.basename(rec.paths[int(h.stream[i])]))[0]
        write_wav(os.path.join(folder, f"{stem}_{format_time_ms(float(h.time_ms[i]))}.wav"), h.pcm[i], rec.rate)


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
    recorder = None
    if args.capture_dir is not None:
        source = live if live is not None else (cascade if cascade is not None else det)
        pending = 1 + max(0, -int(-args.capture_lead_ms * rec.rate // (1000 * step)))      # rows whose clips one call can complete
        recorder = StreamingRecorder(source, lead_ms=args.capture_lead_ms, capacity=len(args.wav) * pending, pcm=True)
    buf = torch.zeros((len(args.wav), step), dtype=torch.float32, device=det.device)
    for _, audio in rec.chunks():                   # the whole recordings, once
        for i in range(rec.n_steps):
            buf.copy_(audio[:, i * step:(i + 1) * step])
            out = push(buf)
            out = out if live is None else live.push(out)
            print_detections(rec, out, i, names, {})
            if recorder is not None:
                write_captured(args, rec, names, recorder.push(buf, out))
    if recorder is not None:
        write_captured(args, rec, names, recorder.flush())
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
