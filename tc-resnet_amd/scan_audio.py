"""Offline keyword scanning of long WAV files with a frozen TC-ResNet artifact (deploy.FrozenModel, include_preprocess):

    python scan_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] [--frames_per_step k] [--labels l0,l1,...]
                         [--average_window_ms MS] [--detection_threshold P] [--suppression_ms MS] [--min_count N]
                         [--max_windows B] [--summary]

The files are scanned in one `scanning.KeywordScanner` call (16-bit PCM at the model's sample rate), zero-padded to the longest;
samples that do not fill a whole step are dropped (noted on stderr).  The output is stream_audio.py's, line for line: one line per
detection on stdout,  file,time_ms,label,score,  in step order and, within a step, in file order -- time_ms is the end of the
window that fired (every file starts as if it had heard one clip of silence).  --summary adds one JSON line on stderr: the hours
of audio scanned (each file's whole steps), the detections per label and the detections per hour."""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import List, Optional

import numpy as np

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.datasets.augmentation_factory import read_wav_pcm16
    from tcresnet_amd.deploy import FrozenModel
    from tcresnet_amd.stream_audio import format_time_ms
else:
    from .datasets.augmentation_factory import read_wav_pcm16
    from .deploy import FrozenModel
    from .stream_audio import format_time_ms


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frozen", required=True, help="frozen TC-ResNet artifact (.npz) exported with include_preprocess")
    p.add_argument("--wav", required=True, nargs="+", help="16-bit PCM WAV files, one signal each")
    p.add_argument("--frames_per_step", type=int, default=1, help="new front-end frames per step (k)")
    p.add_argument("--labels", default=None, help="comma-separated class names (default: class indices)")
    p.add_argument("--average_window_ms", type=float, default=1000.0)
    p.add_argument("--detection_threshold", type=float, default=0.5)
    p.add_argument("--suppression_ms", type=float, default=1500.0)
    p.add_argument("--min_count", type=int, default=3)
    p.add_argument("--max_windows", type=int, default=None, help="windows per network launch (the workspace's size)")
    p.add_argument("--summary", action="store_true", help="one JSON line of totals on stderr")
    return p.parse_args(arguments)


def main(args) -> int:
    import torch
    model = FrozenModel.load(args.frozen)
    scanner = model.scanner(frames_per_step=args.frames_per_step, average_window_ms=args.average_window_ms, min_count=args.min_count,
                            detection_threshold=args.detection_threshold, suppression_ms=args.suppression_ms,
                            max_windows=args.max_windows)
    labels = args.labels.split(",") if args.labels else None
    step = scanner.step_samples
    audio = []
    for path in args.wav:
        pcm = read_wav_pcm16(path).astype(np.float32) * (1.0 / 32768.0)
        if len(pcm) % step:
            print(f"{path}: dropping the last {len(pcm) % step} samples (not a whole step of {step})", file=sys.stderr)
        audio.append(pcm[:len(pcm) // step * step])
    n_steps = max(len(a) for a in audio) // step
    sr = scanner.frontend.cfg.sample_rate
    names = labels if labels else [str(c) for c in range(scanner.net.num_classes)]
    counts = {}
    if n_steps > 0:
        host = np.zeros((len(audio), n_steps * step), np.float32)
        for s, a in enumerate(audio):
            host[s, :len(a)] = a
        out = scanner.scan(torch.from_numpy(host).to(scanner.device))
        fired = out.is_new.cpu().numpy()
        top, score = out.top.cpu().numpy(), out.score.cpu().numpy()
        sig, at = np.nonzero(fired.T)                 # step-major: step order, then file order (stream_audio.py's order)
        for i, s in zip(sig, at):
            name = names[top[s, i]]
            counts[name] = counts.get(name, 0) + 1
            print(f"{args.wav[s]},{format_time_ms(1000.0 * (i + 1) * step / sr)},{name},{float(score[s, i]):.6f}", flush=True)
    if args.summary:
        hours = sum(len(a) for a in audio) / sr / 3600.0
        total = sum(counts.values())
        print(json.dumps({"hours": hours, "detections": total, "detections_per_label": counts,
                          "detections_per_hour": total / hours if hours > 0 else None}), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
