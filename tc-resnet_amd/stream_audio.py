"""Streaming keyword detection over long WAV files with a frozen artifact (TC-ResNet, DS-CNN or 2-D graph; deploy.FrozenModel, include_preprocess):

    python stream_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] [--frames_per_step k] [--labels l0,l1,...]
                           [--average_window_ms MS] [--detection_threshold P] [--suppression_ms MS] [--min_count N]

Each file is one stream of a `streaming.StreamingDetector` (16-bit PCM; a file at another sample rate than the model's is converted
whole on the device first, `resampling.Resampler`, and noted on stderr); the files are fed in lockstep,
k * hop samples per step, and a file that has ended is fed zeros until every file is done.  Samples that do not fill a whole step
are dropped (noted on stderr).  One line per detection on stdout:  file,time_ms,label,score  -- time_ms is the end of the window
that fired (every stream starts as if it had heard one clip of silence)."""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

import numpy as np

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.datasets.augmentation_factory import read_wav_pcm16_rate
    from tcresnet_amd.deploy import FrozenModel
    from tcresnet_amd.resampling import Resampler
else:
    from .datasets.augmentation_factory import read_wav_pcm16_rate
    from .deploy import FrozenModel
    from .resampling import Resampler


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frozen", required=True, help="frozen artifact (.npz) of any model family exported with include_preprocess")
    p.add_argument("--wav", required=True, nargs="+", help="16-bit PCM WAV files, one stream each")
    p.add_argument("--frames_per_step", type=int, default=1, help="new front-end frames per step (k)")
    p.add_argument("--labels", default=None, help="comma-separated class names (default: class indices)")
    p.add_argument("--average_window_ms", type=float, default=1000.0)
    p.add_argument("--detection_threshold", type=float, default=0.5)
    p.add_argument("--suppression_ms", type=float, default=1500.0)
    p.add_argument("--min_count", type=int, default=3)
    return p.parse_args(arguments)


def format_time_ms(ms: float) -> str:
    return f"{round(ms, 3):g}"


def load_streams(paths: List[str], det) -> List[np.ndarray]:
    """Each file as float32 at the model's rate, cut to whole steps (host arrays): decoded on the host at the model's rate, converted
    whole on the device otherwise."""
    import torch
    step, sr = det.step_samples, det.frontend.cfg.sample_rate
    audio, resamplers = [], {}
    for path in paths:
        pcm, rate = read_wav_pcm16_rate(path)
        if rate == sr:
            pcm = pcm.astype(np.float32) * (1.0 / 32768.0)
        else:
            print(f"{path}: {rate} Hz -> {sr} Hz", file=sys.stderr)
            if rate not in resamplers:
                resamplers[rate] = Resampler(rate, sr, 1, device=det.device, lib=det.lib)
            pcm = resamplers[rate].resample(torch.from_numpy(np.array(pcm[None, :])).to(det.device))[0].cpu().numpy()
        if len(pcm) % step:
            print(f"{path}: dropping the last {len(pcm) % step} samples (not a whole step of {step})", file=sys.stderr)
        audio.append(pcm[:len(pcm) // step * step])
    return audio


def main(args) -> int:
    import torch
    model = FrozenModel.load(args.frozen)
    det = model.streaming(len(args.wav), frames_per_step=args.frames_per_step, average_window_ms=args.average_window_ms,
                          min_count=args.min_count, detection_threshold=args.detection_threshold, suppression_ms=args.suppression_ms)
    labels = args.labels.split(",") if args.labels else None
    step = det.step_samples
    audio = load_streams(args.wav, det)
    n_steps = max(len(a) for a in audio) // step
    host = np.zeros((len(audio), step), np.float32)
    buf = torch.zeros((len(audio), step), dtype=torch.float32, device=det.device)
    sr = det.frontend.cfg.sample_rate
    for i in range(n_steps):
        host[:] = 0.0
        for s, a in enumerate(audio):
            if (i + 1) * step <= len(a):
                host[s] = a[i * step:(i + 1) * step]
        buf.copy_(torch.from_numpy(host))
        out = det.push(buf)
        fired = out.is_new.cpu().numpy()
        if fired.any():
            top, score = out.top.cpu().numpy(), out.score.cpu().numpy()
            t_ms = 1000.0 * (i + 1) * step / sr
            for s in np.nonzero(fired)[0]:
                name = labels[top[s]] if labels else str(int(top[s]))
                print(f"{args.wav[s]},{format_time_ms(t_ms)},{name},{float(score[s]):.6f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
