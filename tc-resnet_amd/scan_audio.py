"""Offline keyword scanning of long WAV files with a frozen artifact (TC-ResNet, DS-CNN or 2-D graph; deploy.FrozenModel, include_preprocess):

    python scan_audio.py --frozen MODEL.npz --wav a.wav [b.wav ...] [--frames_per_step k] [--labels l0,l1,...]
                         [--average_window_ms MS] [--detection_threshold P] [--suppression_ms MS] [--min_count N]
                         [--max_windows B] [--summary] [--chunk_seconds X]

The files are scanned in one `scanning.KeywordScanner` call (16-bit PCM), zero-padded to the longest; samples that do not fill a
whole step are dropped (noted on stderr).  A file at another sample rate than the model's (its `fmt ` chunk) is converted on the
device (`resampling.Resampler`: the int16 PCM is uploaded, one stderr line  a.wav: 48000 Hz -> 16000 Hz), its length is the
converted signal's, and time_ms is real time; files at the model's rate are decoded on the host as before.  With --chunk_seconds, the files are read X seconds at a time
(rounded down to whole steps) and fed to one `streaming.StreamingDetector` by `push_many`, so host memory holds one chunk per file;
a file that has ended reads as zeros until the longest ends, and the output is the one-call output, byte for byte.  The output is stream_audio.py's, line for line: one line per
detection on stdout,  file,time_ms,label,score,  in step order and, within a step, in file order -- time_ms is the end of the
window that fired (every file starts as if it had heard one clip of silence).  --summary adds one JSON line on stderr: the hours
of audio scanned (each file's whole steps), the detections per label and the detections per hour."""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
from typing import Iterator, List, Optional, Tuple

import numpy as np

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.datasets.augmentation_factory import read_wav_pcm16_rate
    from tcresnet_amd.deploy import FrozenModel
    from tcresnet_amd.resampling import Resampler
    from tcresnet_amd.stream_audio import format_time_ms
else:
    from .datasets.augmentation_factory import read_wav_pcm16_rate
    from .deploy import FrozenModel
    from .resampling import Resampler
    from .stream_audio import format_time_ms


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frozen", required=True, help="frozen artifact (.npz) of any model family exported with include_preprocess")
    p.add_argument("--wav", required=True, nargs="+", help="16-bit PCM WAV files, one signal each")
    p.add_argument("--frames_per_step", type=int, default=1, help="new front-end frames per step (k)")
    p.add_argument("--labels", default=None, help="comma-separated class names (default: class indices)")
    p.add_argument("--average_window_ms", type=float, default=1000.0)
    p.add_argument("--detection_threshold", type=float, default=0.5)
    p.add_argument("--suppression_ms", type=float, default=1500.0)
    p.add_argument("--min_count", type=int, default=3)
    p.add_argument("--max_windows", type=int, default=None, help="windows per network launch (the workspace's size)")
    p.add_argument("--summary", action="store_true", help="one JSON line of totals on stderr")
    p.add_argument("--chunk_seconds", type=float, default=None, help="read and scan the files this many seconds at a time")
    return p.parse_args(arguments)


class WavReader:
    """Channel 0 of a 16-bit PCM WAV file (read_wav_pcm16's parsing), read sequentially without loading the file: `read(n)` returns
    the next n samples as float32 / 32768, zeros past the end.  `rate` is the file's sample rate; `read_pcm(first, n)` returns the
    int16 samples [first, first + n) from anywhere in the file, zeros outside it."""

    def __init__(self, path: str):
        self.fh = open(path, "rb")
        size = os.fstat(self.fh.fileno()).st_size
        head = self.fh.read(12)
        if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        pos, self.channels, self.rate, data = 12, 1, 0, None
        while pos + 8 <= size:
            self.fh.seek(pos)
            tag, n = self.fh.read(4), struct.unpack("<I", self.fh.read(4))[0]
            if tag == b"fmt ":
                fmt, self.channels, self.rate, _br, _align, bits = struct.unpack("<HHIIHH", self.fh.read(16))
                if fmt != 1 or bits != 16:
                    raise ValueError(f"{path}: only 16-bit PCM is supported (format {fmt}, {bits} bits)")
            elif tag == b"data":
                data = (pos + 8, min(n, size - pos - 8))
            pos += 8 + n + (n & 1)
        if data is None:
            raise ValueError(f"{path}: no data chunk")
        self.start, self.length, self.pos = data[0], data[1] // 2 // self.channels, 0

    def read(self, n: int) -> np.ndarray:
        out = np.zeros(n, np.float32)
        m = max(0, min(n, self.length - self.pos))
        if m:
            self.fh.seek(self.start + self.pos * 2 * self.channels)
            pcm = np.frombuffer(self.fh.read(m * 2 * self.channels), dtype="<i2").reshape(-1, self.channels)[:, 0]
            out[:m] = pcm.astype(np.float32) * (1.0 / 32768.0)
        self.pos += n
        return out

    def read_pcm(self, first: int, n: int) -> np.ndarray:
        out = np.zeros(n, np.int16)
        lo, hi = max(first, 0), min(first + n, self.length)
        if hi > lo:
            self.fh.seek(self.start + lo * 2 * self.channels)
            out[lo - first:hi - first] = np.frombuffer(self.fh.read((hi - lo) * 2 * self.channels), dtype="<i2").reshape(-1, self.channels)[:, 0]
        return out


def whole_step_lengths(paths: List[str], step: int, sample_rate: Optional[int] = None) -> List[int]:
    """Each file's length in whole steps' samples; the dropped samples are noted on stderr (as the one-call path notes them).  With
    sample_rate, a file at another rate counts with its converted length, ceil(n sample_rate / rate), and is noted on stderr too."""
    lengths = []
    for path in paths:
        r = WavReader(path)
        n = r.length
        if sample_rate is not None and r.rate != sample_rate:
            print(f"{path}: {r.rate} Hz -> {sample_rate} Hz", file=sys.stderr)
            n = -(-n * sample_rate // r.rate)
        if n % step:
            print(f"{path}: dropping the last {n % step} samples (not a whole step of {step})", file=sys.stderr)
        lengths.append(n // step * step)
    return lengths


class _Resamplers:
    """One `Resampler` per input rate, built when a file first needs it."""

    def __init__(self, det):
        self.det, self.by_rate = det, {}

    def get(self, rate: int) -> "Resampler":
        if rate not in self.by_rate:
            self.by_rate[rate] = Resampler(rate, self.det.frontend.cfg.sample_rate, 1, device=self.det.device, lib=self.det.lib)
        return self.by_rate[rate]


def load_signals(paths: List[str], det):
    """The files as the detector takes them: (float32 [N, n_steps * step] on det's device, each file's length in whole steps'
    samples), rows zero-padded to the longest.  Files at the model's rate are decoded on the host; the others are uploaded as
    int16 and converted on the device, each into its row.  None for the buffer when no file holds a whole step."""
    import torch
    step, sr = det.step_samples, det.frontend.cfg.sample_rate
    lengths = whole_step_lengths(paths, step, sr)
    n = max(lengths)
    if n == 0:
        return None, lengths
    pcms = [read_wav_pcm16_rate(path) for path in paths]
    if all(rate == sr for _, rate in pcms):
        host = np.zeros((len(paths), n), np.float32)
        for s, (pcm, _) in enumerate(pcms):
            host[s, :lengths[s]] = (pcm.astype(np.float32) * (1.0 / 32768.0))[:lengths[s]]
        return torch.from_numpy(host).to(det.device), lengths
    buf = torch.zeros((len(paths), n), dtype=torch.float32, device=det.device)
    rs = _Resamplers(det)
    for s, (pcm, rate) in enumerate(pcms):
        if lengths[s] == 0:
            continue
        if rate == sr:
            buf[s, :lengths[s]] = torch.from_numpy((pcm.astype(np.float32) * (1.0 / 32768.0))[:lengths[s]]).to(det.device)
        else:
            rs.get(rate).convert(torch.from_numpy(np.array(pcm[None, :])).to(det.device), 0, 0, lengths[s], out=buf[s:s + 1, :lengths[s]])
    return buf, lengths


def signal_chunks(paths: List[str], det, chunk_seconds: float):
    """wav_chunks for files of any rate, on det's device: (first step, float32 [N, m * step]).  For a file at another rate than the
    model's, each chunk reads exactly the input span its outputs need (seeking back for the overlap, zeros outside the file) and
    converts it by global position, so the chunks are the one-call buffer's columns, bitwise; no resampler state is kept."""
    import torch
    step, sr = det.step_samples, det.frontend.cfg.sample_rate
    readers = [WavReader(p) for p in paths]
    if all(r.rate == sr for r in readers):
        for i0, host in wav_chunks(paths, step, chunk_seconds, sr):
            yield i0, torch.from_numpy(host).to(det.device)
        return
    chunk_steps = int(chunk_seconds * sr) // step
    if chunk_steps < 1:
        raise SystemExit(f"--chunk_seconds {chunk_seconds:g} is shorter than one step ({step} samples)")
    lengths = [(r.length if r.rate == sr else -(-r.length * sr // r.rate)) // step * step for r in readers]
    n_steps = max(lengths) // step
    rs = _Resamplers(det)
    for i0 in range(0, n_steps, chunk_steps):
        m = min(chunk_steps, n_steps - i0)
        buf = torch.zeros((len(paths), m * step), dtype=torch.float32, device=det.device)
        for s, r in enumerate(readers):
            keep = max(0, min(m * step, lengths[s] - i0 * step))
            if keep == 0:
                continue
            if r.rate == sr:
                r.pos = i0 * step
                buf[s, :keep] = torch.from_numpy(r.read(keep)).to(det.device)
            else:
                first, n = rs.get(r.rate).span(i0 * step, keep)
                x = torch.from_numpy(r.read_pcm(first, n)[None, :]).to(det.device)
                rs.get(r.rate).convert(x, first, i0 * step, keep, out=buf[s:s + 1, :keep])
        yield i0, buf


def wav_chunks(paths: List[str], step: int, chunk_seconds: float, sample_rate: int) -> Iterator[Tuple[int, np.ndarray]]:
    """(first step, samples [N, m * step]) of the files chunk by chunk, chunk_seconds rounded down to whole steps, up to the longest
    file's last whole step; a file that has ended (or ends inside its last partial step) reads as zeros."""
    chunk_steps = int(chunk_seconds * sample_rate) // step
    if chunk_steps < 1:
        raise SystemExit(f"--chunk_seconds {chunk_seconds:g} is shorter than one step ({step} samples)")
    readers = [WavReader(p) for p in paths]
    lengths = [r.length // step * step for r in readers]
    n_steps = max(lengths) // step
    for i0 in range(0, n_steps, chunk_steps):
        m = min(chunk_steps, n_steps - i0)
        host = np.zeros((len(paths), m * step), np.float32)
        for s, r in enumerate(readers):
            x = r.read(m * step)
            keep = max(0, min(m * step, lengths[s] - i0 * step))
            host[s, :keep] = x[:keep]
        yield i0, host


def main(args) -> int:
    if args.chunk_seconds is not None:
        return main_chunked(args)
    model = FrozenModel.load(args.frozen)
    scanner = model.scanner(frames_per_step=args.frames_per_step, average_window_ms=args.average_window_ms, min_count=args.min_count,
                            detection_threshold=args.detection_threshold, suppression_ms=args.suppression_ms,
                            max_windows=args.max_windows)
    labels = args.labels.split(",") if args.labels else None
    step = scanner.step_samples
    samples, lengths = load_signals(args.wav, scanner)
    sr = scanner.frontend.cfg.sample_rate
    names = labels if labels else [str(c) for c in range(scanner.net.num_classes)]
    counts = {}
    if samples is not None:
        out = scanner.scan(samples)
        fired = out.is_new.cpu().numpy()
        top, score = out.top.cpu().numpy(), out.score.cpu().numpy()
        sig, at = np.nonzero(fired.T)                 # step-major: step order, then file order (stream_audio.py's order)
        for i, s in zip(sig, at):
            name = names[top[s, i]]
            counts[name] = counts.get(name, 0) + 1
            print(f"{args.wav[s]},{format_time_ms(1000.0 * (i + 1) * step / sr)},{name},{float(score[s, i]):.6f}", flush=True)
    if args.summary:
        hours = sum(lengths) / sr / 3600.0
        total = sum(counts.values())
        print(json.dumps({"hours": hours, "detections": total, "detections_per_label": counts,
                          "detections_per_hour": total / hours if hours > 0 else None}), file=sys.stderr)
    return 0


def main_chunked(args) -> int:
    model = FrozenModel.load(args.frozen)
    det = model.streaming(len(args.wav), frames_per_step=args.frames_per_step, average_window_ms=args.average_window_ms,
                          min_count=args.min_count, detection_threshold=args.detection_threshold, suppression_ms=args.suppression_ms,
                          max_windows=args.max_windows)
    labels = args.labels.split(",") if args.labels else None
    step, sr = det.step_samples, det.frontend.cfg.sample_rate
    names = labels if labels else [str(c) for c in range(det.net.num_classes)]
    lengths = whole_step_lengths(args.wav, step, sr)
    counts = {}
    for i0, samples in signal_chunks(args.wav, det, args.chunk_seconds):
        out = det.push_many(samples)
        fired = out.is_new.cpu().numpy()
        top, score = out.top.cpu().numpy(), out.score.cpu().numpy()
        sig, at = np.nonzero(fired.T)                 # step-major within the chunk; chunks come in step order
        for i, s in zip(sig, at):
            name = names[top[s, i]]
            counts[name] = counts.get(name, 0) + 1
            print(f"{args.wav[s]},{format_time_ms(1000.0 * (i0 + i + 1) * step / sr)},{name},{float(score[s, i]):.6f}", flush=True)
    if args.summary:
        hours = sum(lengths) / sr / 3600.0
        total = sum(counts.values())
        print(json.dumps({"hours": hours, "detections": total, "detections_per_label": counts,
                          "detections_per_hour": total / hours if hours > 0 else None}), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
