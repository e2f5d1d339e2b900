"""What scan_audio.py, stream_audio.py, sweep_audio.py and mine_audio.py share: the WAV parser (`WavFile`, the package's only one) and
writer (`write_wav`), the files as the
detector takes them (`Recordings`: whole steps at the model's rate, on its device, chunk by chunk or whole), the detection lines and
the --summary line, and the flags the tools have in common."""
from __future__ import annotations

import json
import os
import struct
import sys
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch

from .resampling import Resampler


class WavFile:
    """The header of a 16-bit PCM RIFF/WAVE file: `rate`, `channels`, `length` (frames).  `read_pcm(first, n)` returns channel 0 of
    the frames [first, first + n) as int16, zeros outside the file.  A data chunk that ends inside a frame counts its whole frames."""

    def __init__(self, path: str):
        self.path = path
        with open(path, "rb") as fh:
            size = os.fstat(fh.fileno()).st_size
            head = fh.read(12)
            if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
                raise ValueError(f"{path}: not a RIFF/WAVE file")
            pos, self.channels, self.rate, data = 12, 1, 0, None
            while pos + 8 <= size:
                fh.seek(pos)
                tag, n = fh.read(4), struct.unpack("<I", fh.read(4))[0]
                if tag == b"fmt ":
                    fmt, self.channels, self.rate, _br, _align, bits = struct.unpack("<HHIIHH", fh.read(16))
                    if fmt != 1 or bits != 16:
                        raise ValueError(f"{path}: only 16-bit PCM is supported (format {fmt}, {bits} bits)")
                elif tag == b"data":
                    data = (pos + 8, min(n, size - pos - 8))
                pos += 8 + n + (n & 1)
        if data is None:
            raise ValueError(f"{path}: no data chunk")
        self.start, self.length = data[0], data[1] // 2 // self.channels

    def read_pcm(self, first: int, n: int) -> np.ndarray:
        out = np.zeros(n, np.int16)
        lo, hi = max(first, 0), min(first + n, self.length)
        if hi > lo:
            with open(self.path, "rb") as fh:
                fh.seek(self.start + lo * 2 * self.channels)
                out[lo - first:hi - first] = np.frombuffer(fh.read((hi - lo) * 2 * self.channels), dtype="<i2").reshape(-1, self.channels)[:, 0]
        return out


def write_wav(path: str, pcm: np.ndarray, rate: int) -> None:
    """int16 samples as a 16-bit mono PCM RIFF/WAVE file at `rate` Hz: what `WavFile` (and the dataset loader through it) reads back
    sample for sample."""
    data = np.ascontiguousarray(np.asarray(pcm).reshape(-1), dtype="<i2").tobytes()
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        fh.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, int(rate), 2 * int(rate), 2, 16))
        fh.write(b"data" + struct.pack("<I", len(data)) + data)


class Recordings:
    """The files as `det` (a KeywordScanner or StreamingDetector) takes them.  Each file is parsed once; `lengths` are the files'
    lengths at the model's rate in whole steps' samples (a file at another rate counts with its converted length,
    ceil(n sample_rate / rate)), `n_steps` the longest's steps.  The conversions and the dropped samples are noted on stderr."""

    def __init__(self, paths: List[str], det):
        self.paths, self.det, self.step, self.rate = list(paths), det, det.step_samples, det.frontend.cfg.sample_rate
        self.files, self.lengths, self.resamplers = [WavFile(p) for p in paths], [], {}
        for f in self.files:
            n = f.length
            if f.rate != self.rate:
                print(f"{f.path}: {f.rate} Hz -> {self.rate} Hz", file=sys.stderr)
                n = -(-n * self.rate // f.rate)
            if n % self.step:
                print(f"{f.path}: dropping the last {n % self.step} samples (not a whole step of {self.step})", file=sys.stderr)
            self.lengths.append(n // self.step * self.step)
        self.n_steps = max(self.lengths) // self.step

    def resampler(self, rate: int) -> Resampler:
        """One `Resampler` per input rate, built when a file first needs it."""
        if rate not in self.resamplers:
            self.resamplers[rate] = Resampler(rate, self.rate, 1, device=self.det.device, lib=self.det.lib)
        return self.resamplers[rate]

    def chunks(self, chunk_seconds: Optional[float] = None) -> Iterator[Tuple[int, torch.Tensor]]:
        """(first step, float32 [N, m * step] on det's device) up to the longest file's last whole step, chunk_seconds (rounded down
        to whole steps) at a time; None: the whole recordings as one chunk.  A file that has ended reads as zeros.  A file at the
        model's rate is decoded on the host; of a file at another rate each chunk reads exactly the input span its outputs need
        (zeros outside the file) and converts it by global position on the device, so the chunks are the whole buffer's columns,
        bitwise, and no resampler state is kept."""
        chunk_steps = max(self.n_steps, 1) if chunk_seconds is None else int(chunk_seconds * self.rate) // self.step
        if chunk_steps < 1:
            raise SystemExit(f"--chunk_seconds {chunk_seconds:g} is shorter than one step ({self.step} samples)")
        dev = self.det.device
        for i0 in range(0, self.n_steps, chunk_steps):
            m, at = min(chunk_steps, self.n_steps - i0), i0 * self.step
            buf = torch.zeros((len(self.files), m * self.step), dtype=torch.float32, device=dev)
            for s, f in enumerate(self.files):
                keep = max(0, min(m * self.step, self.lengths[s] - at))
                if keep == 0:
                    continue
                if f.rate == self.rate:
                    buf[s, :keep] = torch.from_numpy(f.read_pcm(at, keep).astype(np.float32) * (1.0 / 32768.0)).to(dev)
                else:
                    rs = self.resampler(f.rate)
                    first, n = rs.span(at, keep)
                    rs.convert(torch.from_numpy(f.read_pcm(first, n)[None, :]).to(dev), first, at, keep, out=buf[s:s + 1, :keep])
            yield i0, buf

    def ragged_chunks(self, chunk_seconds: float) -> Iterator[Tuple[int, torch.Tensor, List[int]]]:
        """(first step, float32 1-D on det's device, lengths) chunk_seconds (rounded down to whole steps) at a time, up to the longest
        file's last whole step: every file contributes its next min(chunk, what remains) whole steps, possibly none, one after the
        other -- what `StreamingDetector.push_ragged` takes.  Every chunk covers the same step range of every file that still has
        steps, and a file's samples are the bytes `packed()` holds for them: the same host decode, the same `Resampler.convert` calls
        by global position."""
        chunk_steps = int(chunk_seconds * self.rate) // self.step
        if chunk_steps < 1:
            raise SystemExit(f"--ragged_chunk_seconds {chunk_seconds:g} is shorter than one step ({self.step} samples)")
        dev = self.det.device
        for i0 in range(0, self.n_steps, chunk_steps):
            at = i0 * self.step
            lengths = [max(0, min(chunk_steps * self.step, n - at)) for n in self.lengths]
            buf = torch.zeros(sum(lengths), dtype=torch.float32, device=dev)
            pos = 0
            for f, keep in zip(self.files, lengths):
                if keep == 0:
                    continue
                if f.rate == self.rate:
                    buf[pos:pos + keep] = torch.from_numpy(f.read_pcm(at, keep).astype(np.float32) * (1.0 / 32768.0)).to(dev)
                else:
                    rs = self.resampler(f.rate)
                    first, n = rs.span(at, keep)
                    rs.convert(torch.from_numpy(f.read_pcm(first, n)[None, :]).to(dev), first, at, keep, out=buf[pos:pos + keep].unsqueeze(0))
                pos += keep
            yield i0, buf, lengths

    def packed(self) -> Tuple[torch.Tensor, List[int]]:
        """(float32 1-D on det's device, lengths): the files one after the other, each at its own whole-step length -- what
        `KeywordScanner.scan_ragged` takes.  A file's samples are the columns `chunks()` yields for it, bitwise: decoded on the host at
        the model's rate, converted on the device by the same `Resampler` calls at another."""
        dev = self.det.device
        buf = torch.zeros(sum(self.lengths), dtype=torch.float32, device=dev)
        at = 0
        for f, keep in zip(self.files, self.lengths):
            if keep == 0:
                continue
            if f.rate == self.rate:
                buf[at:at + keep] = torch.from_numpy(f.read_pcm(0, keep).astype(np.float32) * (1.0 / 32768.0)).to(dev)
            else:
                rs = self.resampler(f.rate)
                first, n = rs.span(0, keep)
                rs.convert(torch.from_numpy(f.read_pcm(first, n)[None, :]).to(dev), first, 0, keep, out=buf[at:at + keep].unsqueeze(0))
            at += keep
        return buf, list(self.lengths)


def format_time_ms(ms: float) -> str:
    return f"{round(ms, 3):g}"


def print_detections(rec: Recordings, out, i0: int, names: List[str], counts: Dict[str, int]) -> None:
    """One line per detection of `out` (is_new / top / score [N, m], or [N] for one step: a ScanOutput or StreamOutput) on stdout,
    file,time_ms,label,score,  in step order and, within a step, in file order; `i0` is out's first step, time_ms the end of the
    window that fired.  `counts` gains the detections per label."""
    fired = out.is_new.cpu().numpy().reshape(len(rec.paths), -1)
    if not fired.any():
        return
    top, score = out.top.cpu().numpy().reshape(fired.shape), out.score.cpu().numpy().reshape(fired.shape)
    for i, s in zip(*np.nonzero(fired.T)):
        name = names[top[s, i]]
        counts[name] = counts.get(name, 0) + 1
        print(f"{rec.paths[s]},{format_time_ms(1000.0 * (i0 + i + 1) * rec.step / rec.rate)},{name},{float(score[s, i]):.6f}", flush=True)


def print_detections_ragged(rec: Recordings, out, names: List[str], counts: Dict[str, int], i0: int = 0) -> None:
    """`print_detections` for a scanning.RaggedScanOutput over rec's files: the same lines in the same order (step order, then file
    order); a file has no steps past its own end, so none is printed there.  `i0`: the step of every file that out's rows start at
    (a chunk of `Recordings.ragged_chunks`)."""
    fired = np.flatnonzero(out.is_new.cpu().numpy())
    if not fired.size:
        return
    top, score = out.top.cpu().numpy(), out.score.cpu().numpy()
    s = np.searchsorted(out.offsets, fired, side="right") - 1
    i = fired - out.offsets[s]
    for o in np.lexsort((s, i)):
        name = names[top[fired[o]]]
        counts[name] = counts.get(name, 0) + 1
        print(f"{rec.paths[s[o]]},{format_time_ms(1000.0 * (i0 + int(i[o]) + 1) * rec.step / rec.rate)},{name},{float(score[fired[o]]):.6f}", flush=True)


def summary_line(rec: Recordings, counts: Dict[str, int], extra: Optional[Dict[str, int]] = None) -> str:
    """--summary's JSON: the hours of audio (each file's whole steps), the detections per label and per hour; `extra`: more entries
    (a cascade run's selected_steps and total_steps)."""
    hours, total = sum(rec.lengths) / rec.rate / 3600.0, sum(counts.values())
    return json.dumps({"hours": hours, "detections": total, "detections_per_label": counts,
                       "detections_per_hour": total / hours if hours > 0 else None, **(extra or {})})


def add_detector_flags(p, each: str = "signal", threshold: bool = True, offline: bool = True, phrases: bool = False) -> None:
    """The model, input and detector flags of the three tools; `offline`: the scanning tools' --max_windows and --chunk_seconds;
    `phrases`: the --phrases flags of scan_audio.py, sweep_audio.py and stream_audio.py (`open_phrases`)."""
    p.add_argument("--frozen", required=True, help="frozen artifact (.npz) of any model family exported with include_preprocess")
    p.add_argument("--wav", required=True, nargs="+", help=f"16-bit PCM WAV files, one {each} each")
    p.add_argument("--frames_per_step", type=int, default=1, help="new front-end frames per step (k)")
    p.add_argument("--labels", default=None, help="comma-separated class names (default: class indices)")
    p.add_argument("--average_window_ms", type=float, default=1000.0)
    if threshold:
        p.add_argument("--detection_threshold", type=float, default=0.5)
    p.add_argument("--suppression_ms", type=float, default=1500.0)
    p.add_argument("--min_count", type=int, default=3)
    if offline:
        p.add_argument("--max_windows", type=int, default=None, help="windows per network launch (the workspace's size)")
        p.add_argument("--chunk_seconds", type=float, default=None, help="read and scan the files this many seconds at a time")
        p.add_argument("--ragged", action="store_true",
                       help="scan every file at its own length in one ragged call (KeywordScanner.scan_ragged): no padding to the longest")
        p.add_argument("--ragged_chunk_seconds", type=float, default=None,
                       help="read the files this many seconds at a time, each at its own length (StreamingDetector.push_ragged): --ragged's "
                            "output with one chunk of every file in host memory")
        p.add_argument("--second_frozen", default=None,
                       help="cascade (with --ragged): --frozen flags steps, this artifact rescores only those (CascadeScanner); the "
                            "detector flags configure the final detector, which is this model's")
        p.add_argument("--enter_threshold", type=float, default=None,
                       help="cascade: a step is flagged when a keyword class (every class from 2 on) of --frozen reaches this probability")
        p.add_argument("--cascade_pad_ms", type=float, default=None,
                       help="cascade: audio selected in front of and behind every flag (default: --average_window_ms minus one step)")
        p.add_argument("--second_frames_per_step", type=int, default=1, help="cascade: --second_frozen's frames per step")
        p.add_argument("--cascade_pad_before_ms", type=float, default=None,
                       help="cascade: audio selected in front of every flag, when it differs from --cascade_pad_ms behind it (default: "
                            "--cascade_pad_ms's value; 0: the causal cascade stream_audio.py computes)")
    else:
        p.add_argument("--second_frozen", default=None,
                       help="streaming cascade: --frozen steps every stream and flags, this artifact's network runs only on the flagged "
                            "streams (StreamingCascade); the detector flags configure the final detector, which is this model's")
        p.add_argument("--enter_threshold", type=float, default=None,
                       help="cascade: a stream is flagged when a keyword class (every class from 2 on) of --frozen reaches this probability")
        p.add_argument("--cascade_pad_ms", type=float, default=None,
                       help="cascade: audio a stream stays selected behind a flag (default: --average_window_ms minus one step)")
        p.add_argument("--second_frames_per_step", type=int, default=1, help="cascade: --second_frozen's frames per step")
    if phrases:
        p.add_argument("--phrases", default=None,
                       help='detect phrases instead of single words: "go left;stop no" (words: --labels names or class indices), or @FILE '
                            "with one phrase per line (scanning.PhraseDetector)" + ("; not with --chunk_seconds / --ragged_chunk_seconds" if offline else ""))
        p.add_argument("--phrase_window_ms", type=float, default=1500.0, help="phrases: the window a phrase's words must fall in")
        p.add_argument("--phrase_unordered", action="store_true", help="phrases: the words in any order (default: in the given order)")
        p.add_argument("--phrase_combine", choices=("product", "min"), default="product",
                       help="phrases: a phrase's score is the product or the minimum of its words' posteriors")
        p.add_argument("--templates", default=None,
                       help="detect enrolled keywords instead of the model's words: a TEMPLATES.npz of enroll_audio.py (scanning.TemplateDetector); "
                            "not with --phrases" + (" or --chunk_seconds / --ragged_chunk_seconds" if offline else ""))
        p.add_argument("--template_max_stretch", type=float, default=3.0,
                       help="templates: a match longer than this many times the longest template scores 0 (<= 0: no limit)")


def detector_settings(args) -> dict:
    """FrozenModel.scanner's / .streaming's keyword arguments from the flags the tool has."""
    keys = ("frames_per_step", "average_window_ms", "min_count", "detection_threshold", "suppression_ms", "max_windows")
    return {k: getattr(args, k) for k in keys if hasattr(args, k)}


def open_detector(model, args):
    """(detector, its call on one chunk): a KeywordScanner and `scan` for the one-call run, which allocates no stream state; with
    --chunk_seconds a StreamingDetector over the files and `push_many`, which carries the state from chunk to chunk; with
    --ragged_chunk_seconds the same detector and `push_ragged`, every file advancing by what it has left."""
    if getattr(args, "ragged", False) and args.chunk_seconds is not None:
        raise SystemExit("--ragged scans the whole files in one call: it cannot be combined with --chunk_seconds")
    if getattr(args, "ragged_chunk_seconds", None) is not None:
        if args.chunk_seconds is not None:
            raise SystemExit("--ragged_chunk_seconds reads every file at its own length: it cannot be combined with --chunk_seconds")
        if getattr(args, "ragged", False):
            raise SystemExit("--ragged_chunk_seconds is the chunked form of --ragged: give one of the two")
        det = model.streaming(len(args.wav), **detector_settings(args))
        return det, det.push_ragged
    if args.chunk_seconds is None:
        det = model.scanner(**detector_settings(args))
        return det, det.scan
    det = model.streaming(len(args.wav), **detector_settings(args))
    return det, det.push_many


def cascade_argv(argv: Optional[List[str]]) -> List[str]:
    """The command line with `--enter_threshold -inf` (which argparse reads as an option) joined into one word."""
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):
        if argv[i] == "--enter_threshold" and argv[i + 1].lower() in ("-inf", "-infinity"):
            argv[i:i + 2] = [f"--enter_threshold={argv[i + 1]}"]
            break
    return argv


def open_cascade(args):
    """The `scanning.CascadeScanner` of --second_frozen / --enter_threshold (None without them): --frozen at --frames_per_step is the
    first stage, --second_frozen at --second_frames_per_step the second, and the detector flags are the second's.  Accepted with
    --ragged only: a cascade carries no state from chunk to chunk."""
    check_cascade_flags(args)
    if getattr(args, "second_frozen", None) is None:
        return None
    if args.chunk_seconds is not None or args.ragged_chunk_seconds is not None or not args.ragged:
        raise SystemExit("--second_frozen (a cascade) runs with --ragged only: not with the padded one-call run, --chunk_seconds or "
                         "--ragged_chunk_seconds, because no state is carried")
    from .deploy import FrozenModel
    from .scanning import CascadeScanner
    settings = detector_settings(args)
    first = FrozenModel.load(args.frozen).scanner(**settings)
    second = FrozenModel.load(args.second_frozen).scanner(**dict(settings, frames_per_step=args.second_frames_per_step))
    before = args.cascade_pad_ms if getattr(args, "cascade_pad_before_ms", None) is None else args.cascade_pad_before_ms
    return CascadeScanner(first, second, args.enter_threshold, pad_before_ms=before, pad_after_ms=args.cascade_pad_ms)


def check_cascade_flags(args) -> None:
    """The cascade flags belong together (checked before any model is opened): --enter_threshold, --cascade_pad_ms and
    --cascade_pad_before_ms need --second_frozen, and --second_frozen needs --enter_threshold."""
    if getattr(args, "second_frozen", None) is None:
        if any(getattr(args, f, None) is not None for f in ("enter_threshold", "cascade_pad_ms", "cascade_pad_before_ms")):
            raise SystemExit("--enter_threshold, --cascade_pad_ms and --cascade_pad_before_ms belong to a cascade: give --second_frozen")
    elif args.enter_threshold is None:
        raise SystemExit("--second_frozen needs --enter_threshold")


def open_streaming_cascade(args, n_streams: int):
    """stream_audio.py's `streaming.StreamingCascade` of --second_frozen / --enter_threshold over n_streams streams (None without
    them): --frozen at --frames_per_step is the first stage, --second_frozen at --second_frames_per_step the second, the detector
    flags are the second's, and --cascade_pad_ms is the audio a stream stays selected behind a flag."""
    check_cascade_flags(args)
    if getattr(args, "second_frozen", None) is None:
        return None
    from .deploy import FrozenModel
    from .streaming import StreamingCascade
    settings = detector_settings(args)
    first = FrozenModel.load(args.frozen).streaming(n_streams, **settings)
    second = FrozenModel.load(args.second_frozen).streaming(n_streams, **dict(settings, frames_per_step=args.second_frames_per_step))
    return StreamingCascade(first, second, args.enter_threshold, pad_after_ms=args.cascade_pad_ms)


def check_phrase_flags(args) -> None:
    """--phrases is refused with the scanning tools' chunked runs (before any model is loaded); a tool without those flags
    (stream_audio.py) has nothing to refuse."""
    chunked = getattr(args, "chunk_seconds", None) is not None or getattr(args, "ragged_chunk_seconds", None) is not None
    if getattr(args, "phrases", None) is not None and chunked:
        raise SystemExit("--phrases scores whole scans: it cannot be combined with --chunk_seconds or --ragged_chunk_seconds (a chunk's "
                         "first steps would need the previous chunk's rows)")
    if getattr(args, "templates", None) is not None:
        if getattr(args, "phrases", None) is not None:
            raise SystemExit("--templates and --phrases are two detectors over the scan's posteriors: give one of them")
        if chunked:
            raise SystemExit("--templates scores whole scans: it cannot be combined with --chunk_seconds or --ragged_chunk_seconds (a chunk's "
                             "first steps would need the previous chunk's DTW column)")


def open_templates(args, scanner):
    """The `scanning.TemplateDetector` of --templates over `scanner`'s outputs (None without the flag): the enrolled keywords of an
    enroll_audio.py file, its threshold and suppression the detector flags', its labels the keyword names and _background_."""
    path = getattr(args, "templates", None)
    if path is None:
        return None
    from .templates import KeywordTemplates, TemplateDetector
    return TemplateDetector(scanner, KeywordTemplates.load(path), max_stretch=args.template_max_stretch)


def open_phrases(args, scanner):
    """The `scanning.PhraseDetector` of --phrases over `scanner`'s outputs (a `KeywordScanner`, or stream_audio.py's
    `StreamingDetector`; with --templates instead: `open_templates`' `scanning.TemplateDetector`, which has the same methods; None
    without either flag): its threshold and suppression are the detector flags', its labels the phrase names and _background_.  Refused with the scanning tools' chunked runs, which do not carry a phrase state yet."""
    check_phrase_flags(args)
    spec = getattr(args, "phrases", None)
    if spec is None:
        return open_templates(args, scanner)            # (--templates: the same place in the tools, the same methods)
    if spec.startswith("@"):
        with open(spec[1:]) as fh:
            lines = [x.strip() for x in fh]
    else:
        lines = [x.strip() for x in spec.split(";")]
    phrases = [x.split() for x in lines if x]
    from .scanning import PhraseDetector
    return PhraseDetector(scanner, phrases, window_ms=args.phrase_window_ms, ordered=not args.phrase_unordered, combine=args.phrase_combine,
                          labels=args.labels.split(",") if args.labels else None)


def label_names(args, det) -> List[str]:
    return args.labels.split(",") if args.labels else [str(c) for c in range(det.net.num_classes)]
