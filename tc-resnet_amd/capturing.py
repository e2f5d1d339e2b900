"""Capturing detections' audio on live streams (tcr_capture_* of include/tcresnet_hip.h): a `StreamingRecorder` rides next to a
streaming detector (`StreamingDetector`, `StreamingCascade`, `StreamingPhraseDetector`), is pushed the samples the detector was pushed
and the output it returned, and hands back the finished clips of that output's detections -- bitwise what `DetectionStage.mine`'s
gather cuts from the whole recording, however the streams were cut into pushes.  The audio lives in a ring per stream on the device;
a push only enqueues kernels and reads nothing back."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import TcrError
from .detection import PendingResets, RaggedScanOutput, _ragged_signals, _step_ms, reset_mask
from .runtime import stream_of
from .scoring import _class_mask


class CapturedHost(NamedTuple):
    """`CapturedClips.host()`: the clips written, trimmed, as host arrays -- clips float32 [n, n_samples], pcm int16 [n, n_samples] or
    None, and per clip stream, step (the detection's row, counted from the stream's start or last reset), time_ms (the end of that
    step's window, `mine`'s stamp), label and score."""
    clips: np.ndarray
    pcm: Optional[np.ndarray]
    stream: np.ndarray
    step: np.ndarray
    time_ms: np.ndarray
    label: np.ndarray
    score: np.ndarray


class CapturedClips:
    """What `StreamingRecorder.push` / `flush` return: the recorder's own device tensors, overwritten by its next call (copy what must
    survive it) -- clips float32 [capacity, n_samples], pcm int16 [capacity, n_samples] or None, stream int32, step int64, label int32,
    score float32 [capacity], in (stream, step) order, and count int32 [2]: the clips written, then the clips due (more than
    `capacity`: the rest were dropped).  Only the first count[0] rows are this call's.  Nothing is read back until asked: `len()`,
    `due` and `host()` read the count (and wait for the device)."""

    def __init__(self, recorder: "StreamingRecorder"):
        r = self._rec = recorder
        self.clips, self.pcm, self.stream, self.step, self.label, self.score, self.count = r._clips, r._pcm, r._stream, r._step, r._label, \
            r._score, r._count

    def __len__(self) -> int:
        return int(self.count[0].item())

    @property
    def due(self) -> int:
        return int(self.count[1].item())

    def host(self) -> CapturedHost:
        n, r = len(self), self._rec
        step = self.step[:n].cpu().numpy()
        return CapturedHost(self.clips[:n].cpu().numpy(), None if self.pcm is None else self.pcm[:n].cpu().numpy(),
                            self.stream[:n].cpu().numpy(), step, _step_ms(step, r.step_samples, r.sample_rate), self.label[:n].cpu().numpy(),
                            self.score[:n].cpu().numpy())

    def to_pool(self, device=None):
        """The clips written as the training input stage's int16 pool, as `MinedClips.to_pool`; needs a recorder with pcm=True."""
        from .datasets.augmentation_factory import PcmPool
        if self.pcm is None:
            raise TcrError("CapturedClips.to_pool: the recorder was built without pcm=True")
        n, m = len(self), int(self.pcm.shape[1])
        pool = PcmPool.__new__(PcmPool)
        pool.lib, pool.device = self._rec.lib, self.pcm.device if device is None else torch.device(device)
        pool.lengths = np.full(n, m, np.int64)
        pool.offsets = np.arange(n, dtype=np.int64) * m
        pool.data = self.pcm[:n].reshape(-1).to(pool.device) if n else torch.zeros(1, dtype=torch.int16, device=pool.device)
        return pool


def _stage_of(detector):
    """(the detection stage, the stream count) of a streaming detector, cascade or phrase detector."""
    for d in (detector, getattr(detector, "second", None), getattr(detector, "detector", None)):
        stage = getattr(d, "stage", None)
        if stage is not None and hasattr(detector, "n_streams"):
            return stage, int(detector.n_streams)
    raise TcrError(f"StreamingRecorder: {type(detector).__name__} has no detection stage and stream count")


class StreamingRecorder(PendingResets):
    """The clips behind a streaming detector's detections.  `detector`: a `StreamingDetector`, `StreamingCascade` or
    `StreamingPhraseDetector` (anything with a `stage` -- its own, its `second`'s or its `detector`'s -- and `n_streams`): it supplies
    the stream count, the step, the sample rate, the class count and the clip length (n_samples overrides that).  lead_ms: the clip
    ends that long after the detection's step (negative: before it); a positive lead delays the clip until its audio has been heard.
    classes: the detections to capture (default: every class from 2 on; for a phrase detector every phrase, i.e. every class but the
    background, its last).  capacity: the clips one call can return; when more are due the first `capacity` in (stream, step) order
    are returned and the rest dropped (`CapturedClips.due` tells).  pcm: also int16 clips, by mining's rounding.

    The state is one ring of n_samples + max(0, -lead) float32 samples per stream (4096 streams at one second of 16 kHz audio:
    262 MB).  A push enqueues six small kernels, allocates nothing once the workspace has grown to the largest call, and reads
    nothing back."""

    def __init__(self, detector, lead_ms: float = 0.0, classes: Optional[Sequence[int]] = None, capacity: int = 256, pcm: bool = False,
                 n_samples: Optional[int] = None):
        stage, S = _stage_of(detector)
        self.detector, self.lib, self.device = detector, stage.lib, stage.device
        self.n_streams, self.step_samples, self.sample_rate, self.num_classes = S, stage.step_samples, stage.sample_rate, stage.num_classes
        self.n_samples = int(stage.clip_samples if n_samples is None else n_samples)
        self.lead = int(round(float(lead_ms) * self.sample_rate / 1000.0))
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise TcrError(f"StreamingRecorder: capacity must be >= 1 (got {capacity})")
        phrase = hasattr(detector, "detector")
        default = range(self.num_classes - 1) if phrase else range(2, self.num_classes)
        cls = list(default) if classes is None else [int(c) for c in classes]
        lib, dev = self.lib, self.device
        self._cmask = torch.from_numpy(_class_mask("StreamingRecorder", cls, self.num_classes)).to(dev)
        nstate = lib.tcr_capture_state_bytes(S, self.step_samples, self.n_samples, self.lead)
        if nstate == 0:
            raise TcrError(f"StreamingRecorder: {lib.tcr_last_error().decode()}")
        self.state = torch.empty((nstate + 3) // 4, dtype=torch.float32, device=dev)
        self.delay_steps = max(0, -(-self.lead // self.step_samples))
        cap, n = self.capacity, self.n_samples
        self._clips = torch.zeros((cap, n), dtype=torch.float32, device=dev)
        self._pcm = torch.zeros((cap, n), dtype=torch.int16, device=dev) if pcm else None
        self._stream, self._step = torch.zeros(cap, dtype=torch.int32, device=dev), torch.zeros(cap, dtype=torch.int64, device=dev)
        self._label, self._score = torch.zeros(cap, dtype=torch.int32, device=dev), torch.zeros(cap, dtype=torch.float32, device=dev)
        self._count = torch.zeros(2, dtype=torch.int32, device=dev)
        self._init_resets(dev)
        self._mask_dev = torch.zeros(S, dtype=torch.uint8, device=dev)
        self._ws: Optional[torch.Tensor] = None
        self._workspace(max(S, S * self.delay_steps))
        lib.check(lib.tcr_capture_init(S, self.step_samples, n, self.lead, self.state.data_ptr(), stream_of(dev)), "tcr_capture_init")

    def _workspace(self, rows: int) -> torch.Tensor:
        """The calls' workspace: grown (never shrunk) to the largest call so far, so one-step pushes allocate nothing."""
        nws = self.lib.tcr_capture_workspace_bytes(rows)
        if nws == 0:
            raise TcrError(f"StreamingRecorder: {self.lib.tcr_last_error().decode()}")
        if self._ws is None or self._ws.numel() * 4 < nws:
            self._ws = torch.empty((nws + 3) // 4, dtype=torch.int32, device=self.device)
        return self._ws

    def _outputs(self):
        return (self.capacity, self._clips.data_ptr(), None if self._pcm is None else self._pcm.data_ptr(), self._stream.data_ptr(),
                self._step.data_ptr(), self._label.data_ptr(), self._score.data_ptr(), self._count.data_ptr(), stream_of(self.device))

    def _check_rows(self, out, shape) -> None:
        for name in ("top", "score", "is_new"):
            t = getattr(out, name)
            want = torch.float32 if name == "score" else torch.int32
            if tuple(t.shape) != shape or t.dtype != want or not t.is_contiguous() or t.device.type != self.device.type:
                raise TcrError(f"StreamingRecorder.push: the output's {name} {t.dtype} {tuple(t.shape)} on {t.device} is not contiguous "
                               f"{want} {shape} on {self.device}")
        p = getattr(out, "probs", None)
        if p is not None and int(p.shape[-1]) != self.num_classes:
            raise TcrError(f"StreamingRecorder.push: the output is over {int(p.shape[-1])} classes, the recorder's detector has "
                           f"{self.num_classes}")

    def _check_samples(self, samples: torch.Tensor, shape) -> None:
        if tuple(samples.shape) != shape:
            raise TcrError(f"StreamingRecorder.push: samples {tuple(samples.shape)} for an output of {shape} samples (rows * "
                           f"{self.step_samples} per stream)")
        if samples.dtype != torch.float32 or not samples.is_contiguous() or samples.device.type != self.device.type:
            raise TcrError(f"StreamingRecorder.push expects contiguous float32 samples on {self.device}, got {samples.dtype} on "
                           f"{samples.device}")

    def push(self, samples, out) -> CapturedClips:
        """`samples`: exactly what was given to the detector's `push`, `push_many` ([S, rows * step_samples]) or `push_ragged` (a list of
        S 1-D tensors or (packed, lengths)); `out`: what the detector returned for them -- a `StreamOutput`, `ScanOutput` or
        `RaggedScanOutput` (a phrase detector's or a cascade's outputs have the same form).  Returns the clips that became complete
        with these rows.  Only enqueues kernels."""
        lib, S, step, n = self.lib, self.n_streams, self.step_samples, self.n_samples
        head = (step, n, self.lead)
        if isinstance(out, RaggedScanOutput):
            if len(out) != S:
                raise TcrError(f"StreamingRecorder.push: the output holds {len(out)} streams, the recorder {S}")
            packed, lengths, _ = _ragged_signals("StreamingRecorder.push", "stream", samples, S)
            rows = np.diff(out.offsets)
            total = int(out.offsets[-1])
            if (lengths != rows * step).any():
                raise TcrError(f"StreamingRecorder.push: the streams' lengths {lengths.tolist()} are not the output's "
                               f"({(rows * step).tolist()} samples)")
            self._check_rows(out, (total,))
            self._check_samples(packed, (total * step,))
            if total == 0:                                      # (no rows in all: nothing to launch; the resets stay pending)
                self._count.zero_()
                return CapturedClips(self)
            ws = self._workspace(total)
            off_dev = torch.from_numpy(out.offsets).to(self.device)
            reset_ptr = self._begin_ragged_reset()
            lib.check(lib.tcr_capture_push_ragged(S, off_dev.data_ptr(), total, *head, packed.data_ptr(), out.top.data_ptr(),
                                                  out.score.data_ptr(), out.is_new.data_ptr(), self._cmask.data_ptr(), self.num_classes,
                                                  reset_ptr, self.state.data_ptr(), ws.data_ptr(), ws.numel() * 4, *self._outputs()),
                      "tcr_capture_push_ragged")
            self._end_ragged_reset(rows)
            return CapturedClips(self)
        if not isinstance(samples, torch.Tensor):
            raise TcrError("StreamingRecorder.push: a dense output needs the samples tensor [S, rows * step_samples] it was computed from")
        rows = 1 if out.top.dim() == 1 else int(out.top.shape[1])
        self._check_rows(out, (S,) if out.top.dim() == 1 else (S, rows))
        self._check_samples(samples, (S, rows * step))
        if rows == 0:
            self._count.zero_()
            return CapturedClips(self)
        ws = self._workspace(S * rows)
        lib.check(lib.tcr_capture_push(S, rows, *head, samples.data_ptr(), out.top.data_ptr(), out.score.data_ptr(), out.is_new.data_ptr(),
                                       self._cmask.data_ptr(), self.num_classes, self._take_reset(), self.state.data_ptr(), ws.data_ptr(),
                                       ws.numel() * 4, *self._outputs()), "tcr_capture_push")
        return CapturedClips(self)

    def flush(self, mask=None) -> CapturedClips:
        """The pending clips (detections of the last `delay_steps` rows, whose lead has not been heard yet) of the streams in `mask`
        (`reset`'s argument forms; None: all), audio not yet heard as zeros -- what `mine` gives for a detection near a recording's end.
        They are forgotten, so a stream that goes on does not return them again; the recordings go on as they were."""
        mask_ptr = None
        if mask is not None:
            self._mask_dev.copy_(torch.from_numpy(reset_mask(mask, self.n_streams).astype(np.uint8)))
            mask_ptr = self._mask_dev.data_ptr()
        ws = self._workspace(max(1, self.n_streams * self.delay_steps))
        self.lib.check(self.lib.tcr_capture_flush(self.n_streams, mask_ptr, self.step_samples, self.n_samples, self.lead, self.state.data_ptr(),
                                                  ws.data_ptr(), ws.numel() * 4, *self._outputs()), "tcr_capture_flush")
        return CapturedClips(self)
