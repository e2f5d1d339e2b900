"""What a scan hands on, and the stage that works on it.  The scans' output containers (`ScanOutput`, `RaggedScanOutput`, `CascadeOutput`),
the arithmetic between milliseconds, samples and steps, and `DetectionStage`: what runs on a scan's outputs without the network or the
front-end that made them -- the detector rule with other settings (`redetect`), sweeps and grids against labelled events (`sweep`, `tune`)
and mining (`mine`) -- and what every streaming class does with `reset` (`PendingResets`, `reset_mask`).  `streaming.StreamingDetector` and `scanning.KeywordScanner` build one over their model's classes,
`phrases.PhraseDetector` one over its phrases; the raw-tensor functions it calls are in `scoring` and `mining`."""
from __future__ import annotations

import ctypes as C
from typing import Iterator, NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import DetectCfg, TcrError
from .engine import _Base
from .mining import MINE_KINDS, MinedClips, _mine_workspace, gather_clips, mine_detections, mine_peaks, select_top
from .runtime import stream_of
from .scoring import GridPoint, GridResult, SweepResult, _class_mask, detection_grid, detection_sweep

DEFAULT_MAX_WINDOWS = 4096


class ScanOutput(NamedTuple):
    """Results of a scan, on the device: logits / probs / smoothed [N, steps, classes] float32, top [N, steps] int32 (-1 before
    min_count steps), score [N, steps] float32, is_new [N, steps] int32 (1: a new detection of `top` at that step)."""
    logits: torch.Tensor
    probs: torch.Tensor
    smoothed: torch.Tensor
    top: torch.Tensor
    score: torch.Tensor
    is_new: torch.Tensor


class RaggedScanOutput:
    """Results of a ragged scan (`KeywordScanner.scan_ragged`), on the device, packed over the signals' steps: logits / probs /
    smoothed [total_steps, classes] float32, top / score / is_new [total_steps]; `offsets` (host int64 [N + 1], in steps): signal n's
    steps are rows offsets[n] .. offsets[n + 1] - 1.  `len()` is N; `signal(n)` is that signal's rows as a `ScanOutput` of views with
    a leading dimension of 1, what `scan` of the signal alone returns."""
    FIELDS = ScanOutput._fields

    def __init__(self, logits, probs, smoothed, top, score, is_new, offsets: np.ndarray):
        self.logits, self.probs, self.smoothed, self.top, self.score, self.is_new = logits, probs, smoothed, top, score, is_new
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def tensors(self) -> Iterator[Optional[torch.Tensor]]:
        return (getattr(self, f) for f in self.FIELDS)

    @property
    def steps(self) -> np.ndarray:
        """Every signal's steps, host int64 [N]."""
        return np.diff(self.offsets)

    def signal(self, n: int) -> ScanOutput:
        if not 0 <= n < len(self):
            raise IndexError(f"signal {n} of {len(self)}")
        a, b = int(self.offsets[n]), int(self.offsets[n + 1])
        return ScanOutput(*(None if t is None else t[a:b].unsqueeze(0) for t in self.tensors()))


class CascadeOutput(RaggedScanOutput):
    """Results of a cascade scan: a `RaggedScanOutput` of the merged posteriors and the final (second-stage) detector over them, so
    `sweep` and `tune` of the second scanner take it unchanged.  `selected` (device int64): the packed steps the second model
    computed; `first`: the first stage's own `RaggedScanOutput`."""

    def __init__(self, logits, probs, smoothed, top, score, is_new, offsets, selected: torch.Tensor, first: RaggedScanOutput):
        super().__init__(logits, probs, smoothed, top, score, is_new, offsets)
        self.selected, self.first = selected, first


def ms_to_steps(ms: float, step_ms: float) -> int:
    """Milliseconds -> whole steps (nearest)."""
    return int(round(float(ms) / step_ms))


def check_on(what: str, on: str, choices=("smoothed", "probs")) -> str:
    """`on`, one of an output's two posterior tensors; the message names `choices` in their order."""
    if on not in choices:
        raise TcrError(f"{what}: on must be {choices[0]!r} or {choices[1]!r}, got {on!r}")
    return on


def reset_mask(mask_or_indices, n_streams: int) -> np.ndarray:
    """The `reset` argument of the streaming detectors as a bool mask [n_streams]: a bool / uint8 mask of that many entries, or
    stream indices (any other integer type)."""
    if isinstance(mask_or_indices, torch.Tensor):
        mask_or_indices = mask_or_indices.cpu().numpy()
    arr = np.asarray(mask_or_indices if not isinstance(mask_or_indices, (set, frozenset)) else sorted(mask_or_indices))
    if arr.dtype in (np.bool_, np.uint8):
        if arr.shape != (n_streams,):
            raise TcrError(f"reset mask must have {n_streams} entries, got shape {arr.shape}")
        return arr.astype(bool)
    idx = arr.astype(np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= n_streams):
        raise TcrError(f"reset: stream index outside 0..{n_streams - 1}")
    mask = np.zeros(n_streams, bool)
    mask[idx] = True
    return mask


class PendingResets:
    """The pending-reset rule of everything that carries state for `n_streams` streams: `reset` collects flags on the host (`_pending`:
    None, or a bool array of S entries), the next call takes them to the device (`_reset_dev`, uint8 [S]) and passes that pointer on.
    A ragged call ignores the flag of a stream it brings no rows for, so there the flags stay pending until the call has run and only
    those of the streams that had rows are dropped."""

    def _init_resets(self, device) -> None:
        self._reset_dev = torch.zeros(self.n_streams, dtype=torch.uint8, device=device)
        self._pending: Optional[np.ndarray] = None

    def reset(self, mask_or_indices) -> None:
        """Return streams to their initial state at their NEXT pushed row, before it: a bool / uint8 mask of S entries, or stream
        indices (any other integer type); calls accumulate.  A reset stays pending for a stream that has no rows in a ragged push.
        The initial state is the class's: a `StreamingDetector`'s silent clip, empty ring and no detection yet; a phrase or template
        detector's no rows seen and no detection yet; a `StreamingRecorder`'s pending triggers dropped, earlier audio read as zeros and
        steps counted from 0 (reset the recorder whenever the detector is)."""
        mask = reset_mask(mask_or_indices, self.n_streams)
        self._pending = mask if self._pending is None else (self._pending | mask)

    def _begin_ragged_reset(self) -> Optional[int]:
        """The reset pointer of a ragged call (None: no flags); the flags stay pending until `_end_ragged_reset`."""
        if self._pending is None:
            return None
        self._reset_dev.copy_(torch.from_numpy(self._pending.astype(np.uint8)))
        return self._reset_dev.data_ptr()

    def _end_ragged_reset(self, rows_per_stream) -> None:
        """After a ragged call that ran: only the flags of the streams without rows in it are kept."""
        if self._pending is not None:
            left = self._pending & (np.asarray(rows_per_stream) == 0)
            self._pending = left if left.any() else None

    def _take_reset(self) -> Optional[int]:
        """The reset pointer of a call in which every stream has rows (None: no flags); the flags are cleared."""
        ptr = self._begin_ragged_reset()
        self._pending = None
        return ptr


def _ragged_signals(what: str, noun: str, signals, count: Optional[int] = None):
    """The `signals` argument of `what` (scan_ragged, push_ragged) -> (packed, lengths, offsets in samples [N + 1]): a list of 1-D
    tensors, one per `noun`, or (packed, lengths).  count: the signals the caller expects (None: any number, a list not empty)."""
    if isinstance(signals, tuple) and len(signals) == 2 and isinstance(signals[0], torch.Tensor):
        packed, lengths = signals[0], np.asarray(signals[1], dtype=np.int64).reshape(-1)
        if packed.dim() != 1:
            raise TcrError(f"{what} expects a packed 1-D tensor, got shape {tuple(packed.shape)}")
    else:
        signals = list(signals)
        for n, x in enumerate(signals):
            if not isinstance(x, torch.Tensor) or x.dim() != 1:
                raise TcrError(f"{what} expects 1-D tensors, {noun} {n} is {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        lengths = np.array([int(x.shape[0]) for x in signals], dtype=np.int64)
        if count is None and not signals:
            raise TcrError(f"{what}: no signals")
        packed = signals[0] if len(signals) == 1 else (torch.cat(signals) if signals else None)
    if count is not None and int(lengths.size) != count:
        raise TcrError(f"{what} expects {count} signals (one per stream, empty for a stream without steps), got {int(lengths.size)}")
    offsets = np.zeros(int(lengths.size) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    if int(offsets[-1]) != int(packed.shape[0]) and (lengths >= 0).all():
        raise TcrError(f"{what}: the lengths sum to {int(offsets[-1])} samples, the packed tensor has {int(packed.shape[0])}")
    return packed, lengths, offsets


def _new_tensors(rows, ncls: int, dev, wide: int = 3):
    """New tensors of a scan's output over `rows` (a shape): `wide` of logits / probs / smoothed [*rows, ncls], then top, score, is_new."""
    return (*(torch.empty((*rows, ncls), dtype=torch.float32, device=dev) for _ in range(wide)),
            *(torch.empty(tuple(rows), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32)))


def _scan_output(n: int, steps: int, ncls: int, dev):
    """A `ScanOutput` of new tensors for n signals x steps."""
    return ScanOutput(*_new_tensors((n, steps), ncls, dev))


def _ragged_scan_output(lengths: np.ndarray, offsets: np.ndarray, step: int, ncls: int, dev):
    """A `RaggedScanOutput` of new tensors for signals of `lengths` samples (`offsets`: their running sum) at `step` samples a
    step; without rows when a length is no whole number of steps (the call refuses then, and the outputs are not written)."""
    ok = lengths.size > 0 and bool((lengths >= 0).all()) and not (lengths % step).any()
    total = int(offsets[-1]) // step if ok else 0
    return RaggedScanOutput(*_new_tensors((total,), ncls, dev), offsets // step)


def _step_ms(i: np.ndarray, step: int, sr: int) -> np.ndarray:
    return 1000.0 * (i + 1) * step / sr


def _first_steps(start_ms: np.ndarray, step: int, sr: int) -> np.ndarray:
    """Per entry, the first step i >= 0 with _step_ms(i) >= start_ms."""
    i = np.maximum(0, np.ceil(start_ms * sr / (1000.0 * step)) - 1).astype(np.int64)
    while (m := _step_ms(i, step, sr) < start_ms).any():
        i[m] += 1
    while (m := (i > 0) & (_step_ms(i - 1, step, sr) >= start_ms)).any():
        i[m] -= 1
    return i


def _last_steps(end_ms: np.ndarray, step: int, sr: int) -> np.ndarray:
    """Per entry, the last step i with _step_ms(i) <= end_ms (-1: none)."""
    i = np.maximum(-1, np.floor(end_ms * sr / (1000.0 * step)) - 1).astype(np.int64)
    while (m := (i >= 0) & (_step_ms(i, step, sr) > end_ms)).any():
        i[m] -= 1
    while (m := _step_ms(i + 1, step, sr) <= end_ms).any():
        i[m] += 1
    return i


class DetectionStage:
    """The detector-side stage over a scan's outputs: `num_classes` classes on `device`, steps of `step_samples` samples at `sample_rate`
    Hz, clips of `clip_samples` samples (what `mine` cuts) and the detector settings in steps, `det` (a `DetectCfg`; `detect_cfg` makes
    one from ms).  It owns no model: a keyword scanner's stage has the network's classes, a phrase detector's its P + 1 posteriors.  The
    workspace of `mine`'s calls is kept between calls."""

    def __init__(self, lib, device, num_classes: int, step_samples: int, sample_rate: int, clip_samples: int, det: Optional[DetectCfg] = None):
        self.lib, self.device, self.num_classes = lib, torch.device(device), int(num_classes)
        self.step_samples, self.sample_rate, self.clip_samples = int(step_samples), int(sample_rate), int(clip_samples)
        self.step_ms = 1000.0 * self.step_samples / self.sample_rate
        self.det, self._mine_ws = det, None

    _check_tensor = _Base._check_tensor                     # (the models' rule: the device's type, float32, contiguous; it reads self.device)

    def detect_cfg(self, average_window_ms: float, min_count: int, detection_threshold: float, suppression_ms: float) -> DetectCfg:
        """The detector settings in steps (the nearest whole number; the averaging ring holds at least one vector).  None: this stage's
        own setting, in steps as it is (not its ms converted again)."""
        own = self.det
        return DetectCfg(own.average_steps if average_window_ms is None else max(1, ms_to_steps(average_window_ms, self.step_ms)),
                         own.min_count if min_count is None else int(min_count),
                         own.suppression_steps if suppression_ms is None else max(0, ms_to_steps(suppression_ms, self.step_ms)),
                         own.threshold if detection_threshold is None else float(detection_threshold))

    def event_steps(self, out, events, lengths=None, tolerance_ms: float = 1000.0, labels: Optional[Sequence[str]] = None):
        """`sweep`'s (and `tune`'s, `mine`'s) arguments in steps: (out is ragged, every signal's valid steps, the events as
        inclusive step ranges per signal or None); the shapes come from out.probs where out.top is None."""
        step, sr = self.step_samples, self.sample_rate
        shape = out.top.shape if out.top is not None else out.probs.shape
        ragged = isinstance(out, RaggedScanOutput)
        if ragged:
            if lengths is not None:
                raise TcrError("sweep: lengths given with a ragged scan (the scan's lengths are the lengths)")
            N, steps, valid = len(out), 0, out.steps
            lengths = (valid * step).tolist()           # (the events below are checked against each signal's own end)
        else:
            N, steps = int(shape[0]), int(shape[1])
            valid = np.full(N, steps, np.int64)
            if lengths is not None:
                lens = np.asarray(lengths, np.int64).reshape(-1)
                if lens.shape != (N,):
                    raise TcrError(f"sweep: {lens.size} lengths for {N} signals")
                if (lens < 0).any() or (lens // step > steps).any():
                    raise TcrError(f"sweep: lengths outside 0..{steps * step} samples (the scan's): {lens.tolist()}")
                valid = lens // step
        ev_steps = None
        if events is not None:
            if len(events) != N:
                raise TcrError(f"sweep: events for {len(events)} signals, the scan has {N}")
            names = {str(x): c for c, x in enumerate(labels)} if labels is not None else {}
            ncls, tol = self.num_classes, float(tolerance_ms)
            ev_steps = []
            for n, evs in enumerate(events):
                length_ms = 1000.0 * (float(lengths[n]) if lengths is not None else float(steps * step)) / sr
                cls = [names.get(e[2]) if isinstance(e[2], str) else int(e[2]) for e in evs]
                for e, c in zip(evs, cls):
                    if c is None or not 0 <= c < ncls:
                        raise TcrError(f"sweep: signal {n}: event {tuple(e)} has an unknown label {e[2]!r}")
                se = np.array([(float(e[0]), float(e[1])) for e in evs], np.float64).reshape(-1, 2)
                bad = np.flatnonzero(~(se[:, 1] >= se[:, 0]))
                if bad.size:
                    raise TcrError(f"sweep: signal {n}: event {tuple(evs[bad[0]])} ends before it starts")
                bad = np.flatnonzero(se[:, 0] > length_ms)
                if bad.size:
                    raise TcrError(f"sweep: signal {n}: event {tuple(evs[bad[0]])} starts past the signal's end ({length_ms:g} ms)")
                order = np.lexsort((se[:, 1], se[:, 0]))
                se, cls = se[order], np.asarray(cls, np.int64).reshape(-1)[order]
                ov = np.flatnonzero(se[1:, 0] <= se[:-1, 1] + tol)
                if ov.size:
                    a, b = evs[order[ov[0]]], evs[order[ov[0] + 1]]
                    raise TcrError(f"sweep: signal {n}: events {tuple(a)} and {tuple(b)} overlap with tolerance_ms = {tol:g}")
                ev_steps.append(np.stack([_first_steps(se[:, 0], step, sr), _last_steps(se[:, 1] + tol, step, sr), cls], axis=1))
        return ragged, valid, ev_steps

    def sweep(self, out, thresholds, events=None, lengths=None, tolerance_ms: float = 1000.0, return_fired: bool = False,
              labels: Optional[Sequence[str]] = None) -> SweepResult:
        """`StreamingDetector.sweep` / `KeywordScanner.sweep`: `detection_sweep` over out's top / score with this stage's classes and
        suppression_steps, the events converted by `event_steps`."""
        ragged, valid, ev_steps = self.event_steps(out, events, lengths, tolerance_ms, labels)
        return detection_sweep(out.top, out.score, thresholds, self.det.suppression_steps, self.num_classes, ev_steps, None if ragged else valid,
                               self.step_samples / self.sample_rate, return_fired, self.lib, out.offsets if ragged else None)

    def redetect(self, out, average_window_ms: Optional[float] = None, min_count: Optional[int] = None,
                 detection_threshold: Optional[float] = None, suppression_ms: Optional[float] = None, smoothed: bool = True):
        """`KeywordScanner.redetect` over this stage's classes (None: the stage's own setting, in steps).  smoothed=False: no smoothed
        vector is written (tcr_detect_redetect takes a null pointer and launches its smoothing kernel without one) and `out.probs`
        stands in for it in the result, one tensor under both names."""
        det = self.detect_cfg(average_window_ms, min_count, detection_threshold, suppression_ms)
        lib, ncls, dev = self.lib, self.num_classes, self.device
        probs = out.probs
        self._check_tensor(probs, "redetect probs")
        ragged = isinstance(out, RaggedScanOutput)
        if not ragged and probs.dim() != 3:
            raise TcrError(f"redetect expects probs [N, steps, classes], got shape {tuple(probs.shape)}")
        sm = torch.empty_like(probs) if smoothed else None
        top, score, is_new = _new_tensors(probs.shape[:-1], ncls, dev, 0)
        tail = (ncls, probs.data_ptr(), C.byref(det), None if sm is None else sm.data_ptr(), top.data_ptr(), score.data_ptr(), is_new.data_ptr(),
                stream_of(dev))
        if ragged:
            off = torch.from_numpy(out.offsets).to(dev)
            lib.check(lib.tcr_detect_redetect_ragged(len(out), off.data_ptr(), int(probs.shape[0]), *tail), "tcr_detect_redetect_ragged")
            return RaggedScanOutput(out.logits, probs, probs if sm is None else sm, top, score, is_new, out.offsets)
        lib.check(lib.tcr_detect_redetect(int(probs.shape[0]), int(probs.shape[1]), *tail), "tcr_detect_redetect")
        return ScanOutput(out.logits, probs, probs if sm is None else sm, top, score, is_new)

    def tune(self, out, thresholds, average_window_ms: Sequence[float] = (), min_count: Sequence[int] = (),
             suppression_ms: Sequence[float] = (), events=None, lengths=None, tolerance_ms: float = 1000.0,
             labels: Optional[Sequence[str]] = None) -> GridResult:
        """`KeywordScanner.tune` over this stage's classes: the grid's points from ms to steps, the events by `event_steps`, one
        `detection_grid` call over out's probs."""
        own = self.det
        ws = [(float(w), self.detect_cfg(w, 1, 0.0, 0).average_steps) for w in average_window_ms] or [(None, own.average_steps)]
        mcs = [int(m) for m in min_count] or [own.min_count]
        sps = [(float(x), self.detect_cfg(self.step_ms, 1, 0.0, x).suppression_steps) for x in suppression_ms] or [(None, own.suppression_steps)]
        points, dropped = [], []
        for w_ms, w in ws:
            for mc in mcs:
                for s_ms, sp in sps:
                    (points if 1 <= mc <= w else dropped).append(GridPoint(w_ms, mc, s_ms, w, sp))
        if not points:
            raise TcrError(f"tune: every point of the grid has min_count above its window's steps: {[tuple(p) for p in dropped]}")
        ragged, valid, ev_steps = self.event_steps(out, events, lengths, tolerance_ms, labels)
        self._check_tensor(out.probs, "tune probs")
        res = detection_grid(out.probs, points, thresholds, self.num_classes, ev_steps, out.offsets if ragged else None,
                             None if ragged else valid, self.step_samples / self.sample_rate, self.lib)
        return GridResult(points, dropped, *res)

    def _mine_workspace(self, n: int, ranked: bool) -> Optional[torch.Tensor]:
        """The workspace of `mine`'s calls, kept between calls and replaced when one needs more."""
        if n <= 0:
            return None
        self._mine_ws = _mine_workspace("mine", self.lib, n, ranked, self.device, self._mine_ws)
        return self._mine_ws

    def mine(self, out, signals, events=None, k: int = 1000, source: str = "detections", kinds: Sequence[str] = ("false_accept",),
             classes: Optional[Sequence[int]] = None, on: str = "probs", floor: float = 0.0, radius_ms: Optional[float] = None,
             tolerance_ms: float = 1000.0, labels: Optional[Sequence[str]] = None, lead_ms: float = 0.0, pcm: bool = False) -> MinedClips:
        """`KeywordScanner.mine` over this stage's classes: `mine_detections` or `mine_peaks`, `select_top` and `gather_clips` over out's
        tensors and the packed signals, in one workspace kept between calls."""
        step, sr, ncls, dev, lib, n_samples = self.step_samples, self.sample_rate, self.num_classes, self.device, self.lib, self.clip_samples
        if source not in ("detections", "peaks"):
            raise TcrError(f"mine: source must be 'detections' or 'peaks', got {source!r}")
        kinds = [kinds] if isinstance(kinds, str) else list(kinds)
        bad = [x for x in kinds if x not in MINE_KINDS[:4]]
        if bad:
            raise TcrError(f"mine: unknown kinds {bad} (known: {list(MINE_KINDS[:4])})")
        if int(k) < 0:
            raise TcrError(f"mine: k must be >= 0 (got {k})")
        ragged, _, ev_steps = self.event_steps(out, events, None, tolerance_ms, labels)
        if ragged:
            offsets, flat = out.offsets, out
        else:
            N, steps = int(out.probs.shape[0]), int(out.probs.shape[1])
            offsets = np.arange(N + 1, dtype=np.int64) * steps
            flat = RaggedScanOutput(*(None if t is None else t.reshape(N * steps, *t.shape[2:]) for t in out), offsets)
        if not ragged and isinstance(signals, torch.Tensor) and signals.dim() == 2:
            packed, lengths = signals.reshape(-1), np.full(int(signals.shape[0]), int(signals.shape[1]), np.int64)
        else:
            packed, lengths, _ = _ragged_signals("mine", "signal", signals)
        N = len(offsets) - 1
        if lengths.size != N or (lengths != np.diff(offsets) * step).any():
            raise TcrError(f"mine: the signals' lengths {lengths.tolist()} are not the scan's ({(np.diff(offsets) * step).tolist()} samples)")
        self._check_tensor(packed, "mine samples")
        sample_off = np.zeros(N + 1, np.int64)
        np.cumsum(lengths, out=sample_off[1:])
        # the events in the order of their step ranges (`event_steps` sorts by start, then end): their times and the CSR's offsets
        ev_ms, ev_off = [], np.zeros(N + 1, np.int64)
        if events is not None:
            for n, evs in enumerate(events):
                se = np.array([(float(e[0]), float(e[1])) for e in evs], np.float64).reshape(-1, 2)
                ev_ms.append(se[np.lexsort((se[:, 1], se[:, 0]))])
                ev_off[n + 1] = ev_off[n] + len(evs)
        ev_ms = np.concatenate(ev_ms) if ev_ms else np.zeros((0, 2), np.float64)
        ev_sig = np.repeat(np.arange(N), np.diff(ev_off))
        rows = {name: [] for name in ("pstep", "label", "value", "kind", "event")}

        def add(pstep, label, value, kind, event):
            for name, x in zip(rows, (pstep, label, value, kind, event)):
                rows[name].append(np.asarray(x))

        if source == "detections":
            md = mine_detections(flat.top, flat.score, flat.is_new, offsets, ncls, ev_steps, lib, self._mine_workspace(int(offsets[-1]), False))
            want = [MINE_KINDS.index(x) for x in kinds if x != "miss"]
            kind = md.kind
            if classes is not None and want:
                keep = torch.from_numpy(_class_mask("mine", classes, ncls).astype(np.bool_)).to(dev)[md.label.long()]
                kind = torch.where(keep, kind, torch.full_like(kind, 31))
            if want and int(k) > 0:
                picked = select_top(md.value, k, kind, want, lib, self._mine_workspace(int(md.value.numel()), True))
                add(*(t[picked].cpu().numpy() for t in (md.step, md.label, md.value, md.kind, md.event)))
            if "miss" in kinds and md.event_hit is not None:
                missed = np.flatnonzero(md.event_hit.cpu().numpy() < 0)
                ev_label = np.concatenate([e[:, 2] for e in ev_steps]) if ev_steps else np.zeros(0, np.int64)
                if classes is not None:
                    missed = missed[_class_mask("mine", classes, ncls)[ev_label[missed]] != 0]
                sig = ev_sig[missed]
                last = np.minimum(_last_steps(ev_ms[missed, 1], step, sr), np.diff(offsets)[sig] - 1)
                ok = last >= 0
                add(offsets[sig[ok]] + last[ok], ev_label[missed[ok]], np.full(int(ok.sum()), np.nan, np.float32),
                    np.full(int(ok.sum()), 3, np.uint8), missed[ok])
        else:
            check_on("mine", on, ("probs", "smoothed"))
            radius = max(1, self.det.suppression_steps if radius_ms is None else ms_to_steps(radius_ms, self.step_ms))
            exclude = None
            if events is not None:
                clip_ms, exclude = 1000.0 * n_samples / sr, []
                for n in range(N):
                    se = ev_ms[ev_off[n]:ev_off[n + 1]]
                    first, last = _first_steps(se[:, 0], step, sr), np.minimum(_last_steps(se[:, 1] + clip_ms, step, sr), int(offsets[n + 1] - offsets[n]) - 1)
                    keep = last >= first
                    order = np.argsort(first[keep], kind="stable")
                    first, last = first[keep][order], last[keep][order]
                    if first.size:                  # a range opens where it does not touch the ones before it
                        reach = np.maximum.accumulate(last)
                        opens = np.flatnonzero(np.concatenate([[True], first[1:] > reach[:-1] + 1]))
                        first, last = first[opens], np.maximum.reduceat(last, opens)
                    exclude.append(np.stack([first, last], axis=1))
            cls = list(range(2, ncls)) if classes is None else [int(c) for c in classes]
            mp = mine_peaks(getattr(flat, on), offsets, floor, radius, cls, exclude, None, lib, self._mine_workspace(int(offsets[-1]) * ncls, False))
            if int(k) > 0 and mp.count > 0:
                picked = select_top(mp.value, k, lib=lib, workspace=self._mine_workspace(int(mp.value.numel()), True))
                m = int(picked.numel())
                add(mp.step[picked].cpu().numpy(), mp.label[picked].cpu().numpy(), mp.value[picked].cpu().numpy(), np.full(m, 4, np.uint8),
                    np.full(m, -1, np.int32))
        cat = lambda name, dt: np.concatenate([x.astype(dt) for x in rows[name]]) if rows[name] else np.zeros(0, dt)
        pstep, label, value = cat("pstep", np.int64), cat("label", np.int32), cat("value", np.float32)
        kind, event = cat("kind", np.uint8), cat("event", np.int32)
        signal = (np.searchsorted(offsets, pstep, side="right") - 1).astype(np.int32)
        i = pstep - offsets[signal]
        lead = int(round(float(lead_ms) * sr / 1000.0))
        first = (i + 1) * step + lead - n_samples
        clips, pcm16 = gather_clips(packed, sample_off, signal, first.astype(np.int64), n_samples, True, bool(pcm), lib)
        start_ms = np.where(event >= 0, ev_ms[np.maximum(event, 0), 0] if len(ev_ms) else np.nan, np.nan) if len(event) else np.zeros(0)
        return MinedClips(clips, pcm16, signal, i, _step_ms(i, step, sr), label, value, kind, event, np.asarray(start_ms, np.float64), lib, sr)
