"""Scoring detections against labelled events on the device, over raw tensors: `detection_sweep` (tcr_detect_sweep: the suppression rule
for many thresholds at once, counted into a `SweepResult`, a DET curve) and `detection_grid` (tcr_detect_grid: the same for a grid of
detector settings from a scan's probs, a `GridResult`), and the argument checks that every raw-tensor function of the detection modules
shares: packed offsets, valid steps, class masks, thresholds, the events' CSR form.  `detection.DetectionStage` takes events in ms."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TcrError
from .runtime import stream_of


# ---- detection sweeps ------------------------------------------------------------------------------------------------------------
class SweepResult(NamedTuple):
    """Results of a detection sweep (tcr_detect_sweep) over N signals, T thresholds and C classes.

    detections / hits / duplicates [N, T, C] int32 on the device, per detection label (hits / duplicates are zero without events);
    fired [T, N, steps] uint8 on the device ([T, total_steps] for a ragged scan) or None (1 at the steps that fire at thresholds[t]);
    thresholds [T] float32 (host);
    events [N, C] int64 (host): the labelled events per signal and label; hours [N] float64 (host): each signal's valid steps in
    hours (NaN when the step length is unknown)."""
    detections: torch.Tensor
    hits: torch.Tensor
    duplicates: torch.Tensor
    fired: Optional[torch.Tensor]
    thresholds: np.ndarray
    events: np.ndarray
    hours: np.ndarray

    def false_accepts(self) -> torch.Tensor:
        """[N, T, C] int32: detections that hit no event of their label for the first time or again."""
        return self.detections - self.hits - self.duplicates

    def curve(self, classes: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
        """The DET curve over every signal and the chosen classes (default: all), one entry per threshold: threshold, hits,
        events, false_accepts, duplicates, frr = 1 - hits / events (NaN without events), fa_per_hour = false_accepts / hours."""
        cls = list(range(self.detections.shape[2])) if classes is None else [int(c) for c in classes]
        det = self.detections.cpu().numpy().astype(np.int64)[:, :, cls].sum(axis=(0, 2))
        hits = self.hits.cpu().numpy().astype(np.int64)[:, :, cls].sum(axis=(0, 2))
        dup = self.duplicates.cpu().numpy().astype(np.int64)[:, :, cls].sum(axis=(0, 2))
        events = int(self.events[:, cls].sum())
        fa = det - hits - dup
        hours = float(self.hours.sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            frr = 1.0 - hits / events if events > 0 else np.full(len(hits), np.nan)
            fa_h = fa / hours if hours > 0 else np.full(len(fa), np.nan)
        return {"threshold": self.thresholds.astype(np.float64), "hits": hits, "events": np.full(len(hits), events, np.int64),
                "false_accepts": fa, "duplicates": dup, "frr": np.asarray(frr, np.float64), "fa_per_hour": np.asarray(fa_h, np.float64)}

    def operating_point(self, max_fa_per_hour: float, classes: Optional[Sequence[int]] = None) -> Optional[Dict[str, float]]:
        """The threshold of the lowest FRR among those with fa_per_hour <= max_fa_per_hour (ties: fewer false accepts per hour,
        then the higher threshold), as {threshold, frr, fa_per_hour, hits, events, false_accepts}; None when none is in budget."""
        cv = self.curve(classes)
        best = None
        for t in range(len(cv["threshold"])):
            if not cv["fa_per_hour"][t] <= max_fa_per_hour:
                continue
            frr = cv["frr"][t]
            key = (0.0 if np.isnan(frr) else frr, cv["fa_per_hour"][t], -cv["threshold"][t])
            if best is None or key < best[0]:
                best = (key, t)
        if best is None:
            return None
        t = best[1]
        return {"threshold": float(cv["threshold"][t]), "frr": float(cv["frr"][t]), "fa_per_hour": float(cv["fa_per_hour"][t]),
                "hits": int(cv["hits"][t]), "events": int(cv["events"][t]), "false_accepts": int(cv["false_accepts"][t])}


def _thresholds(thresholds) -> np.ndarray:
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1).astype(np.float32))
    if thr.size == 0:
        raise TcrError("detection sweep: no thresholds")
    if np.isnan(thr).any():
        raise TcrError(f"detection sweep: NaN thresholds at positions {np.flatnonzero(np.isnan(thr)).tolist()}")
    return thr


def _offsets(what: str, noun: str, offsets, total: int, end: str = "{}", int64_only: bool = False) -> np.ndarray:
    """`what`'s `noun` (the offsets of N packed signals, [N + 1]) as a host int64 array, checked: from 0 to `total` without decreasing.
    int64_only: a tensor is taken too, and any other integer type is refused, not converted."""
    if int64_only:
        if isinstance(offsets, torch.Tensor):
            if offsets.dtype != torch.int64:
                raise TcrError(f"{what} expects int64 {noun}, got {offsets.dtype}")
            offsets = offsets.detach().cpu().numpy()
        if np.asarray(offsets).dtype != np.int64:
            raise TcrError(f"{what} expects int64 {noun}, got {np.asarray(offsets).dtype}")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if off.size < 2 or off[0] != 0 or (np.diff(off) < 0).any() or int(off[-1]) != total:
        raise TcrError(f"{what}: {noun} must run from 0 to {end.format(total)} without decreasing")
    return off


def _signal_steps(what: str, step_offsets, valid_steps, N: int, steps: int, total: int):
    """The signals of `what`'s rows -> (the packed form's step_offsets, host int64, or None; every signal's steps that count, host int64),
    checked: dense [N, steps] rows with valid_steps (None: all of them), or `total` packed rows with step_offsets."""
    if step_offsets is not None:
        if valid_steps is not None:
            raise TcrError(f"{what}: valid_steps with step_offsets (a ragged scan's offsets are its signals' lengths)")
        soff = _offsets(what, "step_offsets", step_offsets, total, "the {} packed steps")
        return soff, np.diff(soff)
    vs = np.full(N, steps, np.int64) if valid_steps is None else np.asarray(valid_steps, np.int64).reshape(-1)
    if vs.shape != (N,):
        raise TcrError(f"{what}: {vs.size} valid_steps for {N} signals")
    if (vs < 0).any() or (vs > steps).any():
        raise TcrError(f"{what}: valid_steps outside 0..{steps}: {vs.tolist()}")
    return None, vs


def _class_mask(what: str, classes, ncls: int) -> np.ndarray:
    cls = np.asarray(list(classes), dtype=np.int64).reshape(-1)
    if cls.size and (cls.min() < 0 or cls.max() >= ncls):
        raise TcrError(f"{what}: classes outside 0..{ncls - 1}: {cls.tolist()}")
    mask = np.zeros(max(ncls, 1), np.uint8)
    mask[cls] = 1
    return mask


def _pack_events(events, N: int, ncls: int, dev):
    """events (per signal, inclusive step ranges (first, last, label)) -> (the events per signal and label [N, ncls] int64, the four
    CSR device pointers of the C calls (None without events), the tensors that own them)."""
    counts = np.zeros((N, ncls), np.int64)
    if events is None:
        return counts, [None, None, None, None], []
    if len(events) != N:
        raise TcrError(f"detection sweep: events for {len(events)} signals, the scan has {N}")
    off, rows = np.zeros(N + 1, np.int32), []
    for n, evs in enumerate(events):
        a = np.asarray(evs, dtype=np.int64).reshape(-1, 3)
        a = a[np.lexsort((a[:, 1], a[:, 0]))]
        bad = np.flatnonzero((a[:, 2] < 0) | (a[:, 2] >= ncls))
        if bad.size:
            raise TcrError(f"detection sweep: signal {n}: event {tuple(a[bad[0]].tolist())} has an unknown label "
                           f"(classes 0..{ncls - 1})")
        ov = np.flatnonzero(a[1:, 0] <= a[:-1, 1])
        if ov.size:
            raise TcrError(f"detection sweep: signal {n}: events {tuple(a[ov[0]].tolist())} and {tuple(a[ov[0] + 1].tolist())} overlap")
        counts[n] = np.bincount(a[:, 2], minlength=ncls)
        rows.append(a)
        off[n + 1] = off[n] + len(a)
    a = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
    if len(a) == 0:
        a = np.zeros((1, 3), np.int64)              # (never read: every signal's range is empty)
    host = [off, np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), np.ascontiguousarray(a[:, 2].astype(np.int32))]
    keep = [torch.from_numpy(x).to(dev) for x in host]
    return counts, [t.data_ptr() for t in keep], keep


def detection_sweep(top: torch.Tensor, score: torch.Tensor, thresholds, suppression_steps: int, num_classes: int,
                    events: Optional[Sequence[Sequence[Tuple[int, int, int]]]] = None, valid_steps=None,
                    step_seconds: Optional[float] = None, return_fired: bool = False, lib=None, step_offsets=None) -> SweepResult:
    """The streaming detector's suppression rule (include/tcresnet_hip.h, tcr_detect_sweep) for every threshold at once, over top
    int32 / score float32 [N, steps] on the device (a scan's, or streaming outputs stacked over steps), scored against events.

    events: per signal, a list of (first_step, last_step, label) or an integer array [E, 3] of them (no conversion then): inclusive
    step ranges, disjoint within a signal (checked);
    valid_steps: per signal, the steps that count (None: all); step_seconds: one step's duration, for SweepResult.hours.

    step_offsets (host int64 [N + 1], from 0, non-decreasing): the ragged form (tcr_detect_sweep_ragged) -- top / score are packed
    [total_steps], signal n's steps are rows step_offsets[n] .. step_offsets[n + 1] - 1, events are in steps relative to the signal's
    first, fired is [T, total_steps]; valid_steps is refused (the offsets are the lengths)."""
    lib = _lib.get() if lib is None else lib
    ragged = step_offsets is not None
    if top.dim() != (1 if ragged else 2) or score.shape != top.shape:
        want = "with step_offsets expects packed top and score [total_steps]" if ragged else "expects top and score [N, steps]"
        raise TcrError(f"detection sweep {want}, got {tuple(top.shape)} and {tuple(score.shape)}")
    soff, vs = _signal_steps("detection sweep", step_offsets, valid_steps, int(top.shape[0]), int(top.shape[-1]), int(top.shape[0]))
    if top.dtype != torch.int32 or score.dtype != torch.float32 or not top.is_contiguous() or not score.is_contiguous():
        raise TcrError("detection sweep expects contiguous int32 top and float32 score")
    if top.device != score.device:
        raise TcrError("detection sweep: top and score are on different devices")
    dev = top.device
    N, steps, ncls = int(vs.size), int(top.shape[-1]), int(num_classes)
    thr = _thresholds(thresholds)
    T = int(thr.size)
    i32 = dict(dtype=torch.int32, device=dev)
    detections = torch.empty((N, T, ncls), **i32)
    hits = torch.zeros((N, T, ncls), **i32)
    dups = torch.zeros((N, T, ncls), **i32)
    fired = torch.empty((T, steps) if ragged else (T, N, steps), dtype=torch.uint8, device=dev) if return_fired else None
    counts, ev_args, keep = _pack_events(events, N, ncls, dev)
    thr_dev = torch.from_numpy(thr).to(dev)
    hours = vs * float(step_seconds) / 3600.0 if step_seconds is not None else np.full(N, np.nan)
    tail = (int(suppression_steps), T, thr_dev.data_ptr(), *ev_args, detections.data_ptr(), hits.data_ptr(), dups.data_ptr(),
            None if fired is None else fired.data_ptr(), stream_of(dev))
    steps_dev = torch.from_numpy(soff if ragged else vs).to(dev)
    if ragged:
        lib.check(lib.tcr_detect_sweep_ragged(N, steps_dev.data_ptr(), ncls, top.data_ptr(), score.data_ptr(), *tail), "tcr_detect_sweep_ragged")
    else:
        lib.check(lib.tcr_detect_sweep(N, steps, ncls, top.data_ptr(), score.data_ptr(), steps_dev.data_ptr(), *tail), "tcr_detect_sweep")
    return SweepResult(detections, hits, dups, fired, thr, counts, hours)


# ---- detector tuning -------------------------------------------------------------------------------------------------------------
class GridPoint(NamedTuple):
    """One point of a detector grid: the settings as given and in steps."""
    average_window_ms: Optional[float]
    min_count: int
    suppression_ms: Optional[float]
    average_steps: int
    suppression_steps: int

    @property
    def steps(self) -> Tuple[int, int, int]:
        """(average_steps, min_count, suppression_steps): tcr_detect_point."""
        return self.average_steps, self.min_count, self.suppression_steps


class GridResult:
    """Results of a detector grid (tcr_detect_grid) over J points, N signals, T thresholds and C classes.

    points: the J `GridPoint`s in grid order; dropped: the combinations left out (min_count > average_steps), as `GridPoint`s;
    detections / hits / duplicates [J, N, T, C] int32 on the device; thresholds, events, hours: `SweepResult`'s.
    `result(j)` is point j's `SweepResult` (views; fired is None), so `curve` and `operating_point` apply to it unchanged."""

    def __init__(self, points, dropped, detections, hits, duplicates, thresholds, events, hours):
        self.points, self.dropped = list(points), list(dropped)
        self.detections, self.hits, self.duplicates = detections, hits, duplicates
        self.thresholds, self.events, self.hours = thresholds, events, hours

    def __len__(self) -> int:
        return len(self.points)

    def result(self, j: int) -> SweepResult:
        if not 0 <= j < len(self):
            raise IndexError(f"point {j} of {len(self)}")
        return SweepResult(self.detections[j], self.hits[j], self.duplicates[j], None, self.thresholds, self.events, self.hours)

    def best(self, max_fa_per_hour: float, classes: Optional[Sequence[int]] = None) -> Optional[Dict]:
        """The point and threshold of the lowest FRR with fa_per_hour <= max_fa_per_hour (ties: fewer false accepts per hour, then
        grid order; within a point, `SweepResult.operating_point`'s rule): {"index": j, "point": points[j], **operating point}, or
        None when no point has a threshold in budget."""
        best = None
        for j in range(len(self)):
            op = self.result(j).operating_point(max_fa_per_hour, classes)
            if op is None:
                continue
            key = (0.0 if np.isnan(op["frr"]) else op["frr"], op["fa_per_hour"])
            if best is None or key < best[0]:
                best = (key, j, op)
        if best is None:
            return None
        return {"index": best[1], "point": self.points[best[1]], **best[2]}


def detection_grid(probs: torch.Tensor, points, thresholds, num_classes: int,
                   events: Optional[Sequence[Sequence[Tuple[int, int, int]]]] = None, step_offsets=None, valid_steps=None,
                   step_seconds: Optional[float] = None, lib=None, workspace_bytes: Optional[int] = None):
    """tcr_detect_grid over a scan's probs (float32 on the device, [N, steps, C]; with step_offsets (host int64 [N + 1]) packed
    [total_steps, C]): for every point (average_steps, min_count, suppression_steps) the counts of `detection_sweep` over the top /
    score a scan with those settings returns.  thresholds, events (in steps), valid_steps, step_seconds: `detection_sweep`'s.
    workspace_bytes: the bytes to run in (None: enough for every pair at once; fewer run the pairs in batches).
    Returns (detections, hits, duplicates [J, N, T, C] int32 on the device, thresholds, events [N, C], hours [N])."""
    lib = _lib.get() if lib is None else lib
    ragged = step_offsets is not None
    ncls = int(num_classes)
    if probs.dtype != torch.float32 or not probs.is_contiguous():
        raise TcrError("detection grid expects contiguous float32 probs")
    if probs.dim() != (2 if ragged else 3) or int(probs.shape[-1]) != ncls:
        want = f"with step_offsets expects packed probs [total_steps, {ncls}]" if ragged else f"expects probs [N, steps, {ncls}]"
        raise TcrError(f"detection grid {want}, got {tuple(probs.shape)}")
    steps = 0 if ragged else int(probs.shape[1])
    total = int(probs.shape[0]) * (1 if ragged else steps)
    soff, vs = _signal_steps("detection grid", step_offsets, valid_steps, int(probs.shape[0]), steps, total)
    N = int(vs.size)
    pts = [tuple(int(v) for v in (p.steps if isinstance(p, GridPoint) else p)) for p in points]
    J = len(pts)
    arr = (_lib.DetectPoint * max(J, 1))(*(_lib.DetectPoint(*p) for p in pts))
    thr = _thresholds(thresholds)
    T = int(thr.size)
    dev = probs.device
    counts, ev_args, keep = _pack_events(events, N, ncls, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    detections, hits, dups = (torch.zeros((J, N, T, ncls), **i32) for _ in range(3))
    nws = lib.tcr_detect_grid_workspace_bytes(total, max(J, 1)) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(nws, 4) // 4 + 1, dtype=torch.int32, device=dev)
    thr_dev = torch.from_numpy(thr).to(dev)
    off_dev = torch.from_numpy(soff).to(dev) if ragged else None
    vs_dev = None if ragged else torch.from_numpy(vs).to(dev)
    stream = stream_of(dev)
    lib.check(lib.tcr_detect_grid(N, steps, None if off_dev is None else off_dev.data_ptr(), total, ncls, probs.data_ptr(),
                                  None if vs_dev is None else vs_dev.data_ptr(), J, arr, T, thr_dev.data_ptr(), *ev_args,
                                  detections.data_ptr(), hits.data_ptr(), dups.data_ptr(), ws.data_ptr(), nws, stream), "tcr_detect_grid")
    hours = vs * float(step_seconds) / 3600.0 if step_seconds is not None else np.full(N, np.nan)
    return detections, hits, dups, thr, counts, hours

