"""Mining hard examples from a scan's outputs on the device, over raw tensors (tcr_mine_*): `mine_detections` classifies the detections
against labelled events by the sweep's rule, `mine_peaks` finds the near misses, `select_top` keeps the best k, `gather_clips` cuts
their audio; `MinedClips` is what `detection.DetectionStage.mine` (`KeywordScanner.mine`) makes of them."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TcrError
from .runtime import stream_of
from .scoring import _class_mask, _offsets, _pack_events

MINE_KINDS = ("false_accept", "hit", "duplicate", "miss", "peak")      # `MinedClips.kind` codes; the first three are tcr_mine_detections'


def _mine_workspace(what: str, lib, n: int, ranked: bool, dev, have: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 tensor of tcr_mine_workspace_bytes(n, ranked); `have` when that is one and large enough."""
    nws = lib.tcr_mine_workspace_bytes(n, int(ranked))
    if nws == 0:
        raise TcrError(f"{what}: {lib.tcr_last_error().decode()}")
    if have is not None and have.dtype == torch.int32 and have.device == dev and have.numel() * 4 >= nws:
        return have
    return torch.empty((nws + 3) // 4, dtype=torch.int32, device=dev)


class MinedDetections(NamedTuple):
    """tcr_mine_detections' tables, on the device, one row per candidate in increasing packed step: step int64, label int32, value
    float32 (the score), kind uint8 (0 false accept, 1 hit, 2 duplicate), event int32 (the covering event's index in the signals'
    sorted events one after the other, -1: none); event_hit int64 [events] (the packed step that hit the event, -1: a miss; None
    without events)."""
    step: torch.Tensor
    label: torch.Tensor
    value: torch.Tensor
    kind: torch.Tensor
    event: torch.Tensor
    event_hit: Optional[torch.Tensor]


def mine_detections(top: torch.Tensor, score: torch.Tensor, is_new: torch.Tensor, offsets, num_classes: int,
                    events: Optional[Sequence[Sequence[Tuple[int, int, int]]]] = None, lib=None,
                    workspace: Optional[torch.Tensor] = None) -> MinedDetections:
    """The raw form of tcr_mine_detections: the detections of packed top / score / is_new [total_steps] (a ragged scan's or a
    redetect's; offsets host int64 [N + 1] in steps) classified against events (`detection_sweep`'s: per signal inclusive step ranges
    (first, last, label), disjoint).  The rule is the sweep's; see `MinedDetections`.  Reads one integer back (the number of
    candidates), so the call waits for the device."""
    lib = _lib.get() if lib is None else lib
    if top.dim() != 1 or score.shape != top.shape or is_new.shape != top.shape:
        raise TcrError(f"mine_detections expects packed top, score and is_new [total_steps], got {tuple(top.shape)}, {tuple(score.shape)} "
                       f"and {tuple(is_new.shape)}")
    if top.dtype != torch.int32 or is_new.dtype != torch.int32 or score.dtype != torch.float32 or \
            not (top.is_contiguous() and score.is_contiguous() and is_new.is_contiguous()):
        raise TcrError("mine_detections expects contiguous int32 top, float32 score and int32 is_new")
    total, ncls, dev = int(top.shape[0]), int(num_classes), top.device
    soff = _offsets("mine_detections", "offsets", offsets, total, int64_only=True)
    N = int(soff.size) - 1
    _, ev_args, keep = _pack_events(events, N, ncls, dev)
    n_events = int(keep[0][-1].item()) if keep else 0
    i64 = dict(dtype=torch.int64, device=dev)
    step, label = torch.empty(total, **i64), torch.empty(total, dtype=torch.int32, device=dev)
    value, kind = torch.empty(total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    event, count = torch.empty(total, dtype=torch.int32, device=dev), torch.zeros(1, **i64)
    hit = torch.empty(max(n_events, 1), **i64) if keep else None
    n = 0
    if total > 0:
        ws = _mine_workspace("mine_detections", lib, total, False, dev, workspace)
        off_dev = torch.from_numpy(soff).to(dev)
        lib.check(lib.tcr_mine_detections(N, off_dev.data_ptr(), total, ncls, top.data_ptr(), score.data_ptr(), is_new.data_ptr(), *ev_args,
                                          n_events, ws.data_ptr(), ws.numel() * 4, step.data_ptr(), label.data_ptr(), value.data_ptr(),
                                          kind.data_ptr(), event.data_ptr(), count.data_ptr(), None if hit is None else hit.data_ptr(),
                                          stream_of(dev)), "tcr_mine_detections")
        n = int(count.item())
    elif hit is not None:
        hit.fill_(-1)
    return MinedDetections(step[:n], label[:n], value[:n], kind[:n], event[:n], None if hit is None else hit[:n_events])


class MinedPeaks(NamedTuple):
    """tcr_mine_peaks' tables, on the device, in (packed step, class) order: step int64, label int32, value float32 -- the first
    `capacity` candidates; count: how many there are in all."""
    step: torch.Tensor
    label: torch.Tensor
    value: torch.Tensor
    count: int


def mine_peaks(values: torch.Tensor, offsets, floor: float, radius: int, classes: Sequence[int],
               exclude: Optional[Sequence[Sequence[Tuple[int, int]]]] = None, capacity: Optional[int] = None, lib=None,
               workspace: Optional[torch.Tensor] = None) -> MinedPeaks:
    """The raw form of tcr_mine_peaks: the local maxima of values [total_steps, C] (float32 on the device: a ragged scan's probs or
    smoothed; offsets host int64 [N + 1] in steps) over the classes `classes`: values[p, c] >= floor, above every value of its class
    in the `radius` steps of its signal before it, at or above those in the `radius` steps after it (NaNs ignored), outside `exclude`
    (per signal, inclusive step ranges (first, last), sorted and disjoint).  capacity: the rows stored (None: all of them; a second
    call only when there are more than 2^24).  Reads the count back, so the call waits for the device."""
    lib = _lib.get() if lib is None else lib
    if values.dim() != 2 or values.dtype != torch.float32 or not values.is_contiguous():
        raise TcrError(f"mine_peaks expects contiguous float32 values [total_steps, classes], got {values.dtype} {tuple(values.shape)}")
    total, ncls, dev = int(values.shape[0]), int(values.shape[1]), values.device
    soff = _offsets("mine_peaks", "offsets", offsets, total, int64_only=True)
    N = int(soff.size) - 1
    cmask = _class_mask("mine_peaks", classes, ncls)
    ex_args, keep = [None, None, None], []
    if exclude is not None:
        if len(exclude) != N:
            raise TcrError(f"mine_peaks: exclusion ranges for {len(exclude)} signals, the scan has {N}")
        off, rows = np.zeros(N + 1, np.int32), []
        for n, ranges in enumerate(exclude):
            a = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
            if (a[:, 1] < a[:, 0]).any() or (a[1:, 0] <= a[:-1, 1]).any():
                raise TcrError(f"mine_peaks: signal {n}: the exclusion ranges are not sorted and disjoint: {a.tolist()}")
            rows.append(a)
            off[n + 1] = off[n] + len(a)
        a = np.concatenate(rows + [np.zeros((1, 2), np.int64)])
        keep = [torch.from_numpy(x).to(dev) for x in (off, np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]))]
        ex_args = [t.data_ptr() for t in keep]
    empty = MinedPeaks(torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                       torch.empty(0, dtype=torch.float32, device=dev), 0)
    if total == 0:
        return empty
    ws = _mine_workspace("mine_peaks", lib, total * ncls, False, dev, workspace)
    off_dev, cmask_dev = torch.from_numpy(soff).to(dev), torch.from_numpy(cmask).to(dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    # (two peaks of a class and signal are more than `radius` steps apart: the first try holds them all unless that is past 2^24 rows)
    bound = (total // (max(int(radius), 1) + 1) + N) * max(int(cmask.sum()), 1)
    cap = min(total * ncls, bound, 1 << 24) if capacity is None else int(capacity)
    while True:
        room = max(cap, 1)
        step, label = torch.empty(room, dtype=torch.int64, device=dev), torch.empty(room, dtype=torch.int32, device=dev)
        value = torch.empty(room, dtype=torch.float32, device=dev)
        lib.check(lib.tcr_mine_peaks(N, off_dev.data_ptr(), total, ncls, values.data_ptr(), cmask_dev.data_ptr(), float(floor), int(radius),
                                     *ex_args, ws.data_ptr(), ws.numel() * 4, cap, step.data_ptr(), label.data_ptr(), value.data_ptr(),
                                     count.data_ptr(), stream_of(dev)), "tcr_mine_peaks")
        n = int(count.item())
        if capacity is not None or n <= cap:
            break
        cap = n
    m = min(n, cap)
    return MinedPeaks(step[:m], label[:m], value[:m], n)


def select_top(value: torch.Tensor, k: int, kind: Optional[torch.Tensor] = None, kinds: Sequence[int] = (), lib=None,
               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw form of tcr_mine_select: the indices (int64 on the device, increasing) of the k best of value [n] (float32 on the
    device): the larger value first, -0 equal to +0, then the lower index.  kind (uint8 [n]) with kinds: only candidates whose kind
    is one of `kinds` are eligible.  Exact, no sort.  Reads the number picked back, so the call waits for the device."""
    lib = _lib.get() if lib is None else lib
    if value.dim() != 1 or value.dtype != torch.float32 or not value.is_contiguous():
        raise TcrError(f"select_top expects contiguous float32 values [n], got {value.dtype} {tuple(value.shape)}")
    n, dev = int(value.shape[0]), value.device
    mask = 0
    if kind is not None:
        if kind.dtype != torch.uint8 or tuple(kind.shape) != (n,) or not kind.is_contiguous():
            raise TcrError(f"select_top expects contiguous uint8 kinds [{n}], got {kind.dtype} {tuple(kind.shape)}")
        for c in kinds:
            if not 0 <= int(c) < 32:
                raise TcrError(f"select_top: kind {c} outside 0..31")
            mask |= 1 << int(c)
    k = int(k)
    room = max(min(k, n), 1)
    picked, count = torch.empty(room, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _mine_workspace("select_top", lib, n, True, dev, workspace) if n > 0 and k > 0 else None
    lib.check(lib.tcr_mine_select(n, value.data_ptr(), None if kind is None else kind.data_ptr(), mask, k,
                                  None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, picked.data_ptr(),
                                  count.data_ptr(), stream_of(dev)), "tcr_mine_select")
    return picked[:int(count.item())]


def _index_arg(what: str, name: str, x, dtype, dev) -> torch.Tensor:
    want = {torch.int32: np.int32, torch.int64: np.int64}[dtype]
    if isinstance(x, torch.Tensor):
        if x.dtype != dtype:
            raise TcrError(f"{what} expects {str(dtype).split('.')[-1]} {name}, got {str(x.dtype).split('.')[-1]}")
        return x.to(dev).contiguous().reshape(-1)
    a = np.asarray(x)
    if a.dtype != want:
        raise TcrError(f"{what} expects {np.dtype(want).name} {name}, got {a.dtype}")
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1))).to(dev)


def gather_clips(samples: torch.Tensor, sample_offsets, clip_signal, clip_first, n_samples: int, floats: bool = True, pcm: bool = False,
                 lib=None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The raw form of tcr_mine_gather: clip i = n_samples samples of signal clip_signal[i] (int32) from its sample clip_first[i]
    (int64, relative to the signal's start; negative or past the end: zeros there) of the packed float32 `samples` (sample_offsets:
    int64 [N + 1]).  Returns (float32 [n, n_samples] bitwise the samples or None, int16 [n, n_samples] or None) on the device; the
    int16 rows are clamp(rint(x * 32768), -32768, 32767), which inverts the int16 decode."""
    lib = _lib.get() if lib is None else lib
    if samples.dim() != 1 or samples.dtype != torch.float32 or not samples.is_contiguous():
        raise TcrError(f"gather_clips expects contiguous packed float32 samples, got {samples.dtype} {tuple(samples.shape)}")
    dev = samples.device
    soff = _offsets("gather_clips", "offsets", sample_offsets, int(samples.shape[0]), int64_only=True)
    sig, first = _index_arg("gather_clips", "clip_signal", clip_signal, torch.int32, dev), \
        _index_arg("gather_clips", "clip_first", clip_first, torch.int64, dev)
    n = int(sig.shape[0])
    if int(first.shape[0]) != n:
        raise TcrError(f"gather_clips: {n} clip_signal for {int(first.shape[0])} clip_first")
    m = int(n_samples)
    out = torch.empty((n, max(m, 0)), dtype=torch.float32, device=dev) if floats else None
    out_pcm = torch.empty((n, max(m, 0)), dtype=torch.int16, device=dev) if pcm else None
    if n == 0:                  # (nothing to launch; an empty tensor has no address to pass)
        return out, out_pcm
    off_dev = torch.from_numpy(soff).to(dev)
    lib.check(lib.tcr_mine_gather(int(soff.size) - 1, off_dev.data_ptr(), samples.data_ptr(), n, sig.data_ptr(), first.data_ptr(), m,
                                  None if out is None else out.data_ptr(), None if out_pcm is None else out_pcm.data_ptr(),
                                  stream_of(dev)), "tcr_mine_gather")
    return out, out_pcm


class MinedClips:
    """What `KeywordScanner.mine` returns.  clips float32 [n, n_samples] on the device (bitwise the signals' samples, zeros outside
    them), pcm int16 [n, n_samples] on the device or None; host arrays, one entry per clip: signal, step (within the signal), time_ms
    (the end of the step's window, `sweep`'s stamp), label (the detection's or peak's class; a miss: the event's), value (the score
    or peak value; NaN for a miss), kind (an index into `MINE_KINDS`), event (the index of the covering / missed event among the
    signals' events sorted by start, one signal after the other; -1: none) and event_start_ms (NaN: none)."""

    def __init__(self, clips, pcm, signal, step, time_ms, label, value, kind, event, event_start_ms, lib, sample_rate: int):
        self.clips, self.pcm = clips, pcm
        self.signal, self.step, self.time_ms, self.label, self.value = signal, step, time_ms, label, value
        self.kind, self.event, self.event_start_ms = kind, event, event_start_ms
        self.lib, self.sample_rate = lib, sample_rate

    def __len__(self) -> int:
        return int(self.signal.size)

    def kind_names(self) -> Sequence[str]:
        return [MINE_KINDS[k] for k in self.kind]

    def to_pool(self, device=None):
        """The clips as the training input stage's int16 pool (`datasets.augmentation_factory.PcmPool`: one device tensor and
        offsets), without a trip through the host; needs `mine(..., pcm=True)`."""
        from .datasets.augmentation_factory import PcmPool
        if self.pcm is None:
            raise TcrError("MinedClips.to_pool: the clips were mined without pcm=True")
        n, m = int(self.pcm.shape[0]), int(self.pcm.shape[1])
        pool = PcmPool.__new__(PcmPool)
        pool.lib, pool.device = self.lib, self.pcm.device if device is None else torch.device(device)
        pool.lengths = np.full(n, m, np.int64)
        pool.offsets = np.arange(n, dtype=np.int64) * m
        pool.data = self.pcm.reshape(-1).to(pool.device) if n else torch.zeros(1, dtype=torch.int16, device=pool.device)
        return pool

