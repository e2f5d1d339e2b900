"""Offline keyword scanning of long recordings, on the device (tcr_scan of include/tcresnet_hip.h).

A `KeywordScanner` takes a batch of N signals of equal length and returns, for every signal and every step, exactly what a fresh
`streaming.StreamingDetector` with the same settings returns from its (i + 1)-th `push` when fed that signal k * hop samples at a
time: logits, probs, smoothed, top, score and is_new, bitwise.  One call computes every window at the network's batch throughput;
only the suppression rule runs in step order, over the candidate steps.

`KeywordScanner.scan_ragged` takes signals of different lengths in one call (tcr_scan_ragged): packed one after the other, each
signal's rows bitwise its own `scan`, no padding computed, stored or detected in.

`KeywordScanner.sweep` (and `detection_sweep` over raw top / score tensors) then runs that rule for many thresholds at once on the
device and scores the detections against labelled keyword events: a DET curve (false rejects against false accepts per hour) for
the cost of one scan and a pass over its top / score.

`KeywordScanner.scan_steps` computes a chosen subset of a ragged scan's steps at the cost of that subset (tcr_scan_steps),
`select_steps` picks the steps around a first model's flags (tcr_scan_select), and a `CascadeScanner` puts the two together: a cheap
scanner looks at everything, an expensive one only where the cheap one flagged, and the detector runs on the merged posteriors.

`KeywordScanner.mine` collects the audio a scan got wrong, for retraining: the windows that fired outside any event, the events never
hit, the windows that came close (`mine_detections`, `mine_peaks`, `select_top`, `gather_clips` over raw tensors: tcr_mine_*), as
`MinedClips` whose `to_pool()` is the int16 clip pool the training input stage takes.

A `PhraseDetector` scores multi-word phrases from a scan's posteriors (tcr_phrase_scores): posteriors over the phrases and a background
class, on which the detector rule, `sweep`, `tune` and `mine` run with P + 1 classes.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterator, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TcrError
from .engine import Frontend
from .streaming import Network, _Detection, _ragged_scan_output, _ragged_signals, _scan_output, ms_to_steps

DEFAULT_MAX_WINDOWS = 4096
DEFAULT_MAX_SIGNALS = 65536


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


class KeywordScanner(_Detection):
    """Scans signals through `frontend` and `net` (a TCResNet, DSCNN or finalized Graph2D) with the streaming detector's settings
    (see `streaming.StreamingDetector`: the same arguments, the same ms -> steps conversion, the same weight and fold rules).  Step i of a signal is its window after
    (i + 1) * k * hop samples of audio, with one clip of silence in front.

    max_windows bounds the windows the network runs per launch (default 4096); the workspace, allocated once here, is sized by it
    and not by the signals' length.  max_signals (default 65536) sizes the offset tables of `scan_ragged`'s workspace, which is
    allocated on its first call and again when a call brings more signals; `scan_steps` has a workspace of its own, sized by the
    signals and selected steps of the largest call so far."""

    def __init__(self, net: Network, frontend: Frontend, frames_per_step: int = 1, average_window_ms: float = 1000,
                 min_count: int = 3, detection_threshold: float = 0.5, suppression_ms: float = 1500,
                 frozen_ss: Optional[torch.Tensor] = None, max_windows: Optional[int] = None, max_signals: Optional[int] = None):
        self._setup("KeywordScanner", "scanner", net, frontend, frames_per_step, average_window_ms, min_count, detection_threshold,
                    suppression_ms)
        self.max_windows = DEFAULT_MAX_WINDOWS if max_windows is None else int(max_windows)
        self.max_signals = DEFAULT_MAX_SIGNALS if max_signals is None else int(max_signals)
        if self.max_signals < 1:
            raise TcrError(f"KeywordScanner: max_signals must be >= 1 (got {self.max_signals})")
        self._ragged_ws: Optional[torch.Tensor] = None
        self._steps_ws: Optional[torch.Tensor] = None
        self._steps_ws_size = (0, 0)            # the signals and selected steps `_steps_ws` holds tables for
        lib, cfg = self.lib, frontend.cfg
        nws = lib.tcr_scan_workspace_bytes_m(C.byref(cfg), C.byref(self._ref()), self.k, self.max_windows)
        if nws == 0:
            raise TcrError(f"KeywordScanner: {lib.tcr_last_error().decode()}")
        self._bind_frozen(frozen_ss)
        self.workspace = torch.empty(nws // 4, dtype=torch.float32, device=self.device)

    def scan(self, samples: torch.Tensor) -> ScanOutput:
        """samples [N, L] float32 on the device, L a multiple of k * hop -> ScanOutput with L / (k * hop) steps per signal (new tensors).
        TC-ResNet: refolds BN first when the net's weights changed (without `frozen_ss`); with `frozen_ss`, raises once the conv / fc arena
        changed since construction."""
        if samples.dim() != 2:
            raise TcrError(f"scan expects samples [N, L], got shape {tuple(samples.shape)}")
        self.net._check_tensor(samples, "scan samples")
        N, L = int(samples.shape[0]), int(samples.shape[1])        # (tcr_scan refuses N <= 0 and L not a multiple of k * hop)
        ref = self._call_ref()
        out = _scan_output(N, max(L // self.step_samples, 0), self.net.num_classes, self.device)
        fe, net = self.frontend, self.net
        self.lib.check(self.lib.tcr_scan_m(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), N, L, self.k, C.byref(self.det),
                                           samples.data_ptr(), self.workspace.data_ptr(), self.workspace.numel() * 4,
                                           *(t.data_ptr() for t in out), net._stream()), "tcr_scan")
        self._after_call()
        return out

    def scan_ragged(self, signals) -> RaggedScanOutput:
        """Signals of different lengths in one call (tcr_scan_ragged): a list of 1-D float32 device tensors, or (packed, lengths) --
        one 1-D float32 device tensor holding the signals one after the other and their lengths in samples.  Every length is a multiple
        of k * hop; 0 is allowed (no rows).  Returns a `RaggedScanOutput` of new tensors: `signal(n)` is bitwise `scan` of signal n
        alone, whatever max_windows and the other signals.  The weight rules are `scan`'s."""
        packed, lengths, offsets = _ragged_signals("scan_ragged", "signal", signals)
        N = int(lengths.size)
        self.net._check_tensor(packed, "scan samples")
        lib, fe, net = self.lib, self.frontend, self.net
        ws = self._ragged_workspace("scan_ragged", N)
        ref = self._call_ref()
        out = _ragged_scan_output(lengths, offsets, self.step_samples, net.num_classes, self.device)
        lib.check(lib.tcr_scan_ragged(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), N, offsets.ctypes.data, self.k, C.byref(self.det),
                                      packed.data_ptr(), ws.data_ptr(), ws.numel() * 4, *(t.data_ptr() for t in out.tensors()),
                                      net._stream()), "tcr_scan_ragged")
        self._after_call()
        return out

    def _steps_workspace(self, n: int, n_selected: int) -> torch.Tensor:
        """The workspace of `scan_steps` (sized by max_windows, the signals and the selected steps), allocated on the first call and
        again when a call brings more signals or more selected steps than it holds tables for."""
        have_n, have_sel = self._steps_ws_size
        if self._steps_ws is None or n > have_n or n_selected > have_sel:
            lib = self.lib
            size = (max(have_n, n, 1), max(have_sel, n_selected, self.max_windows))
            nws = lib.tcr_scan_steps_workspace_bytes(C.byref(self.frontend.cfg), C.byref(self._ref()), self.k, self.max_windows, *size)
            if nws == 0:
                raise TcrError(f"KeywordScanner.scan_steps: {lib.tcr_last_error().decode()}")
            self._steps_ws = torch.empty(nws // 4, dtype=torch.float32, device=self.device)
            self._steps_ws_size = size
        return self._steps_ws

    def _steps_args(self, signals, selected):
        packed, lengths, offsets = _ragged_signals("scan_steps", "signal", signals)
        self.net._check_tensor(packed, "scan samples")
        if isinstance(selected, torch.Tensor):
            if selected.dtype != torch.int64:
                raise TcrError(f"scan_steps expects int64 selected steps, got {selected.dtype}")
            selected = selected.detach().cpu().numpy()
        sel = np.ascontiguousarray(np.asarray(selected, dtype=np.int64))
        if sel.ndim != 1:
            raise TcrError(f"scan_steps expects 1-D selected steps, got shape {sel.shape}")
        return packed, lengths, offsets, sel

    def scan_steps(self, signals, selected) -> Tuple[torch.Tensor, torch.Tensor]:
        """A chosen subset of `scan_ragged`'s steps, at the cost of that subset (tcr_scan_steps).  `signals`: the forms `scan_ragged`
        takes; `selected`: packed step indices (rows of `scan_ragged`'s outputs), strictly increasing -- a 1-D int64 tensor on either
        side, or an array.  Returns (logits, probs) [n_selected, classes] (new tensors): row b is bitwise row selected[b] of
        `scan_ragged(signals)`, whatever max_windows and the other selected steps.  Only the front-end rows that hold a selected step
        and the selected windows are computed; no detector runs (merge the rows into a scan's probs and `redetect`).  The weight
        rules are `scan`'s.  The workspace is allocated on the first call and again when a call brings more signals or more
        selected steps."""
        packed, lengths, offsets, sel = self._steps_args(signals, selected)
        N, n_sel = int(lengths.size), int(sel.size)
        lib, fe, net = self.lib, self.frontend, self.net
        ws = self._steps_workspace(N, n_sel)
        ref = self._call_ref()
        logits = torch.empty((n_sel, net.num_classes), dtype=torch.float32, device=self.device)
        probs = torch.empty_like(logits)
        lib.check(lib.tcr_scan_steps(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), N, offsets.ctypes.data, self.k, sel.ctypes.data,
                                     n_sel, packed.data_ptr(), ws.data_ptr(), ws.numel() * 4, logits.data_ptr(), probs.data_ptr(),
                                     net._stream()), "tcr_scan_steps")
        self._after_call()
        return logits, probs

    def steps_plan(self, signals, selected) -> Dict[str, int]:
        """What `scan_steps(signals, selected)` would run, from the host alone (tcr_scan_steps_plan): group_steps (G), rows (front-end
        rows staged), row_frames (frames of a row), chunk_rows (rows per network launch) and windows (= the selected steps)."""
        packed, lengths, offsets, sel = self._steps_args(signals, selected)
        N, n_sel = int(lengths.size), int(sel.size)
        ws = self._steps_workspace(N, n_sel)
        plan = np.zeros(4, np.int64)
        lib = self.lib
        lib.check(lib.tcr_scan_steps_plan(C.byref(self.frontend.cfg), C.byref(self._ref()), N, offsets.ctypes.data, self.k, sel.ctypes.data,
                                          n_sel, ws.numel() * 4, plan.ctypes.data), "tcr_scan_steps_plan")
        return {"group_steps": int(plan[0]), "rows": int(plan[1]), "row_frames": int(plan[2]), "chunk_rows": int(plan[3]), "windows": n_sel}

    # ---- detector tuning from one scan ---------------------------------------------------------------------------------------
    def redetect(self, out, average_window_ms: Optional[float] = None, min_count: Optional[int] = None,
                 detection_threshold: Optional[float] = None, suppression_ms: Optional[float] = None):
        """The detector tail of `out` (a `ScanOutput` or `RaggedScanOutput` of this scanner's net and front-end) with other settings
        (None: the scanner's own; ms become steps as in the constructor): the same kind of output, logits / probs `out`'s own
        tensors, smoothed / top / score / is_new new tensors, bitwise what a scanner built with those settings returns for the same
        audio (tcr_detect_redetect).  Neither the front-end nor the network runs."""
        own = self.det
        det = self._detect_cfg(0.0 if average_window_ms is None else average_window_ms, own.min_count if min_count is None else min_count,
                               own.threshold if detection_threshold is None else detection_threshold,
                               0.0 if suppression_ms is None else suppression_ms)
        if average_window_ms is None:
            det.average_steps = own.average_steps
        if suppression_ms is None:
            det.suppression_steps = own.suppression_steps
        lib, ncls, dev = self.lib, self.net.num_classes, self.device
        probs = out.probs
        self.net._check_tensor(probs, "redetect probs")
        stream = self.net._stream()
        if isinstance(out, RaggedScanOutput):
            total = int(probs.shape[0])
            new = RaggedScanOutput(out.logits, probs, torch.empty_like(probs), torch.empty(total, dtype=torch.int32, device=dev),
                                   torch.empty(total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.int32, device=dev),
                                   out.offsets)
            off = torch.from_numpy(out.offsets).to(dev)
            lib.check(lib.tcr_detect_redetect_ragged(len(out), off.data_ptr(), total, ncls, probs.data_ptr(), C.byref(det),
                                                     new.smoothed.data_ptr(), new.top.data_ptr(), new.score.data_ptr(),
                                                     new.is_new.data_ptr(), stream), "tcr_detect_redetect_ragged")
            return new
        if probs.dim() != 3:
            raise TcrError(f"redetect expects probs [N, steps, classes], got shape {tuple(probs.shape)}")
        N, steps = int(probs.shape[0]), int(probs.shape[1])
        new = ScanOutput(out.logits, probs, torch.empty_like(probs), torch.empty((N, steps), dtype=torch.int32, device=dev),
                         torch.empty((N, steps), dtype=torch.float32, device=dev), torch.empty((N, steps), dtype=torch.int32, device=dev))
        lib.check(lib.tcr_detect_redetect(N, steps, ncls, probs.data_ptr(), C.byref(det), new.smoothed.data_ptr(), new.top.data_ptr(),
                                          new.score.data_ptr(), new.is_new.data_ptr(), stream), "tcr_detect_redetect")
        return new

    def tune(self, out, thresholds, average_window_ms: Sequence[float] = (), min_count: Sequence[int] = (),
             suppression_ms: Sequence[float] = (), events=None, lengths=None, tolerance_ms: float = 1000.0,
             labels: Optional[Sequence[str]] = None) -> "GridResult":
        """Every detector setting from one scan (tcr_detect_grid): the Cartesian grid average_window_ms x min_count x suppression_ms
        (in this nesting order; an empty axis: the scanner's own setting) x thresholds over `out`'s probs.  Point j's
        `GridResult.result(j)` equals `sweep(redetect(out, *point), thresholds, ...)`; events, lengths, tolerance_ms and labels are
        `sweep`'s (lengths is refused for a ragged output).  Combinations with min_count above the window's steps are dropped and
        listed in `GridResult.dropped`."""
        own = self.det
        ws = [(float(w), self._detect_cfg(w, 1, 0.0, 0).average_steps) for w in average_window_ms] or [(None, own.average_steps)]
        mcs = [int(m) for m in min_count] or [own.min_count]
        sps = [(float(x), self._detect_cfg(self.step_ms, 1, 0.0, x).suppression_steps) for x in suppression_ms] or \
            [(None, own.suppression_steps)]
        points, dropped = [], []
        for w_ms, w in ws:
            for mc in mcs:
                for s_ms, sp in sps:
                    (points if 1 <= mc <= w else dropped).append(GridPoint(w_ms, mc, s_ms, w, sp))
        if not points:
            raise TcrError(f"tune: every point of the grid has min_count above its window's steps: {[tuple(p) for p in dropped]}")
        ragged, valid, ev_steps = self._sweep_inputs(out, events, lengths, tolerance_ms, labels)
        self.net._check_tensor(out.probs, "tune probs")
        step_s = self.step_samples / self.frontend.cfg.sample_rate
        res = detection_grid(out.probs, points, thresholds, self.net.num_classes, ev_steps, out.offsets if ragged else None,
                             None if ragged else valid, step_s, self.lib)
        return GridResult(points, dropped, *res)


    # ---- mining hard examples ---------------------------------------------------------------------------------------------
    def _mine_workspace(self, n: int, ranked: bool) -> Optional[torch.Tensor]:
        """The workspace of `mine`'s calls, kept between calls and replaced when one needs more."""
        if n <= 0:
            return None
        ws = _mine_workspace("mine", self.lib, n, ranked, self.device, getattr(self, "_mine_ws", None))
        self._mine_ws = ws
        return ws

    def mine(self, out, signals, events=None, k: int = 1000, source: str = "detections", kinds: Sequence[str] = ("false_accept",),
              classes: Optional[Sequence[int]] = None, on: str = "probs", floor: float = 0.0, radius_ms: Optional[float] = None,
              tolerance_ms: float = 1000.0, labels: Optional[Sequence[str]] = None, lead_ms: float = 0.0, pcm: bool = False) -> MinedClips:
        """The audio `out` got wrong, for retraining.  out: a `ScanOutput` or `RaggedScanOutput` of this scanner (or a `redetect` /
        cascade of it); signals: the audio it scanned, in the forms `scan` / `scan_ragged` take; events, tolerance_ms, labels: `sweep`'s
        (the same conversion to step ranges).

        source="detections": out's detections (is_new) classified by the sweep's rule (tcr_mine_detections); `kinds` chooses among
        "false_accept", "hit" and "duplicate" (and `classes` among their labels; None: all), the k with the highest score are kept
        (tcr_mine_select), and "miss" adds one clip per event no detection hit, ending at the event's last step before the tolerance.
        source="peaks": the k highest local maxima of out's `on` ("probs" or "smoothed") over `classes` (None: every class from 2 on)
        that reach `floor`, within radius_ms on both sides (None: the suppression time; at least one step), outside every step whose
        window overlaps an event (tcr_mine_peaks): the near misses, whatever the threshold.

        The clip of step i of a signal is  signal[(i + 1) * step_samples + lead - n_samples : (i + 1) * step_samples + lead]  with lead =
        lead_ms in samples and zeros outside the signal (tcr_mine_gather): at lead_ms = 0 the window the network saw.  pcm: also as
        int16.  Rows are in increasing (signal, step) order, the misses after the rest."""
        step, sr, ncls, dev, lib = self.step_samples, self.frontend.cfg.sample_rate, self.net.num_classes, self.device, self.lib
        n_samples = int(self.frontend.cfg.n_samples)
        if source not in ("detections", "peaks"):
            raise TcrError(f"mine: source must be 'detections' or 'peaks', got {source!r}")
        kinds = [kinds] if isinstance(kinds, str) else list(kinds)
        bad = [x for x in kinds if x not in MINE_KINDS[:4]]
        if bad:
            raise TcrError(f"mine: unknown kinds {bad} (known: {list(MINE_KINDS[:4])})")
        if int(k) < 0:
            raise TcrError(f"mine: k must be >= 0 (got {k})")
        ragged, _, ev_steps = self._sweep_inputs(out, events, None, tolerance_ms, labels)
        if ragged:
            offsets = out.offsets
            packed, lengths, _ = _ragged_signals("mine", "signal", signals)
            flat = out
        else:
            N, steps = int(out.probs.shape[0]), int(out.probs.shape[1])
            offsets = np.arange(N + 1, dtype=np.int64) * steps
            if isinstance(signals, torch.Tensor) and signals.dim() == 2:
                packed, lengths = signals.reshape(-1), np.full(int(signals.shape[0]), int(signals.shape[1]), np.int64)
            else:
                packed, lengths, _ = _ragged_signals("mine", "signal", signals)
            flat = RaggedScanOutput(*(None if t is None else t.reshape(N * steps, *t.shape[2:]) for t in out), offsets)
        N = len(offsets) - 1
        if lengths.size != N or (lengths != np.diff(offsets) * step).any():
            raise TcrError(f"mine: the signals' lengths {lengths.tolist()} are not the scan's ({(np.diff(offsets) * step).tolist()} samples)")
        self.net._check_tensor(packed, "mine samples")
        sample_off = np.zeros(N + 1, np.int64)
        np.cumsum(lengths, out=sample_off[1:])
        # the events in the order of their step ranges (`_sweep_inputs` sorts by start, then end): their times and the CSR's offsets
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
                if classes is not None:
                    ev_label = np.concatenate([e[:, 2] for e in ev_steps]) if ev_steps else np.zeros(0, np.int64)
                    missed = missed[_class_mask("mine", classes, ncls)[ev_label[missed]] != 0]
                sig = ev_sig[missed]
                last = np.minimum(_last_steps(ev_ms[missed, 1], step, sr), np.diff(offsets)[sig] - 1)
                ok = last >= 0
                ev_label = np.concatenate([e[:, 2] for e in ev_steps]) if ev_steps else np.zeros(0, np.int64)
                add(offsets[sig[ok]] + last[ok], ev_label[missed[ok]], np.full(int(ok.sum()), np.nan, np.float32),
                    np.full(int(ok.sum()), 3, np.uint8), missed[ok])
        else:
            if on not in ("probs", "smoothed"):
                raise TcrError(f"mine: on must be 'probs' or 'smoothed', got {on!r}")
            radius = max(1, self.suppression_steps if radius_ms is None else ms_to_steps(radius_ms, self.step_ms))
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


def _thresholds(thresholds) -> np.ndarray:
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1).astype(np.float32))
    if thr.size == 0:
        raise TcrError("detection sweep: no thresholds")
    if np.isnan(thr).any():
        raise TcrError(f"detection sweep: NaN thresholds at positions {np.flatnonzero(np.isnan(thr)).tolist()}")
    return thr


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
    if lib is None:
        lib = _lib.get()
    ragged = step_offsets is not None
    if ragged:
        soff = np.ascontiguousarray(np.asarray(step_offsets, dtype=np.int64).reshape(-1))
        if valid_steps is not None:
            raise TcrError("detection sweep: valid_steps with step_offsets (a ragged scan's offsets are its signals' lengths)")
        if top.dim() != 1 or score.shape != top.shape:
            raise TcrError(f"detection sweep with step_offsets expects packed top and score [total_steps], got {tuple(top.shape)} and "
                           f"{tuple(score.shape)}")
        if soff.size < 2 or soff[0] != 0 or (np.diff(soff) < 0).any() or int(soff[-1]) != int(top.shape[0]):
            raise TcrError(f"detection sweep: step_offsets must run from 0 to the {int(top.shape[0])} packed steps without decreasing")
    elif top.dim() != 2 or score.shape != top.shape:
        raise TcrError(f"detection sweep expects top and score [N, steps], got {tuple(top.shape)} and {tuple(score.shape)}")
    if top.dtype != torch.int32 or score.dtype != torch.float32 or not top.is_contiguous() or not score.is_contiguous():
        raise TcrError("detection sweep expects contiguous int32 top and float32 score")
    if top.device != score.device:
        raise TcrError("detection sweep: top and score are on different devices")
    dev = top.device
    if ragged:
        N, steps, ncls = int(soff.size) - 1, int(top.shape[0]), int(num_classes)
    else:
        N, steps, ncls = int(top.shape[0]), int(top.shape[1]), int(num_classes)
    thr = _thresholds(thresholds)
    T = int(thr.size)
    if ragged:
        vs = np.diff(soff)
    else:
        vs = np.full(N, steps, np.int64) if valid_steps is None else np.asarray(valid_steps, np.int64).reshape(-1)
    if vs.shape != (N,):
        raise TcrError(f"detection sweep: {vs.size} valid_steps for {N} signals")
    if not ragged and ((vs < 0).any() or (vs > steps).any()):
        raise TcrError(f"detection sweep: valid_steps outside 0..{steps}: {vs.tolist()}")
    i32 = dict(dtype=torch.int32, device=dev)
    detections = torch.empty((N, T, ncls), **i32)
    hits = torch.zeros((N, T, ncls), **i32)
    dups = torch.zeros((N, T, ncls), **i32)
    fired = torch.empty((T, steps) if ragged else (T, N, steps), dtype=torch.uint8, device=dev) if return_fired else None
    counts, ev_args, keep = _pack_events(events, N, ncls, dev)
    thr_dev = torch.from_numpy(thr).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    hours = vs * float(step_seconds) / 3600.0 if step_seconds is not None else np.full(N, np.nan)
    if ragged:
        off_dev = torch.from_numpy(soff).to(dev)
        lib.check(lib.tcr_detect_sweep_ragged(N, off_dev.data_ptr(), ncls, top.data_ptr(), score.data_ptr(), int(suppression_steps), T,
                                              thr_dev.data_ptr(), *ev_args, detections.data_ptr(), hits.data_ptr(), dups.data_ptr(),
                                              None if fired is None else fired.data_ptr(), stream), "tcr_detect_sweep_ragged")
        return SweepResult(detections, hits, dups, fired, thr, counts, hours)
    vs_dev = torch.from_numpy(vs).to(dev)
    lib.check(lib.tcr_detect_sweep(N, steps, ncls, top.data_ptr(), score.data_ptr(), vs_dev.data_ptr(), int(suppression_steps), T,
                                   thr_dev.data_ptr(), *ev_args, detections.data_ptr(), hits.data_ptr(), dups.data_ptr(),
                                   None if fired is None else fired.data_ptr(), stream), "tcr_detect_sweep")
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
    if lib is None:
        lib = _lib.get()
    ragged = step_offsets is not None
    ncls = int(num_classes)
    if probs.dtype != torch.float32 or not probs.is_contiguous():
        raise TcrError("detection grid expects contiguous float32 probs")
    if ragged:
        soff = np.ascontiguousarray(np.asarray(step_offsets, dtype=np.int64).reshape(-1))
        if valid_steps is not None:
            raise TcrError("detection grid: valid_steps with step_offsets (a ragged scan's offsets are its signals' lengths)")
        if probs.dim() != 2 or int(probs.shape[1]) != ncls:
            raise TcrError(f"detection grid with step_offsets expects packed probs [total_steps, {ncls}], got {tuple(probs.shape)}")
        if soff.size < 2 or soff[0] != 0 or (np.diff(soff) < 0).any() or int(soff[-1]) != int(probs.shape[0]):
            raise TcrError(f"detection grid: step_offsets must run from 0 to the {int(probs.shape[0])} packed steps without decreasing")
        N, steps, total = int(soff.size) - 1, 0, int(probs.shape[0])
        vs = np.diff(soff)
    else:
        if probs.dim() != 3 or int(probs.shape[2]) != ncls:
            raise TcrError(f"detection grid expects probs [N, steps, {ncls}], got {tuple(probs.shape)}")
        N, steps = int(probs.shape[0]), int(probs.shape[1])
        total = N * steps
        vs = np.full(N, steps, np.int64) if valid_steps is None else np.asarray(valid_steps, np.int64).reshape(-1)
        if vs.shape != (N,):
            raise TcrError(f"detection grid: {vs.size} valid_steps for {N} signals")
        if (vs < 0).any() or (vs > steps).any():
            raise TcrError(f"detection grid: valid_steps outside 0..{steps}: {vs.tolist()}")
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
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    lib.check(lib.tcr_detect_grid(N, steps, None if off_dev is None else off_dev.data_ptr(), total, ncls, probs.data_ptr(),
                                  None if vs_dev is None else vs_dev.data_ptr(), J, arr, T, thr_dev.data_ptr(), *ev_args,
                                  detections.data_ptr(), hits.data_ptr(), dups.data_ptr(), ws.data_ptr(), nws, stream), "tcr_detect_grid")
    hours = vs * float(step_seconds) / 3600.0 if step_seconds is not None else np.full(N, np.nan)
    return detections, hits, dups, thr, counts, hours


# ---- cascades --------------------------------------------------------------------------------------------------------------------
def select_steps(values: torch.Tensor, offsets, enter: float, classes: Sequence[int], pad_before: int = 0, pad_after: int = 0,
                 lib=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The raw form of tcr_scan_select: the steps around the flags of `values`.  values [total_steps, C] float32 on the device (a
    ragged scan's probs or smoothed), offsets host int64 [N + 1] in steps (`RaggedScanOutput.offsets`), classes: the class indices
    that can flag.  Step p is flagged when one of those classes has values[p, c] >= enter (float32; NaN never flags) and selected
    when a flagged step of its signal lies in p - pad_after .. p + pad_before.  Returns (selected, mask) on the device: the selected
    packed steps, int64, increasing, and uint8 [total_steps] membership.  Reads one integer back (the number of selected steps), so
    the call waits for the device."""
    if lib is None:
        lib = _lib.get()
    soff = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if values.dim() != 2 or values.dtype != torch.float32 or not values.is_contiguous():
        raise TcrError(f"select_steps expects contiguous float32 values [total_steps, classes], got {values.dtype} {tuple(values.shape)}")
    total, ncls = int(values.shape[0]), int(values.shape[1])
    if soff.size < 2 or soff[0] != 0 or (np.diff(soff) < 0).any() or int(soff[-1]) != total:
        raise TcrError(f"select_steps: offsets must run from 0 to the {total} packed steps without decreasing")
    cls = np.asarray(list(classes), dtype=np.int64).reshape(-1)
    if cls.size and (cls.min() < 0 or cls.max() >= ncls):
        raise TcrError(f"select_steps: classes outside 0..{ncls - 1}: {cls.tolist()}")
    dev = values.device
    cmask = np.zeros(max(ncls, 1), np.uint8)
    cmask[cls] = 1
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    selected = torch.empty(total, dtype=torch.int64, device=dev)
    if total == 0:
        return selected, mask
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    cmask_dev, off_dev = torch.from_numpy(cmask).to(dev), torch.from_numpy(soff).to(dev)
    nws = lib.tcr_scan_select_workspace_bytes(total)
    if nws == 0:
        raise TcrError(f"select_steps: {lib.tcr_last_error().decode()}")
    ws = torch.empty(nws // 4, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    lib.check(lib.tcr_scan_select(int(soff.size) - 1, off_dev.data_ptr(), total, ncls, values.data_ptr(), cmask_dev.data_ptr(), float(enter),
                                  int(pad_before), int(pad_after), ws.data_ptr(), nws, selected.data_ptr(), count.data_ptr(),
                                  mask.data_ptr(), stream), "tcr_scan_select")
    return selected[:int(count.item())], mask


class CascadeOutput(RaggedScanOutput):
    """Results of a cascade scan: a `RaggedScanOutput` of the merged posteriors and the final (second-stage) detector over them, so
    `sweep` and `tune` of the second scanner take it unchanged.  `selected` (device int64): the packed steps the second model
    computed; `first`: the first stage's own `RaggedScanOutput`."""

    def __init__(self, logits, probs, smoothed, top, score, is_new, offsets, selected: torch.Tensor, first: RaggedScanOutput):
        super().__init__(logits, probs, smoothed, top, score, is_new, offsets)
        self.selected, self.first = selected, first


class CascadeScanner:
    """A two-stage scan: `first` (a cheap `KeywordScanner`) scans every step, the steps around its flags are selected, `second` (an
    expensive one) computes only those (`scan_steps`), and `second`'s detector runs over the merged posteriors.

    A step is flagged when a class of keyword_classes (default: every class from 2 on, after _silence_ and _unknown_) reaches
    enter_threshold in the first stage's `on` ("probs" or "smoothed"); pad_before_ms / pad_after_ms of audio in front of and behind
    every flag are selected with it (default: the second scanner's averaging window minus one step on both sides, so every vector the
    detector smooths at a flagged step, and for a window after it, is the second model's).  The scanners must share library, device,
    sample rate, num_classes and the step: k1 * hop1 == k2 * hop2 samples (a 30 / 10 ms first stage at k = 2 pairs with a 40 / 20 ms
    second stage at k = 1).  No state is carried between calls."""

    def __init__(self, first: KeywordScanner, second: KeywordScanner, enter_threshold: float,
                 keyword_classes: Optional[Sequence[int]] = None, pad_before_ms: Optional[float] = None,
                 pad_after_ms: Optional[float] = None, on: str = "probs"):
        if first.lib is not second.lib or first.device != second.device:
            raise TcrError("CascadeScanner: the two scanners must use the same library and device")
        r1, r2 = first.frontend.cfg.sample_rate, second.frontend.cfg.sample_rate
        if r1 != r2:
            raise TcrError(f"CascadeScanner: the scanners run at different sample rates ({r1} and {r2} Hz)")
        if first.step_samples != second.step_samples:
            raise TcrError(f"CascadeScanner: the scanners' steps differ ({first.step_samples} and {second.step_samples} samples): "
                           "k1 * hop1 must equal k2 * hop2")
        if first.net.num_classes != second.net.num_classes:
            raise TcrError(f"CascadeScanner: the scanners' models have {first.net.num_classes} and {second.net.num_classes} classes")
        if on not in ("probs", "smoothed"):
            raise TcrError(f"CascadeScanner: on must be 'probs' or 'smoothed', got {on!r}")
        if math.isnan(float(enter_threshold)):
            raise TcrError("CascadeScanner: enter_threshold is NaN")
        ncls = second.net.num_classes
        self.keyword_classes = list(range(2, ncls)) if keyword_classes is None else [int(c) for c in keyword_classes]
        if any(not 0 <= c < ncls for c in self.keyword_classes):
            raise TcrError(f"CascadeScanner: keyword_classes outside 0..{ncls - 1}: {self.keyword_classes}")
        self.first, self.second, self.lib, self.device = first, second, second.lib, second.device
        self.enter_threshold, self.on = float(enter_threshold), on
        default = second.average_steps - 1
        self.pad_before = default if pad_before_ms is None else ms_to_steps(pad_before_ms, second.step_ms)
        self.pad_after = default if pad_after_ms is None else ms_to_steps(pad_after_ms, second.step_ms)
        if self.pad_before < 0 or self.pad_after < 0:
            raise TcrError(f"CascadeScanner: negative pads ({pad_before_ms} ms before, {pad_after_ms} ms after)")

    def scan_ragged(self, signals) -> CascadeOutput:
        """`signals` as `KeywordScanner.scan_ragged` takes them -> `CascadeOutput`.  first.scan_ragged, `select_steps`, the read-back
        of the selected steps (their number, then the steps: the host builds the sparse scan's tables from them, the wait a ragged
        scan's tables already cost), second.scan_steps; logits / probs are the first stage's rows with the selected rows replaced
        by the second stage's, and smoothed / top / score / is_new are second.redetect of that merge.  Nothing selected: neither
        the second front-end nor the second network runs."""
        packed, lengths, _ = _ragged_signals("CascadeScanner.scan_ragged", "signal", signals)
        first = self.first.scan_ragged((packed, lengths))
        selected, _ = select_steps(getattr(first, self.on), first.offsets, self.enter_threshold, self.keyword_classes, self.pad_before,
                                   self.pad_after, self.lib)
        logits, probs = first.logits.clone(), first.probs.clone()
        if selected.numel():
            l2, p2 = self.second.scan_steps((packed, lengths), selected.cpu())
            logits.index_copy_(0, selected, l2)
            probs.index_copy_(0, selected, p2)
        det = self.second.redetect(RaggedScanOutput(logits, probs, None, None, None, None, first.offsets))
        return CascadeOutput(*det.tensors(), first.offsets, selected, first)

    def scan(self, samples: torch.Tensor) -> ScanOutput:
        """samples [N, L] float32 on the device, L a multiple of the step -> the cascade over N signals of equal length, as `ScanOutput`
        views [N, steps, ...] of `scan_ragged`'s tensors."""
        if samples.dim() != 2:
            raise TcrError(f"scan expects samples [N, L], got shape {tuple(samples.shape)}")
        N, L = int(samples.shape[0]), int(samples.shape[1])
        out = self.scan_ragged((samples.reshape(-1), [L] * N))
        steps = L // self.second.step_samples
        return ScanOutput(*(t.view(N, steps, *t.shape[1:]) for t in out.tensors()))


# ---- mining hard examples --------------------------------------------------------------------------------------------------------
MINE_KINDS = ("false_accept", "hit", "duplicate", "miss", "peak")      # `MinedClips.kind` codes; the first three are tcr_mine_detections'


def _stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None


def _mine_offsets(what: str, offsets, total: int) -> np.ndarray:
    if isinstance(offsets, torch.Tensor):
        if offsets.dtype != torch.int64:
            raise TcrError(f"{what} expects int64 offsets, got {offsets.dtype}")
        offsets = offsets.detach().cpu().numpy()
    off = np.asarray(offsets)
    if off.dtype != np.int64:
        raise TcrError(f"{what} expects int64 offsets, got {off.dtype}")
    off = np.ascontiguousarray(off.reshape(-1))
    if off.size < 2 or off[0] != 0 or (np.diff(off) < 0).any() or int(off[-1]) != total:
        raise TcrError(f"{what}: offsets must run from 0 to {total} without decreasing")
    return off


def _mine_workspace(what: str, lib, n: int, ranked: bool, dev, have: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 tensor of tcr_mine_workspace_bytes(n, ranked); `have` when that is one and large enough."""
    nws = lib.tcr_mine_workspace_bytes(n, int(ranked))
    if nws == 0:
        raise TcrError(f"{what}: {lib.tcr_last_error().decode()}")
    if have is not None and have.dtype == torch.int32 and have.device == dev and have.numel() * 4 >= nws:
        return have
    return torch.empty((nws + 3) // 4, dtype=torch.int32, device=dev)


def _class_mask(what: str, classes, ncls: int) -> np.ndarray:
    cls = np.asarray(list(classes), dtype=np.int64).reshape(-1)
    if cls.size and (cls.min() < 0 or cls.max() >= ncls):
        raise TcrError(f"{what}: classes outside 0..{ncls - 1}: {cls.tolist()}")
    mask = np.zeros(max(ncls, 1), np.uint8)
    mask[cls] = 1
    return mask


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
    if lib is None:
        lib = _lib.get()
    if top.dim() != 1 or score.shape != top.shape or is_new.shape != top.shape:
        raise TcrError(f"mine_detections expects packed top, score and is_new [total_steps], got {tuple(top.shape)}, {tuple(score.shape)} "
                       f"and {tuple(is_new.shape)}")
    if top.dtype != torch.int32 or is_new.dtype != torch.int32 or score.dtype != torch.float32 or \
            not (top.is_contiguous() and score.is_contiguous() and is_new.is_contiguous()):
        raise TcrError("mine_detections expects contiguous int32 top, float32 score and int32 is_new")
    total, ncls, dev = int(top.shape[0]), int(num_classes), top.device
    soff = _mine_offsets("mine_detections", offsets, total)
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
                                          _stream_of(dev)), "tcr_mine_detections")
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
    if lib is None:
        lib = _lib.get()
    if values.dim() != 2 or values.dtype != torch.float32 or not values.is_contiguous():
        raise TcrError(f"mine_peaks expects contiguous float32 values [total_steps, classes], got {values.dtype} {tuple(values.shape)}")
    total, ncls, dev = int(values.shape[0]), int(values.shape[1]), values.device
    soff = _mine_offsets("mine_peaks", offsets, total)
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
                                     count.data_ptr(), _stream_of(dev)), "tcr_mine_peaks")
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
    if lib is None:
        lib = _lib.get()
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
                                  count.data_ptr(), _stream_of(dev)), "tcr_mine_select")
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
    if lib is None:
        lib = _lib.get()
    if samples.dim() != 1 or samples.dtype != torch.float32 or not samples.is_contiguous():
        raise TcrError(f"gather_clips expects contiguous packed float32 samples, got {samples.dtype} {tuple(samples.shape)}")
    dev = samples.device
    soff = _mine_offsets("gather_clips", sample_offsets, int(samples.shape[0]))
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
                                  _stream_of(dev)), "tcr_mine_gather")
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


# ---- phrase detection ------------------------------------------------------------------------------------------------------------
BACKGROUND_LABEL = "_background_"
PHRASE_COMBINERS = {"product": _lib.PHRASE_PRODUCT, "min": _lib.PHRASE_MIN}


def phrase_scores(values: torch.Tensor, phrases: Sequence[Sequence[int]], window_steps: int, ordered: bool = True,
                  combine: str = "product", step_offsets=None, lib=None) -> torch.Tensor:
    """The raw form of tcr_phrase_scores(_ragged): values float32 on the device, [N, steps, C], or with step_offsets (host int64
    [N + 1]) packed [total_steps, C] -- a scan's smoothed (or probs); phrases: lists of class indices.  Returns the phrase posteriors,
    values' shape with P + 1 columns (the last: the background, 1 - the best phrase's score); see include/tcresnet_hip.h for the
    score.  The call only enqueues a kernel."""
    if lib is None:
        lib = _lib.get()
    if combine not in PHRASE_COMBINERS:
        raise TcrError(f"phrase_scores: combine must be one of {sorted(PHRASE_COMBINERS)}, got {combine!r}")
    ragged = step_offsets is not None
    if values.dtype != torch.float32 or not values.is_contiguous() or values.dim() != (2 if ragged else 3):
        raise TcrError(f"phrase_scores expects contiguous float32 values {'[total_steps, C]' if ragged else '[N, steps, C]'}, got "
                       f"{values.dtype} {tuple(values.shape)}")
    words = [[int(c) for c in q] for q in phrases]
    off = np.zeros(len(words) + 1, np.int32)
    np.cumsum([len(q) for q in words], out=off[1:])
    flat = np.ascontiguousarray(np.array([c for q in words for c in q] or [0], np.int32))
    cfg = _lib.PhraseCfg(int(window_steps), int(bool(ordered)), PHRASE_COMBINERS[combine])
    dev, ncls, P = values.device, int(values.shape[-1]), len(words)
    out = torch.empty((*values.shape[:-1], P + 1), dtype=torch.float32, device=dev)
    if ragged:
        soff = _mine_offsets("phrase_scores", step_offsets, int(values.shape[0]))
        if int(values.shape[0]) == 0:
            return out
        off_dev = torch.from_numpy(soff).to(dev)
        lib.check(lib.tcr_phrase_scores_ragged(int(soff.size) - 1, off_dev.data_ptr(), int(values.shape[0]), ncls, values.data_ptr(), P,
                                               off.ctypes.data, flat.ctypes.data, C.byref(cfg), out.data_ptr(), _stream_of(dev)),
                  "tcr_phrase_scores_ragged")
        return out
    lib.check(lib.tcr_phrase_scores(int(values.shape[0]), int(values.shape[1]), ncls, values.data_ptr(), P, off.ctypes.data,
                                    flat.ctypes.data, C.byref(cfg), out.data_ptr(), _stream_of(dev)), "tcr_phrase_scores")
    return out


class PhraseSweepResult(SweepResult):
    """A `SweepResult` over P phrases and the background class: `curve` and `operating_point` score the phrases only unless told
    otherwise (the background's firings are how a phrase gets to fire again, not detections)."""
    __slots__ = ()

    def curve(self, classes: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
        return super().curve(range(int(self.detections.shape[2]) - 1) if classes is None else classes)


class PhraseGridResult(GridResult):
    """A `GridResult` whose points' results are `PhraseSweepResult`s: `best` scores the phrases only by default."""

    def result(self, j: int) -> PhraseSweepResult:
        return PhraseSweepResult(*super().result(j))


class _PhraseClasses:
    """The model a `_PhraseView` shows to the detector-side methods: P + 1 classes on the scanner's device."""

    def __init__(self, net, num_classes: int):
        self._net, self.num_classes = net, num_classes

    def _check_tensor(self, t: torch.Tensor, what: str) -> None:
        self._net._check_tensor(t, what)

    def _stream(self):
        return self._net._stream()


class _PhraseView(KeywordScanner):
    """`KeywordScanner`'s detector-side methods (`sweep`, `tune`, `mine`: they read a scan's outputs and call `detection_sweep`,
    `detection_grid`, `mine_detections` / `mine_peaks` / `gather_clips`) over a phrase detector's P + 1 classes, with its detector
    settings: one vector per decision, no warm-up.  It owns no workspace and scans nothing."""

    def __init__(self, scanner: KeywordScanner, num_classes: int, det: _lib.DetectCfg):
        self.net, self.frontend, self.lib, self.device = _PhraseClasses(scanner.net, num_classes), scanner.frontend, scanner.lib, scanner.device
        self.k, self.step_samples, self.step_ms, self.det = scanner.k, scanner.step_samples, scanner.step_ms, det
        self._what, self._noun = "PhraseDetector", "phrase detector"


class PhraseDetector:
    """Multi-word phrases ("go left", "stop ... no") detected from a scan's posteriors on the device (tcr_phrase_scores): a phrase's
    score at a step is the best product (combine="product"; Chen et al. 2014) or minimum ("min") of its words' posteriors over the
    last window_ms of steps, the words in order (ordered=True; Prabhavalkar et al. 2015) or each at its own maximum.  The scores are
    posteriors over the phrases and a background class (1 - the best phrase's score), so the keyword stages apply to them with
    P + 1 classes: `detect` is the detector rule over them, `sweep`, `tune` and `mine` are the scanner's.

    scanner: the `KeywordScanner` whose outputs are scored (a cascade: its second scanner); phrases: a dict name -> words, or a list
    of word lists (name: the words joined by a space); a word is a class index or one of `labels` (the model's class names).
    window_ms becomes steps like the scanner's other ms settings (at least one); detection_threshold / suppression_ms: None takes the
    scanner's.  `labels` here are the phrase names and "_background_" last.  With "product" a per-word confidence p corresponds to a
    threshold of p ** n for a phrase of n words; "min" keeps thresholds on the single-word scale."""

    def __init__(self, scanner: KeywordScanner, phrases, window_ms: float = 1500, ordered: bool = True, combine: str = "product",
                 detection_threshold: Optional[float] = None, suppression_ms: Optional[float] = None,
                 labels: Optional[Sequence[str]] = None):
        if combine not in PHRASE_COMBINERS:
            raise TcrError(f"PhraseDetector: combine must be one of {sorted(PHRASE_COMBINERS)}, got {combine!r}")
        ncls = scanner.net.num_classes
        known = {str(x): c for c, x in enumerate(labels)} if labels is not None else {}
        items = list(phrases.items()) if isinstance(phrases, dict) else [(None, q) for q in phrases]
        if not 1 <= len(items) <= _lib.PHRASE_MAX:
            raise TcrError(f"PhraseDetector: {len(items)} phrases (1..{_lib.PHRASE_MAX})")
        self.names, self.words = [], []
        for name, q in items:
            q = q.split() if isinstance(q, str) else list(q)
            name = " ".join(str(x) for x in q) if name is None else str(name)
            if not q:
                raise TcrError(f"PhraseDetector: phrase {name!r} is empty")
            if len(q) > _lib.PHRASE_MAX_WORDS:
                raise TcrError(f"PhraseDetector: phrase {name!r} has {len(q)} words (1..{_lib.PHRASE_MAX_WORDS})")
            cls = []
            for x in q:
                c = known.get(x) if isinstance(x, str) else int(x)
                if c is None and isinstance(x, str) and labels is None and x.isdigit():
                    c = int(x)
                if c is None or not 0 <= c < ncls:
                    raise TcrError(f"PhraseDetector: phrase {name!r}: unknown word {x!r} (classes 0..{ncls - 1}"
                                   f"{'' if labels is None else ', labels ' + str(list(known))})")
                cls.append(c)
            if name in self.names or name == BACKGROUND_LABEL:
                raise TcrError(f"PhraseDetector: duplicate phrase name {name!r}")
            self.names.append(name)
            self.words.append(cls)
        self.scanner, self.lib, self.device = scanner, scanner.lib, scanner.device
        self.labels = self.names + [BACKGROUND_LABEL]
        self.ordered, self.combine = bool(ordered), combine
        self.window_steps = max(1, ms_to_steps(window_ms, scanner.step_ms))
        distinct = len({c for q in self.words for c in q})
        w_max = self.lib.tcr_phrase_window_max(distinct)
        if self.window_steps > w_max:
            raise TcrError(f"PhraseDetector: window_ms {window_ms:g} is {self.window_steps} steps, above the {w_max} that "
                           f"tcr_phrase_window_max allows for {distinct} distinct words")
        own = scanner.det
        det = scanner._detect_cfg(0.0, 1, own.threshold if detection_threshold is None else detection_threshold,
                                  0.0 if suppression_ms is None else suppression_ms)
        if suppression_ms is None:
            det.suppression_steps = own.suppression_steps
        self.det = det                                  # (average_steps = min_count = 1: a phrase posterior is a decision's whole input)
        self._view = _PhraseView(scanner, len(self.labels), det)

    @property
    def num_classes(self) -> int:
        """P + 1: the phrases and the background."""
        return len(self.labels)

    def _values(self, out, on: str) -> torch.Tensor:
        if on not in ("smoothed", "probs"):
            raise TcrError(f"PhraseDetector: on must be 'smoothed' or 'probs', got {on!r}")
        v, ncls = getattr(out, on), self.scanner.net.num_classes
        want_dim = 2 if isinstance(out, RaggedScanOutput) else 3
        if v is None or v.dim() != want_dim or int(v.shape[-1]) != ncls:
            raise TcrError(f"PhraseDetector: the output's {on} {None if v is None else tuple(v.shape)} is not a scan of the scanner's {ncls} "
                           "classes")
        self.scanner.net._check_tensor(v, f"phrase {on}")
        return v

    def scores(self, out, on: str = "smoothed") -> torch.Tensor:
        """The phrase posteriors of `out` (a `ScanOutput`, `RaggedScanOutput` or `CascadeOutput` of the scanner): float32 shaped
        like out.probs with P + 1 columns, from out's `on` ("smoothed", or "probs")."""
        v = self._values(out, on)
        return phrase_scores(v, self.words, self.window_steps, self.ordered, self.combine,
                             out.offsets if isinstance(out, RaggedScanOutput) else None, self.lib)

    def _is_detected(self, out) -> bool:
        return out.logits is None and out.probs is not None and out.smoothed is out.probs and int(out.probs.shape[-1]) == self.num_classes

    def detect(self, out, on: str = "smoothed"):
        """The phrase detections of a scan: the same kind of output object over P + 1 classes -- logits None, probs and smoothed the
        phrase posteriors (one tensor), top / score / is_new the detector rule over them (tcr_detect_redetect with average_steps =
        min_count = 1 and this detector's threshold and suppression): a phrase fires when it is on top above the threshold, and again
        only after the background (or another phrase) has been."""
        ph = self.scores(out, on)
        dev, lib, ncls = self.device, self.lib, self.num_classes
        rows = ph.shape[:-1]
        top, score = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev)
        is_new = torch.empty(rows, dtype=torch.int32, device=dev)
        stream = self.scanner.net._stream()
        if isinstance(out, RaggedScanOutput):
            total = int(ph.shape[0])
            if total > 0:
                off = torch.from_numpy(out.offsets).to(dev)
                lib.check(lib.tcr_detect_redetect_ragged(len(out), off.data_ptr(), total, ncls, ph.data_ptr(), C.byref(self.det), None,
                                                         top.data_ptr(), score.data_ptr(), is_new.data_ptr(), stream),
                          "tcr_detect_redetect_ragged")
            if isinstance(out, CascadeOutput):
                return CascadeOutput(None, ph, ph, top, score, is_new, out.offsets, out.selected, out.first)
            return RaggedScanOutput(None, ph, ph, top, score, is_new, out.offsets)
        lib.check(lib.tcr_detect_redetect(int(ph.shape[0]), int(ph.shape[1]), ncls, ph.data_ptr(), C.byref(self.det), None, top.data_ptr(),
                                          score.data_ptr(), is_new.data_ptr(), stream), "tcr_detect_redetect")
        return ScanOutput(None, ph, ph, top, score, is_new)

    def _detected(self, out):
        return out if self._is_detected(out) else self.detect(out)

    def sweep(self, out, thresholds, events=None, lengths=None, tolerance_ms: float = 1000.0, return_fired: bool = False) -> PhraseSweepResult:
        """`KeywordScanner.sweep` over the phrase detections of `out` (a scan's output, or `detect`'s): `detection_sweep` over their
        top / score with P + 1 classes and this detector's suppression.  Events are (start_ms, end_ms, phrase name or index)."""
        return PhraseSweepResult(*self._view.sweep(self._detected(out), thresholds, events, lengths, tolerance_ms, return_fired, self.labels))

    def tune(self, out, thresholds, suppression_ms: Sequence[float] = (), events=None, lengths=None,
             tolerance_ms: float = 1000.0) -> PhraseGridResult:
        """`KeywordScanner.tune` over the phrase posteriors of `out`: suppression_ms x thresholds in one `detection_grid` call (the
        window and min_count stay one step).  Point j equals `sweep` of a detector built with suppression_ms[j]."""
        g = self._view.tune(self._detected(out), thresholds, suppression_ms=suppression_ms, events=events, lengths=lengths,
                            tolerance_ms=tolerance_ms, labels=self.labels)
        return PhraseGridResult(g.points, g.dropped, g.detections, g.hits, g.duplicates, g.thresholds, g.events, g.hours)

    def mine(self, out, signals, events=None, k: int = 1000, source: str = "detections", kinds: Sequence[str] = ("false_accept",),
             classes: Optional[Sequence[int]] = None, **kw) -> MinedClips:
        """`KeywordScanner.mine` over the phrase detections of `out` (`signals`: the audio the scan read): the phrases that fired
        outside any event, the missed events, the near misses.  classes: phrase indices (default: every phrase, never the
        background); a clip ends at the step that fired (lead_ms moves it)."""
        cls = list(range(len(self.names))) if classes is None else [int(c) for c in classes]
        return self._view.mine(self._detected(out), signals, events, k, source, kinds, cls, labels=self.labels, **kw)
