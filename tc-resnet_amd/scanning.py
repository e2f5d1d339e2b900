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

A `TemplateDetector` does the same for keywords enrolled from a few recorded examples (`KeywordTemplates`), matched against the scan's
posteriors by subsequence dynamic time warping (tcr_dtw_scores).

This module holds the scanners and the cascade; the rest is importable from here and lives in `detection` (the outputs, the ms / step
arithmetic and `DetectionStage`: `redetect`, `sweep`, `tune`, `mine` over a scan's outputs, no network needed), `scoring` (`detection_sweep`,
`detection_grid`, their results), `mining` (`mine_*`, `select_top`, `gather_clips`, `MinedClips`), `phrases` (`PhraseDetector`, `StreamingPhraseDetector`), `templates` (`KeywordTemplates`, `TemplateDetector`, `StreamingTemplateDetector`) and `capturing`
(`StreamingRecorder`, `CapturedClips`).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TcrError
from .capturing import CapturedClips, CapturedHost, StreamingRecorder  # noqa: F401
from .detection import (DEFAULT_MAX_WINDOWS, CascadeOutput, RaggedScanOutput, ScanOutput, _ragged_scan_output, _ragged_signals,  # noqa: F401
                        _scan_output, ms_to_steps)
from .engine import Frontend
from .mining import MINE_KINDS, MinedClips, MinedDetections, MinedPeaks, gather_clips, mine_detections, mine_peaks, select_top  # noqa: F401
from .phrases import BACKGROUND_LABEL, PHRASE_COMBINERS, PhraseDetector, PhraseGridResult, PhraseSweepResult, StreamingPhraseDetector, phrase_scores  # noqa: F401
from .runtime import stream_of
from .scoring import GridPoint, GridResult, SweepResult, _class_mask, _offsets, detection_grid, detection_sweep  # noqa: F401
from .streaming import Network, _cascade_pair, _Detection
from .templates import KeywordTemplates, StreamingTemplateDetector, TemplateDetector, dtw_scores  # noqa: F401

DEFAULT_MAX_SIGNALS = 65536


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

    # ---- detector tuning and mining from one scan: the detection stage's ---------------------------------------------------------
    def redetect(self, out, average_window_ms: Optional[float] = None, min_count: Optional[int] = None,
                 detection_threshold: Optional[float] = None, suppression_ms: Optional[float] = None):
        """The detector tail of `out` (a `ScanOutput` or `RaggedScanOutput` of this scanner's net and front-end) with other settings
        (None: the scanner's own; ms become steps as in the constructor): the same kind of output, logits / probs `out`'s own
        tensors, smoothed / top / score / is_new new tensors, bitwise what a scanner built with those settings returns for the same
        audio (tcr_detect_redetect).  Neither the front-end nor the network runs."""
        return self.stage.redetect(out, average_window_ms, min_count, detection_threshold, suppression_ms)

    def tune(self, out, thresholds, average_window_ms: Sequence[float] = (), min_count: Sequence[int] = (),
             suppression_ms: Sequence[float] = (), events=None, lengths=None, tolerance_ms: float = 1000.0,
             labels: Optional[Sequence[str]] = None) -> GridResult:
        """Every detector setting from one scan (tcr_detect_grid): the Cartesian grid average_window_ms x min_count x suppression_ms
        (in this nesting order; an empty axis: the scanner's own setting) x thresholds over `out`'s probs.  Point j's
        `GridResult.result(j)` equals `sweep(redetect(out, *point), thresholds, ...)`; events, lengths, tolerance_ms and labels are
        `sweep`'s (lengths is refused for a ragged output).  Combinations with min_count above the window's steps are dropped and
        listed in `GridResult.dropped`."""
        return self.stage.tune(out, thresholds, average_window_ms, min_count, suppression_ms, events, lengths, tolerance_ms, labels)

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
        return self.stage.mine(out, signals, events, k, source, kinds, classes, on, floor, radius_ms, tolerance_ms, labels, lead_ms, pcm)


# ---- cascades --------------------------------------------------------------------------------------------------------------------
def select_steps(values: torch.Tensor, offsets, enter: float, classes: Sequence[int], pad_before: int = 0, pad_after: int = 0,
                 lib=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The raw form of tcr_scan_select: the steps around the flags of `values`.  values [total_steps, C] float32 on the device (a
    ragged scan's probs or smoothed), offsets host int64 [N + 1] in steps (`RaggedScanOutput.offsets`), classes: the class indices
    that can flag.  Step p is flagged when one of those classes has values[p, c] >= enter (float32; NaN never flags) and selected
    when a flagged step of its signal lies in p - pad_after .. p + pad_before.  Returns (selected, mask) on the device: the selected
    packed steps, int64, increasing, and uint8 [total_steps] membership.  Reads one integer back (the number of selected steps), so
    the call waits for the device."""
    lib = _lib.get() if lib is None else lib
    if values.dim() != 2 or values.dtype != torch.float32 or not values.is_contiguous():
        raise TcrError(f"select_steps expects contiguous float32 values [total_steps, classes], got {values.dtype} {tuple(values.shape)}")
    total, ncls = int(values.shape[0]), int(values.shape[1])
    soff = _offsets("select_steps", "offsets", offsets, total, "the {} packed steps")
    cmask = _class_mask("select_steps", classes, ncls)
    dev = values.device
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
    lib.check(lib.tcr_scan_select(int(soff.size) - 1, off_dev.data_ptr(), total, ncls, values.data_ptr(), cmask_dev.data_ptr(), float(enter),
                                  int(pad_before), int(pad_after), ws.data_ptr(), nws, selected.data_ptr(), count.data_ptr(),
                                  mask.data_ptr(), stream_of(dev)), "tcr_scan_select")
    return selected[:int(count.item())], mask


class CascadeScanner:
    """A two-stage scan: `first` (a cheap `KeywordScanner`) scans every step, the steps around its flags are selected, `second` (an
    expensive one) computes only those (`scan_steps`), and `second`'s detector runs over the merged posteriors.

    A step is flagged when a class of keyword_classes (default: every class from 2 on, after _silence_ and _unknown_) reaches
    enter_threshold in the first stage's `on` ("probs" or "smoothed"); pad_before_ms / pad_after_ms of audio in front of and behind
    every flag are selected with it (default: the second scanner's averaging window minus one step on both sides, so every vector the
    detector smooths at a flagged step, and for a window after it, is the second model's).  The scanners must share library, device,
    sample rate, num_classes and the step: k1 * hop1 == k2 * hop2 samples (a 30 / 10 ms first stage at k = 2 pairs with a 40 / 20 ms
    second stage at k = 1).  No state is carried between calls; `streaming.StreamingCascade` is the cascade over live streams (the
    causal one: pad_before = 0), whose pushes are bitwise this scanner's scan at pad_before_ms = 0."""

    def __init__(self, first: KeywordScanner, second: KeywordScanner, enter_threshold: float,
                 keyword_classes: Optional[Sequence[int]] = None, pad_before_ms: Optional[float] = None,
                 pad_after_ms: Optional[float] = None, on: str = "probs"):
        self.keyword_classes = _cascade_pair("CascadeScanner", "scanner", first, second, enter_threshold, keyword_classes, on)
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

