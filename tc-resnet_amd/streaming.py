"""Streaming keyword spotting over many concurrent audio streams, on the device (tcr_stream_* of include/tcresnet_hip.h).

A `StreamingDetector` holds S streams.  Each starts as if it had heard one clip of digital silence; every `push` appends
k * hop samples to every stream (k = frames_per_step), computes only the k new front-end frames, runs the network on the
one-second window kept on the device and smooths the posteriors into detections (the speech-commands "recognize commands"
rule, stated in steps: see tcr_stream_step).  After a push, `window()` is bitwise the ordinary `Frontend` of each stream's last
n_samples samples, and the logits / probs are bitwise the network's eval forward of those windows at batch S
(`TCResNet.forward_frozen`, `DSCNN.forward_infer`, `Graph2D.forward_infer`).  `push_many` (tcr_stream_scan) appends many steps at
once at the offline scan's throughput, bitwise the same pushes; `push_ragged` (tcr_stream_scan_ragged) does so with a step count of
its own for every stream, none included.  Every model family runs: TC-ResNet, DS-CNN and the 2-D graphs
(tcr_model_ref of include/tcresnet_hip.h).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from ._lib import FAMILY_G2D, FAMILY_TCRESNET, ModelRef, TcrError, padded_len
from .capturing import CapturedClips, CapturedHost, StreamingRecorder  # noqa: F401
from .detection import (DEFAULT_MAX_WINDOWS, DetectionStage, PendingResets, _new_tensors, _ragged_scan_output,  # noqa: F401
                        _ragged_signals, _scan_output, check_on, ms_to_steps, reset_mask)
from .engine import DSCNN, Frontend, Graph2D, TCResNet

Network = Union[TCResNet, DSCNN, Graph2D]


class StreamOutput(NamedTuple):
    """Results of one step, all on the device: logits / probs / smoothed [S, classes] float32, top [S] int32 (-1 before
    min_count vectors), score [S] float32, is_new [S] int32 (1: a new detection of `top` at this step)."""
    logits: torch.Tensor
    probs: torch.Tensor
    smoothed: torch.Tensor
    top: torch.Tensor
    score: torch.Tensor
    is_new: torch.Tensor


class _Detection:
    """What `StreamingDetector` and `scanning.KeywordScanner` share: the argument checks, the detector settings in steps, the model
    reference of the C calls, the weight / fold rules (see `StreamingDetector`) and `stage`, the `detection.DetectionStage` over the net's
    classes that `sweep` (and the scanner's `redetect`, `tune`, `mine`) delegate to."""

    def _setup(self, what: str, noun: str, net: Network, frontend: Frontend, frames_per_step: int, average_window_ms: float,
               min_count: int, detection_threshold: float, suppression_ms: float) -> None:
        if not isinstance(net, (TCResNet, DSCNN, Graph2D)):
            raise TcrError(f"{what} runs TC-ResNet, DS-CNN and 2-D graph models, got {type(net).__name__}")
        if net.FAMILY == FAMILY_G2D and not net.finalized:
            raise TcrError(f"{what}: the 2-D graph is not finalized")
        if net.lib is not frontend.lib or net.device != frontend.device:
            raise TcrError("the network and the front-end must use the same library and device")
        self.net, self.frontend, self.lib, self.device = net, frontend, net.lib, net.device
        self.k = int(frames_per_step)
        cfg = frontend.cfg
        if not 1 <= self.k <= cfg.n_frames:
            raise TcrError(f"{what}: frames per step k = {self.k} outside 1..T = {cfg.n_frames}")
        self.step_samples = self.k * cfg.hop
        self.stage = st = DetectionStage(self.lib, self.device, net.num_classes, self.step_samples, cfg.sample_rate, cfg.n_samples)
        self.step_ms = st.step_ms
        st.det = self.det = st.detect_cfg(average_window_ms, min_count, detection_threshold, suppression_ms)
        self._what, self._noun = what, noun

    def _bind_frozen(self, frozen_ss: Optional[torch.Tensor]) -> None:
        net = self.net
        if frozen_ss is not None:
            if net.FAMILY != FAMILY_TCRESNET:
                raise TcrError(f"{self._what}: frozen_ss is a TC-ResNet folded BN table; {type(net).__name__} folds its BN from params / "
                               "stats in every call")
            net._check_tensor(frozen_ss, "frozen table")
        self._frozen = frozen_ss
        self._frozen_ver = (net.params._version, net._kver, net.params.data_ptr())

    def _ref(self, aux: Optional[torch.Tensor] = None) -> ModelRef:
        """The tcr_model_ref of a call: TC-ResNet with `aux` = its BN table (None for the size queries and init), DS-CNN / 2-D graph
        with the arenas the net holds now."""
        return self.net.model_ref(aux)

    def _call_ref(self) -> ModelRef:
        """The reference of a push / scan, after the weight rules: TC-ResNet refolds (or checks the frozen table's arena)."""
        if self.net.FAMILY != FAMILY_TCRESNET:
            return self._ref()
        if self._frozen is not None:
            self._check_frozen_arena()
        return self._ref(self._table())

    def _after_call(self) -> None:
        if self.net.FAMILY == FAMILY_TCRESNET:
            self.net._note_fold_reader()

    def _ragged_workspace(self, what: str, n: int) -> torch.Tensor:
        """The workspace of the ragged calls (sized by max_windows and max_signals), allocated on the first call and again when a call
        brings more than max_signals signals."""
        if self._ragged_ws is None or n > self.max_signals:
            self.max_signals = max(self.max_signals, n)
            lib = self.lib
            nws = lib.tcr_scan_ragged_workspace_bytes(C.byref(self.frontend.cfg), C.byref(self._ref()), self.k, self.max_windows, self.max_signals)
            if nws == 0:
                raise TcrError(f"{self._what}.{what}: {lib.tcr_last_error().decode()}")
            self._ragged_ws = torch.empty(nws // 4, dtype=torch.float32, device=self.device)
        return self._ragged_ws

    # ---- detector settings in steps ------------------------------------------------------------------------------------
    @property
    def average_steps(self) -> int:
        return self.det.average_steps

    @property
    def suppression_steps(self) -> int:
        return self.det.suppression_steps

    # ---- weights ------------------------------------------------------------------------------------------------------
    def _table(self) -> torch.Tensor:
        return self._frozen if self._frozen is not None else self.net._folded_table()

    def _check_frozen_arena(self):
        if (self.net.params._version, self.net._kver, self.net.params.data_ptr()) != self._frozen_ver:
            raise TcrError(f"{self._what}: the network's weights changed since the frozen table was bound; build a new {self._noun}")

    # ---- detection sweeps ---------------------------------------------------------------------------------------------
    def sweep(self, out, thresholds, events=None, lengths=None, tolerance_ms: float = 1000.0, return_fired: bool = False,
              labels: Optional[Sequence[str]] = None):
        """The detections of `out` at every threshold, with these settings' suppression_steps: for thresholds[t] exactly the steps
        a scanner built with detection_threshold = thresholds[t] marks in is_new (float32 thresholds; -inf and +inf allowed, NaN
        refused).  `out`: a scanning.ScanOutput of these settings (a KeywordScanner's scan, or StreamingDetector.push_many
        outputs concatenated over steps from a fresh detector); only its top / score are read.  See `scanning.detection_sweep`
        and `scanning.SweepResult`.

        lengths: per signal, its true length in samples (None: the whole scan); only its whole steps count, so signals of several
        lengths can share one zero-padded scan.  events: per signal, a list of (start_ms, end_ms, label), label a class index or
        one of `labels`.  A detection at step i is stamped at  t_i = 1000 * (i + 1) * step_samples / sample_rate  ms (the end of
        the window that fired, scan_audio.py's time) and hits an event of its label when  start_ms <= t_i <= end_ms + tolerance_ms;
        each event becomes the inclusive step range of those i, computed in float64.  Refused: events that overlap once the
        tolerance is added (start of the next <= end + tolerance_ms), that end before they start or start past the signal's
        length, unknown labels.

        `out` may be a scanning.RaggedScanOutput (`KeywordScanner.scan_ragged`): every signal is walked over its own rows, its events
        are relative to its own start, `fired` is [T, total_steps] and `hours` come from each signal's steps; `lengths` is refused,
        because the scan's lengths are the lengths."""
        return self.stage.sweep(out, thresholds, events, lengths, tolerance_ms, return_fired, labels)


def _cascade_pair(what: str, noun: str, first: _Detection, second: _Detection, enter_threshold: float, keyword_classes, on: str) -> list:
    """What a cascade's constructor (`what`) checks about its two stages (`noun`s: scanners or detectors) and its flag settings; returns
    the keyword classes (default: every class from 2 on)."""
    if first.lib is not second.lib or first.device != second.device:
        raise TcrError(f"{what}: the two {noun}s must use the same library and device")
    r1, r2 = first.frontend.cfg.sample_rate, second.frontend.cfg.sample_rate
    if r1 != r2:
        raise TcrError(f"{what}: the {noun}s run at different sample rates ({r1} and {r2} Hz)")
    if first.step_samples != second.step_samples:
        raise TcrError(f"{what}: the {noun}s' steps differ ({first.step_samples} and {second.step_samples} samples): "
                       "k1 * hop1 must equal k2 * hop2")
    ncls = second.net.num_classes
    if first.net.num_classes != ncls:
        raise TcrError(f"{what}: the {noun}s' models have {first.net.num_classes} and {ncls} classes")
    s1, s2 = getattr(first, "n_streams", None), getattr(second, "n_streams", None)      # (scanners hold no streams)
    if s1 != s2:
        raise TcrError(f"{what}: the {noun}s hold {s1} and {s2} streams")
    check_on(what, on, ("probs", "smoothed"))
    if np.isnan(float(enter_threshold)):
        raise TcrError(f"{what}: enter_threshold is NaN")
    classes = list(range(2, ncls)) if keyword_classes is None else [int(c) for c in keyword_classes]
    if any(not 0 <= c < ncls for c in classes):
        raise TcrError(f"{what}: keyword_classes outside 0..{ncls - 1}: {classes}")
    return classes


class StreamingDetector(_Detection, PendingResets):
    """S concurrent streams through `frontend` and `net` (a TCResNet, DSCNN or finalized Graph2D whose input is the front-end's
    n_coef x T features), k = frames_per_step new frames per stream and step.

    average_window_ms / suppression_ms become steps of k * hop / sample_rate seconds (the nearest whole number; the averaging
    ring holds at least one vector).  Silence / unknown classes get no special case: callers filter labels.

    Weights: without `frozen_ss` the detector runs on the net's folded BN table (`TCResNet._folded_table`): `push` refolds when
    the variables or moving statistics changed since the last fold, a `prepared` call refuses to run (prepare it again).  With
    `frozen_ss` (a frozen artifact's table, `FrozenModel.streaming`) that table is used as it is; the net's arena then only
    supplies the conv / fc weights, and both forms refuse to run once the arena changed.  DS-CNN and 2-D graphs have no fold:
    every call folds from the net's `params` / `stats` as they are then (in-place updates are seen by the next call), `frozen_ss`
    is refused, and a `prepared` call refuses to run once `params` or `stats` were rebound to other tensors.

    The output tensors are the detector's own and are overwritten by the next step (copy what must survive it).

    `push_many` advances every stream by many steps in one call at the offline scan's throughput (tcr_stream_scan), bitwise the
    same pushes; max_windows (default scanning.DEFAULT_MAX_WINDOWS) bounds its windows per network launch and sizes the scan
    workspace it allocates on first use.  `push_ragged` advances every stream by its own number of steps (tcr_stream_scan_ragged):
    a stream without steps in a call stays exactly where it is."""

    def __init__(self, net: Network, frontend: Frontend, n_streams: int, frames_per_step: int = 1, average_window_ms: float = 1000,
                 min_count: int = 3, detection_threshold: float = 0.5, suppression_ms: float = 1500,
                 frozen_ss: Optional[torch.Tensor] = None, max_windows: Optional[int] = None):
        self._setup("StreamingDetector", "detector", net, frontend, frames_per_step, average_window_ms, min_count, detection_threshold,
                    suppression_ms)
        self.n_streams = int(n_streams)
        self.max_windows, self.max_signals = int(DEFAULT_MAX_WINDOWS if max_windows is None else max_windows), self.n_streams
        self._scan_ws: Optional[torch.Tensor] = None
        self._ragged_ws: Optional[torch.Tensor] = None
        self._sel_ws: Optional[torch.Tensor] = None
        cfg = frontend.cfg
        S, lib = self.n_streams, self.lib
        if S <= 0:
            raise TcrError(f"StreamingDetector: n_streams must be positive (got {S})")
        ref = self._ref()
        nstate = lib.tcr_stream_state_bytes_m(C.byref(cfg), C.byref(ref), S, self.k, C.byref(self.det))
        if nstate == 0:
            raise TcrError(f"StreamingDetector: {lib.tcr_last_error().decode()}")
        nws = lib.tcr_stream_workspace_bytes_m(C.byref(cfg), C.byref(ref), S, self.k)
        if nws == 0:
            raise TcrError(f"StreamingDetector: {lib.tcr_last_error().decode()}")
        self._bind_frozen(frozen_ss)
        dev, ncls = self.device, net.num_classes
        self.state = torch.empty(nstate // 4, dtype=torch.float32, device=dev)
        self.workspace = torch.empty(nws // 4, dtype=torch.float32, device=dev)
        self.out = StreamOutput(*_new_tensors((S,), ncls, dev))
        self._init_resets(dev)
        lib.check(lib.tcr_stream_init_m(C.byref(cfg), frontend.plan.data_ptr(), C.byref(ref), S, self.k, C.byref(self.det),
                                        self.state.data_ptr(), self.workspace.data_ptr(), self.workspace.numel() * 4, net._stream()),
                  "tcr_stream_init")

    # ---- stream control -----------------------------------------------------------------------------------------------
    def window(self) -> torch.Tensor:
        """The streams' current window features, planar [S, n_coef, T + 2*HALO] (a view of the state)."""
        cfg = self.frontend.cfg
        n = self.n_streams * cfg.n_coef * padded_len(cfg.n_frames)
        return self.state[:n].view(self.n_streams, cfg.n_coef, padded_len(cfg.n_frames))

    # ---- steps --------------------------------------------------------------------------------------------------------
    def _check_samples(self, samples: torch.Tensor) -> None:
        if samples.dim() != 2 or tuple(samples.shape) != (self.n_streams, self.step_samples):
            raise TcrError(f"push expects samples [{self.n_streams}, {self.step_samples}] (k * hop per stream), got {tuple(samples.shape)}")
        self.net._check_tensor(samples, "stream samples")

    def _args(self, samples: torch.Tensor, ref: ModelRef, reset_ptr, stream):
        o, fe = self.out, self.frontend
        return (C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), self.n_streams, self.k, C.byref(self.det), samples.data_ptr(), reset_ptr, self.state.data_ptr(), self.workspace.data_ptr(), self.workspace.numel() * 4,
                o.logits.data_ptr(), o.probs.data_ptr(), o.smoothed.data_ptr(), o.top.data_ptr(), o.score.data_ptr(), o.is_new.data_ptr(),
                stream)

    def push(self, samples: torch.Tensor) -> StreamOutput:
        """Append samples [S, k * hop] (float32, on the device) to every stream; one step.  TC-ResNet: refolds BN first when the net's
        weights changed (without `frozen_ss`); with `frozen_ss`, raises once the conv / fc arena changed since construction."""
        self._check_samples(samples)
        ref = self._call_ref()
        self.lib.check(self.lib.tcr_stream_step_m(*self._args(samples, ref, self._take_reset(), self.net._stream())), "tcr_stream_step")
        self._after_call()
        return self.out

    def push_selected(self, samples: torch.Tensor, selected: torch.Tensor, n_selected: int, fill_logits: Optional[torch.Tensor],
                      fill_probs: Optional[torch.Tensor]) -> StreamOutput:
        """One step in which the network runs only on the streams `selected[:n_selected]` (int64 on the device, strictly increasing
        stream indices; n_selected a host integer): tcr_stream_step_selected_m.  Every stream's window and tail advance exactly as `push`
        advances them; a selected stream's logits / probs rows are `push`'s rows bitwise, every other stream's rows are its rows of
        fill_logits / fill_probs [S, classes] (float32 on the device; None allowed when all S are selected, which is `push` bitwise),
        and the detector runs over the merged probs.  The fill rows must not be this detector's `out` tensors.  Mixes freely with
        `push`, `push_many` and `push_ragged`; the weight / fold rules and pending resets are `push`'s.  The workspace of these steps is
        allocated on the first call."""
        self._check_samples(samples)
        S, ncls, lib, fe = self.n_streams, self.net.num_classes, self.lib, self.frontend
        n = int(n_selected)
        if not 0 <= n <= S:
            raise TcrError(f"push_selected: n_selected {n} outside 0..{S}")
        if selected.dtype != torch.int64 or selected.dim() != 1 or int(selected.numel()) < n or not selected.is_contiguous() \
                or selected.device.type != self.device.type:
            raise TcrError(f"push_selected expects selected: contiguous int64 [>= {n}] on the device, got {selected.dtype} "
                           f"{tuple(selected.shape)} on {selected.device}")
        for name, t in (("fill_logits", fill_logits), ("fill_probs", fill_probs)):
            if t is None:
                if n < S:
                    raise TcrError(f"push_selected: {name} is None with {n} of {S} streams selected")
                continue
            if tuple(t.shape) != (S, ncls):
                raise TcrError(f"push_selected expects {name} [{S}, {ncls}], got {tuple(t.shape)}")
            self.net._check_tensor(t, name)
        if self._sel_ws is None:
            nws = lib.tcr_stream_selected_workspace_bytes_m(C.byref(fe.cfg), C.byref(self._ref()), S, self.k)
            if nws == 0:
                raise TcrError(f"StreamingDetector.push_selected: {lib.tcr_last_error().decode()}")
            self._sel_ws = torch.empty(nws // 4, dtype=torch.float32, device=self.device)
        ref = self._call_ref()
        o, ws = self.out, self._sel_ws
        lib.check(lib.tcr_stream_step_selected_m(
            C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), S, self.k, C.byref(self.det), samples.data_ptr(), self._take_reset(),
            self.state.data_ptr(), ws.data_ptr(), ws.numel() * 4, selected.data_ptr(), n,
            None if fill_logits is None else fill_logits.data_ptr(), None if fill_probs is None else fill_probs.data_ptr(),
            o.logits.data_ptr(), o.probs.data_ptr(), o.smoothed.data_ptr(), o.top.data_ptr(), o.score.data_ptr(), o.is_new.data_ptr(),
            self.net._stream()), "tcr_stream_step_selected")
        self._after_call()
        return self.out

    def push_many(self, samples: torch.Tensor):
        """Append samples [S, m * k * hop] (float32, on the device) to every stream: m steps in one call (tcr_stream_scan), at the
        offline scan's throughput.  Returns a scanning.ScanOutput of new tensors, [S, m, ...]: step i is bitwise what the (i + 1)-th
        of m `push` calls returns, and the detector is left as those pushes leave it, so `push` and `push_many` mix freely.  Pending
        `reset`s apply at the first step; `out` is not touched.  The weight / fold rules are `push`'s.  The scan workspace (sized
        by max_windows) is allocated on the first call."""
        S, step = self.n_streams, self.step_samples
        if samples.dim() != 2 or int(samples.shape[0]) != S:
            raise TcrError(f"push_many expects samples [{S}, m * {step}] (m steps of k * hop per stream), got {tuple(samples.shape)}")
        self.net._check_tensor(samples, "stream samples")
        lib, fe, net = self.lib, self.frontend, self.net
        if self._scan_ws is None:
            nws = lib.tcr_scan_workspace_bytes_m(C.byref(fe.cfg), C.byref(self._ref()), self.k, self.max_windows)
            if nws == 0:
                raise TcrError(f"StreamingDetector.push_many: {lib.tcr_last_error().decode()}")
            self._scan_ws = torch.empty(nws // 4, dtype=torch.float32, device=self.device)
        ref = self._call_ref()
        L = int(samples.shape[1])
        out = _scan_output(S, max(L // step, 0), net.num_classes, self.device)
        ws = self._scan_ws
        lib.check(lib.tcr_stream_scan_m(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), S, L, self.k, C.byref(self.det),
                                        samples.data_ptr(), self._take_reset(), self.state.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                        *(t.data_ptr() for t in out), net._stream()), "tcr_stream_scan")
        self._after_call()
        return out

    def push_ragged(self, signals):
        """Every stream advances by its own number of steps in one call (tcr_stream_scan_ragged): `signals` is a list of S 1-D float32
        device tensors, stream s's m_s * k * hop new samples (m_s = 0: an empty tensor, the stream stays where it is), or (packed,
        lengths) -- one 1-D float32 device tensor holding them one after the other and their lengths in samples: the two forms
        `KeywordScanner.scan_ragged` takes.  Returns a scanning.RaggedScanOutput of new tensors (`offsets` in steps, `signal(s)` views
        of stream s's rows): stream s's rows are bitwise what m_s `push` calls return for it, and it is left as they leave it, so
        `push`, `push_many` and `push_ragged` mix freely.  A pending `reset` applies to a stream at the first call in which it has
        steps and stays pending for a stream without steps in this call; `out` is not touched.  The weight / fold rules are `push`'s.
        The ragged workspace (sized by max_windows and n_streams) is allocated on the first call.  At least one stream must have a
        step."""
        S = self.n_streams
        packed, lengths, offsets = _ragged_signals("push_ragged", "stream", signals, S)
        self.net._check_tensor(packed, "stream samples")
        lib, fe, net = self.lib, self.frontend, self.net
        ws = self._ragged_workspace("push_ragged", S)
        ref = self._call_ref()
        out = _ragged_scan_output(lengths, offsets, self.step_samples, net.num_classes, self.device)
        reset_ptr = self._begin_ragged_reset()
        lib.check(lib.tcr_stream_scan_ragged_m(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), S, offsets.ctypes.data, self.k,
                                               C.byref(self.det), packed.data_ptr(), reset_ptr, self.state.data_ptr(), ws.data_ptr(),
                                               ws.numel() * 4, *(t.data_ptr() for t in out.tensors()), net._stream()),
                  "tcr_stream_scan_ragged")
        self._end_ragged_reset(lengths)
        self._after_call()
        return out

    def prepared(self, samples_buffer: torch.Tensor):
        """A zero-argument callable that runs one step on `samples_buffer` (fill it in place between calls) with every pointer bound,
        on the stream current now: the per-step cost a C / C++ host of the ABI sees.  TC-ResNet: like `TCResNet.waveform_call` it
        refuses to run once the variables / moving statistics (or, with `frozen_ss`, the arena) changed since it was prepared.
        DS-CNN / 2-D graph: in-place weight updates are seen by the next call (push's rule), and it refuses to run once `params` or
        `stats` were rebound to other tensors.  Prepare it again then.  Resets requested with `reset` are applied by the next call."""
        self._check_samples(samples_buffer)
        net = self.net
        if net.FAMILY != FAMILY_TCRESNET:
            ref = self._ref()
            keep = (samples_buffer, net.params, net.stats, ref)
            bound_ptrs = (net.params.data_ptr(), net.stats.data_ptr())

            def stale():
                return (net.params.data_ptr(), net.stats.data_ptr()) != bound_ptrs
            why = "the network's params / stats were rebound since the call was prepared"
        else:
            if self._frozen is not None:
                self._check_frozen_arena()
                ss = self._frozen
            else:
                ss = net._folded_table()
                net._note_fold_reader()
            ref = self._ref(ss)
            keep = (samples_buffer, ss, ref)
            kver = (net.params._version, net.stats._version, net._kver)

            def stale():
                return (net.params._version, net.stats._version, net._kver) != kver
            why = "the weights changed since the call was prepared"
        stream = net._stream()
        args = self._args(samples_buffer, ref, None, stream)
        args_reset = self._args(samples_buffer, ref, self._reset_dev.data_ptr(), stream)
        fn, check, out = self.lib.tcr_stream_step_m, self.lib.check, self.out

        def call(_keep=keep):
            if stale():
                raise TcrError(f"StreamingDetector.prepared: {why}; prepare it again")
            bound = args
            if self._pending is not None:
                self._take_reset()
                bound = args_reset
            rc = fn(*bound)
            if rc:
                check(rc, "tcr_stream_step")
            return out
        return call


class StreamingCascade(PendingResets):
    """The causal cascade over S live streams: `first` (a cheap `StreamingDetector`) steps every stream, the streams at or shortly
    behind one of its flags are selected, `second` (an expensive one) runs its network on those only (`push_selected`), and `second`'s
    detector runs over the merged posteriors.  The pushes stacked over time are bitwise
    `scanning.CascadeScanner(first, second, enter_threshold, keyword_classes, pad_before_ms=0, pad_after_ms=pad_after_ms, on=on)`'s
    scan of the whole signals, on all six outputs and on the selection.

    A stream is flagged when a class of keyword_classes (default: every class from 2 on) reaches enter_threshold in the first stage's
    `on` ("probs" or "smoothed") at this step, and selected when it was flagged at this step or within pad_after_ms of audio before it
    (default: the second detector's averaging window minus one step) since its last reset.  A stream cannot be rescored before its
    flag, so pad_before is 0 by definition: at a flag the detector's average mixes first-stage rows from before it with second-stage
    rows from it on.  The detectors must share library, device, sample rate, num_classes, n_streams and the step (k1 * hop1 == k2 *
    hop2 samples).  Both keep their own state; every stream's second-stage window advances at every push, selected or not.

    Every push reads the number of selected streams back to the host (one small copy and wait, as a cascade scan pays per call), so a
    cascade push cannot be captured into a graph.  After a push: `mask` (uint8 [S]), `n_selected`, `selected` (an int64 view of the
    selected stream indices, increasing) and `first_out` (the first detector's `out`).  The output is the second detector's `out`, a
    `StreamOutput`: `scanning.StreamingPhraseDetector.push` takes it unchanged."""

    def __init__(self, first: StreamingDetector, second: StreamingDetector, enter_threshold: float,
                 keyword_classes: Optional[Sequence[int]] = None, pad_after_ms: Optional[float] = None, on: str = "probs"):
        what, ncls = "StreamingCascade", second.net.num_classes
        self.keyword_classes = _cascade_pair(what, "detector", first, second, enter_threshold, keyword_classes, on)
        self.pad_before = 0
        self.pad_after = second.average_steps - 1 if pad_after_ms is None else ms_to_steps(pad_after_ms, second.step_ms)
        if self.pad_after < 0:
            raise TcrError(f"{what}: negative pads ({pad_after_ms} ms after)")
        self.first, self.second, self.lib, self.device = first, second, second.lib, second.device
        self.enter_threshold, self.on = float(enter_threshold), on
        self.n_streams, self.step_samples = second.n_streams, second.step_samples
        S, dev, lib = self.n_streams, self.device, self.lib
        cmask = np.zeros(ncls, np.uint8)
        cmask[self.keyword_classes] = 1
        self._cmask = torch.from_numpy(cmask).to(dev)
        self._since = torch.empty(S, dtype=torch.int32, device=dev)
        self._selected = torch.zeros(S, dtype=torch.int64, device=dev)
        self._count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.mask = torch.zeros(S, dtype=torch.uint8, device=dev)
        self._init_resets(dev)
        nws = lib.tcr_stream_select_workspace_bytes(S)
        if nws == 0:
            raise TcrError(f"{what}: {lib.tcr_last_error().decode()}")
        self._ws = torch.empty(nws // 4, dtype=torch.int32, device=dev)
        self.n_selected, self.selected, self.first_out = 0, self._selected[:0], first.out
        lib.check(lib.tcr_stream_select_init(S, self._since.data_ptr(), second.net._stream()), "tcr_stream_select_init")

    def reset(self, mask_or_indices) -> None:
        """Return streams to the initial state at the NEXT push, before its samples are appended: both detectors
        (`StreamingDetector.reset`) and the selection (never flagged)."""
        mask = reset_mask(mask_or_indices, self.n_streams)
        self.first.reset(mask)
        self.second.reset(mask)
        super().reset(mask)

    def push(self, samples: torch.Tensor) -> StreamOutput:
        """Append samples [S, step_samples] (float32, on the device) to every stream; one step of both detectors.  first.push, the
        selection (tcr_stream_select), the read-back of the number of selected streams, second.push_selected with the first stage's
        logits / probs as fill rows.  Nothing selected: the second network does not run."""
        lib, S = self.lib, self.n_streams
        reset_ptr = self._take_reset()
        out1 = self.first.push(samples)
        values = getattr(out1, self.on)
        lib.check(lib.tcr_stream_select(S, int(values.shape[1]), values.data_ptr(), self._cmask.data_ptr(), self.enter_threshold,
                                        self.pad_after, reset_ptr, self._since.data_ptr(), self._ws.data_ptr(), self._ws.numel() * 4,
                                        self._selected.data_ptr(), self._count.data_ptr(), self.mask.data_ptr(),
                                        self.second.net._stream()), "tcr_stream_select")
        n = int(self._count.item())
        self.n_selected, self.selected, self.first_out = n, self._selected[:n], out1
        return self.second.push_selected(samples, self._selected, n, out1.logits, out1.probs)
