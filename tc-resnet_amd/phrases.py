"""Phrase detection from a scan's posteriors on the device (tcr_phrase_scores): `phrase_scores` over raw tensors, and `PhraseDetector`,
which scores a `KeywordScanner`'s outputs into posteriors over P phrases and a background class and runs a `detection.DetectionStage`
of P + 1 classes over them: the detector rule, `sweep`, `tune` and `mine`.  `PhraseDetector.streaming` gives the same detector over the
pushes of a `StreamingDetector` (`StreamingPhraseDetector`, tcr_phrase_stream_push): the phrase window and the detector are carried on
the device, so any way of cutting the streams into pushes gives, bitwise, `detect` of the whole scan."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import TcrError
from .detection import CascadeOutput, DetectionStage, PendingResets, RaggedScanOutput, ScanOutput, _new_tensors, check_on, ms_to_steps
from .mining import MinedClips
from .runtime import stream_of
from .scoring import GridResult, SweepResult, _offsets
from .streaming import StreamOutput

BACKGROUND_LABEL = "_background_"
PHRASE_COMBINERS = {"product": _lib.PHRASE_PRODUCT, "min": _lib.PHRASE_MIN}


def phrase_scores(values: torch.Tensor, phrases: Sequence[Sequence[int]], window_steps: int, ordered: bool = True,
                  combine: str = "product", step_offsets=None, lib=None) -> torch.Tensor:
    """The raw form of tcr_phrase_scores(_ragged): values float32 on the device, [N, steps, C], or with step_offsets (host int64
    [N + 1]) packed [total_steps, C] -- a scan's smoothed (or probs); phrases: lists of class indices.  Returns the phrase posteriors,
    values' shape with P + 1 columns (the last: the background, 1 - the best phrase's score); see include/tcresnet_hip.h for the
    score.  The call only enqueues a kernel."""
    lib = _lib.get() if lib is None else lib
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
        soff = _offsets("phrase_scores", "offsets", step_offsets, int(values.shape[0]), int64_only=True)
        if int(values.shape[0]) == 0:
            return out
        off_dev = torch.from_numpy(soff).to(dev)
        lib.check(lib.tcr_phrase_scores_ragged(int(soff.size) - 1, off_dev.data_ptr(), int(values.shape[0]), ncls, values.data_ptr(), P,
                                               off.ctypes.data, flat.ctypes.data, C.byref(cfg), out.data_ptr(), stream_of(dev)),
                  "tcr_phrase_scores_ragged")
        return out
    lib.check(lib.tcr_phrase_scores(int(values.shape[0]), int(values.shape[1]), ncls, values.data_ptr(), P, off.ctypes.data,
                                    flat.ctypes.data, C.byref(cfg), out.data_ptr(), stream_of(dev)), "tcr_phrase_scores")
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

    def __init__(self, scanner, phrases, window_ms: float = 1500, ordered: bool = True, combine: str = "product",
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
        self._make_stage(detection_threshold, suppression_ms)

    def _make_stage(self, detection_threshold: Optional[float], suppression_ms: Optional[float]) -> None:
        """`det` and `stage` over this detector's `labels`, from its scanner's stage."""
        st = self.scanner.stage
        self.det = det = st.detect_cfg(0.0, 1, detection_threshold, suppression_ms)     # (one vector per decision: a posterior is its whole input)
        self.stage = DetectionStage(st.lib, st.device, len(self.labels), st.step_samples, st.sample_rate, st.clip_samples, det)

    on, _noun = "smoothed", "phrase"            # the rows read by default, and this detector's word for itself in messages

    @property
    def num_classes(self) -> int:
        """P + 1: the phrases and the background."""
        return len(self.labels)

    def _values(self, out, on: Optional[str]) -> torch.Tensor:
        what = type(self).__name__
        on = check_on(what, self.on if on is None else on)
        v, ncls = getattr(out, on), self.scanner.net.num_classes
        want_dim = 2 if isinstance(out, RaggedScanOutput) else 3
        if v is None or v.dim() != want_dim or int(v.shape[-1]) != ncls:
            raise TcrError(f"{what}: the output's {on} {None if v is None else tuple(v.shape)} is not a scan of the scanner's {ncls} "
                           "classes")
        self.scanner.net._check_tensor(v, f"{self._noun} {on}")
        return v

    def scores(self, out, on: str = "smoothed") -> torch.Tensor:
        """The phrase posteriors of `out` (a `ScanOutput`, `RaggedScanOutput` or `CascadeOutput` of the scanner): float32 shaped
        like out.probs with P + 1 columns, from out's `on` ("smoothed", or "probs")."""
        v = self._values(out, on)
        return phrase_scores(v, self.words, self.window_steps, self.ordered, self.combine,
                             out.offsets if isinstance(out, RaggedScanOutput) else None, self.lib)

    def streaming(self, n_streams: int) -> "StreamingPhraseDetector":
        """This detector over the pushes of a `StreamingDetector` of n_streams streams: the same phrases, window, order, combine,
        threshold and suppression, carried across pushes (`StreamingPhraseDetector`)."""
        return StreamingPhraseDetector(self, n_streams)

    def _is_detected(self, out) -> bool:
        return out.logits is None and out.probs is not None and out.smoothed is out.probs and int(out.probs.shape[-1]) == self.num_classes

    def detect(self, out, on: str = "smoothed"):
        """The phrase detections of a scan: the same kind of output object over P + 1 classes -- logits None, probs and smoothed the
        phrase posteriors (one tensor), top / score / is_new the detector rule over them (tcr_detect_redetect with average_steps =
        min_count = 1 and this detector's threshold and suppression): a phrase fires when it is on top above the threshold, and again
        only after the background (or another phrase) has been."""
        return self._detect(out, self.scores(out, on))

    def _detect(self, out, ph: torch.Tensor):
        """The detector rule over the posteriors `ph` of `out`, in out's kind of output object."""
        ragged = isinstance(out, RaggedScanOutput)
        if ragged and int(ph.shape[0]) == 0:                # (no rows in all: nothing to launch, and the library refuses the call)
            det = RaggedScanOutput(None, ph, ph, *_new_tensors((0,), 0, self.device, 0), out.offsets)
        else:
            posteriors = RaggedScanOutput(None, ph, None, None, None, None, out.offsets) if ragged else ScanOutput(None, ph, None, None, None, None)
            det = self.stage.redetect(posteriors, smoothed=False)
        if isinstance(out, CascadeOutput):
            return CascadeOutput(*det.tensors(), out.offsets, out.selected, out.first)
        return det

    def _detected(self, out):
        return out if self._is_detected(out) else self.detect(out)

    def sweep(self, out, thresholds, events=None, lengths=None, tolerance_ms: float = 1000.0, return_fired: bool = False) -> PhraseSweepResult:
        """`KeywordScanner.sweep` over the phrase detections of `out` (a scan's output, or `detect`'s): `detection_sweep` over their
        top / score with P + 1 classes and this detector's suppression.  Events are (start_ms, end_ms, phrase name or index)."""
        return PhraseSweepResult(*self.stage.sweep(self._detected(out), thresholds, events, lengths, tolerance_ms, return_fired, self.labels))

    def tune(self, out, thresholds, suppression_ms: Sequence[float] = (), events=None, lengths=None,
             tolerance_ms: float = 1000.0) -> PhraseGridResult:
        """`KeywordScanner.tune` over the phrase posteriors of `out`: suppression_ms x thresholds in one `detection_grid` call (the
        window and min_count stay one step).  Point j equals `sweep` of a detector built with suppression_ms[j]."""
        g = self.stage.tune(self._detected(out), thresholds, suppression_ms=suppression_ms, events=events, lengths=lengths,
                            tolerance_ms=tolerance_ms, labels=self.labels)
        return PhraseGridResult(g.points, g.dropped, g.detections, g.hits, g.duplicates, g.thresholds, g.events, g.hours)

    def mine(self, out, signals, events=None, k: int = 1000, source: str = "detections", kinds: Sequence[str] = ("false_accept",),
             classes: Optional[Sequence[int]] = None, **kw) -> MinedClips:
        """`KeywordScanner.mine` over the phrase detections of `out` (`signals`: the audio the scan read): the phrases that fired
        outside any event, the missed events, the near misses.  classes: phrase indices (default: every phrase, never the
        background); a clip ends at the step that fired (lead_ms moves it)."""
        cls = list(range(len(self.names))) if classes is None else [int(c) for c in classes]
        return self.stage.mine(self._detected(out), signals, events, k, source, kinds, cls, labels=self.labels, **kw)


class _PosteriorStream(PendingResets):
    """What `StreamingPhraseDetector` and `templates.StreamingTemplateDetector` share: a posterior detector (`detector`: a
    `PhraseDetector` or `TemplateDetector`) over the pushes of a `StreamingDetector` of n_streams streams, its state on the device.  A
    subclass names its C entries (`_entry` + _state_bytes / _init / _push / _push_ragged), supplies their table arguments (`_tables`) and
    says whether a push also writes `lengths` (`_has_lengths`: one column per class but the background, after the posteriors)."""
    _entry = ""
    _has_lengths = False

    def __init__(self, detector: PhraseDetector, n_streams: int):
        what = type(self).__name__
        self.detector, self.lib, self.device = detector, detector.lib, detector.device
        self.n_streams = S = int(n_streams)
        if S <= 0:
            raise TcrError(f"{what}: n_streams must be positive (got {S})")
        self.labels, self.num_classes = detector.labels, detector.num_classes
        self._classes = detector.scanner.net.num_classes
        lib, dev = self.lib, self.device
        self._push_c, self._push_ragged_c = getattr(lib, self._entry + "_push"), getattr(lib, self._entry + "_push_ragged")
        nstate = getattr(lib, self._entry + "_state_bytes")(S, self._classes, *self._tables())
        if nstate == 0:
            raise TcrError(f"{what}: {lib.tcr_last_error().decode()}")
        self.state = torch.empty(nstate // 4, dtype=torch.float32, device=dev)
        post, top, score, is_new = _new_tensors((S,), self.num_classes, dev, 1)
        self.out = StreamOutput(None, post, post, top, score, is_new)
        if self._has_lengths:
            self._own_lengths = self.lengths = self._new_lengths((S,))
        self._init_resets(dev)
        lib.check(getattr(lib, self._entry + "_init")(S, self._classes, *self._tables(), self.state.data_ptr(), stream_of(dev)),
                  self._entry + "_init")

    def _tables(self):
        raise NotImplementedError

    def _new_lengths(self, rows) -> torch.Tensor:
        return torch.empty((*rows, self.num_classes - 1), dtype=torch.int32, device=self.device)

    def _values(self, out, on: Optional[str]) -> torch.Tensor:
        what = type(self).__name__
        on = check_on(what, self.detector.on if on is None else on)
        v, S, ncls = getattr(out, on), self.n_streams, self._classes
        if v is None or int(v.shape[-1]) != ncls:
            raise TcrError(f"{what}: the output's {on} {None if v is None else tuple(v.shape)} is not over the detector's "
                           f"{ncls} classes")
        if isinstance(out, RaggedScanOutput):
            ok = v.dim() == 2 and len(out) == S
        else:
            ok = v.dim() == (2 if isinstance(out, StreamOutput) else 3) and int(v.shape[0]) == S
        if not ok:
            raise TcrError(f"{what}: the output's {on} {tuple(v.shape)} is not a push of {S} streams")
        self.detector.scanner.net._check_tensor(v, f"{self.detector._noun} {on}")
        return v

    def push(self, out, on: Optional[str] = None):
        v = self._values(out, on)
        lib, dev, S, K = self.lib, self.device, self.n_streams, self.num_classes
        ragged = isinstance(out, RaggedScanOutput)
        if isinstance(out, StreamOutput):                       # one step: this object's own tensors
            res, count = self.out, 1
            if self._has_lengths:
                self.lengths = self._own_lengths
        else:
            rows = (int(v.shape[0]),) if ragged else (S, int(v.shape[1]))
            count = rows[-1]                                    # the steps of every stream, or (ragged) the rows in all
            post, top, score, is_new = _new_tensors(rows, K, dev, 1)
            if self._has_lengths:
                self.lengths = self._new_lengths(rows)
            res = RaggedScanOutput(None, post, post, top, score, is_new, out.offsets) if ragged else ScanOutput(None, post, post, top, score, is_new)
            if count == 0:                                      # (no rows in all: nothing to launch; the resets stay pending)
                return res
        head = (self._classes, v.data_ptr(), *self._tables(), C.byref(self.detector.det))
        outs = (self.state.data_ptr(), res.probs.data_ptr(), *((self.lengths.data_ptr(),) if self._has_lengths else ()), res.top.data_ptr(),
                res.score.data_ptr(), res.is_new.data_ptr(), stream_of(dev))
        if ragged:
            off_dev = torch.from_numpy(res.offsets).to(dev)
            lib.check(self._push_ragged_c(S, off_dev.data_ptr(), count, *head, self._begin_ragged_reset(), *outs), self._entry + "_push_ragged")
            self._end_ragged_reset(res.steps)
        else:
            lib.check(self._push_c(S, count, *head, self._take_reset(), *outs), self._entry + "_push")
        return res


class StreamingPhraseDetector(_PosteriorStream):
    """`PhraseDetector.detect` over live streams (tcr_phrase_stream_push): `push` takes what a `StreamingDetector` of the same streams
    returned from `push`, `push_many` or `push_ragged` and returns the phrase detections of those steps.  The last window_steps - 1
    rows of every stream's word posteriors and the detector's integers stay on the device, so however the streams are cut into
    pushes, every stream's rows are bitwise `detector.detect` of one scan of everything pushed to it since its start or last `reset`;
    the three forms mix freely.  Build it with `PhraseDetector.streaming(n_streams)`.

    The outputs have `PhraseDetector.detect`'s form over P + 1 classes: logits None, probs and smoothed the phrase posteriors (one
    tensor), top / score / is_new the detector rule.  A `StreamOutput` (one step) gives this object's own [S, ..] tensors, overwritten
    by the next one-step push (copy what must survive it); a `ScanOutput` / `RaggedScanOutput` gives a new one, so outputs
    concatenated over steps go into `PhraseDetector.sweep` / `tune` / `mine` unchanged."""
    _entry = "tcr_phrase_stream"

    def __init__(self, detector: PhraseDetector, n_streams: int):
        words = detector.words
        self._off = np.zeros(len(words) + 1, np.int32)
        np.cumsum([len(q) for q in words], out=self._off[1:])
        self._flat = np.ascontiguousarray(np.array([c for q in words for c in q], np.int32))
        self._cfg = _lib.PhraseCfg(detector.window_steps, int(detector.ordered), PHRASE_COMBINERS[detector.combine])
        super().__init__(detector, n_streams)

    def _tables(self):
        return len(self._off) - 1, self._off.ctypes.data, self._flat.ctypes.data, C.byref(self._cfg)

    def push(self, out, on: str = "smoothed"):
        """The phrase detections of the steps in `out`, what the `StreamingDetector` returned: a `StreamOutput` (`push`: one step ->
        this object's own `StreamOutput`), a `ScanOutput` (`push_many` -> a new `ScanOutput`) or a `RaggedScanOutput` (`push_ragged` ->
        a new `RaggedScanOutput` with out's offsets), read from out's `on` ("smoothed", or "probs").  Pending `reset`s apply before a
        stream's first row of the call.  The call only enqueues kernels."""
        return super().push(out, on)


