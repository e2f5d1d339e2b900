"""Enrolled keywords by template matching on a scan's posteriors, on the device (tcr_dtw_scores): `dtw_scores` over raw tensors,
`KeywordTemplates`, a named set of posterior trajectories cut from recorded examples (`enroll`), and `TemplateDetector`, which matches
them against a `KeywordScanner`'s outputs by subsequence dynamic time warping into posteriors over K keywords and a background class and
runs a `detection.DetectionStage` of K + 1 classes over them: the detector rule, `sweep`, `tune` and `mine`, as `PhraseDetector` does for
phrases -- for words the model was never trained on.  `TemplateDetector.streaming` gives the same detector over the pushes of a
`StreamingDetector` (`StreamingTemplateDetector`, tcr_dtw_stream_push): the DTW column and the detector are carried on the device, so
any way of cutting the streams into pushes gives, bitwise, `detect` of the whole scan."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import TcrError
from .detection import RaggedScanOutput, _first_steps, _last_steps, check_on
from .phrases import BACKGROUND_LABEL, PhraseDetector, _PosteriorStream
from .runtime import stream_of
from .scoring import _offsets


class _Tables:
    """The template tables of a tcr_dtw_* call: the packed frames on the device, the host offset and scale tables, the cfg."""

    def __init__(self, what: str, templates: torch.Tensor, frame_offsets, keyword_offsets, scale, max_steps: int):
        if templates.dtype != torch.float32 or not templates.is_contiguous() or templates.dim() != 2:
            raise TcrError(f"{what} expects contiguous float32 templates [total_frames, F], got {templates.dtype} {tuple(templates.shape)}")
        self.templates = templates
        self.frame_off = np.ascontiguousarray(frame_offsets, np.int32)
        self.kw_off = np.ascontiguousarray(keyword_offsets, np.int32)
        self.scale = np.ascontiguousarray(scale, np.float32)
        if self.frame_off.ndim != 1 or self.kw_off.ndim != 1 or self.frame_off.size < 1 or self.kw_off.size < 1:
            raise TcrError(f"{what}: frame_offsets and keyword_offsets are 1-D tables of Q + 1 and K + 1 entries")
        self.Q, self.K = int(self.frame_off.size) - 1, int(self.kw_off.size) - 1
        if self.scale.shape != (self.Q,):
            raise TcrError(f"{what}: scale has {self.scale.size} entries for {self.Q} templates")
        if self.Q >= 1 and int(self.frame_off[-1]) != int(templates.shape[0]):
            raise TcrError(f"{what}: frame_offsets end at {int(self.frame_off[-1])}, templates hold {int(templates.shape[0])} frames")
        self.cfg = _lib.DtwCfg(int(max_steps))

    def args(self):
        return (self.Q, self.templates.data_ptr(), self.frame_off.ctypes.data, self.K, self.kw_off.ctypes.data, self.scale.ctypes.data,
                C.byref(self.cfg))


def dtw_scores(values: torch.Tensor, templates: torch.Tensor, frame_offsets, keyword_offsets, scale, max_steps: int = 0, step_offsets=None,
               return_lengths: bool = False, lib=None):
    """The raw form of tcr_dtw_scores(_ragged): values float32 on the device, [N, steps, F], or with step_offsets (host int64 [N + 1])
    packed [total_steps, F]; templates float32 on the device, packed [total_frames, F], template q's frames frame_offsets[q] ..
    frame_offsets[q + 1] - 1; keyword k owns templates keyword_offsets[k] .. keyword_offsets[k + 1] - 1; scale [Q] float32.  Returns the
    keyword posteriors, values' shape with K + 1 columns (the last: the background), and with return_lengths also the int32 lengths
    (K columns: the steps the best match spans); see include/tcresnet_hip.h for the score.  The call only enqueues kernels."""
    lib = _lib.get() if lib is None else lib
    ragged = step_offsets is not None
    if values.dtype != torch.float32 or not values.is_contiguous() or values.dim() != (2 if ragged else 3):
        raise TcrError(f"dtw_scores expects contiguous float32 values {'[total_steps, F]' if ragged else '[N, steps, F]'}, got "
                       f"{values.dtype} {tuple(values.shape)}")
    tb = _Tables("dtw_scores", templates, frame_offsets, keyword_offsets, scale, max_steps)
    dev, F = values.device, int(values.shape[-1])
    if int(templates.shape[1]) != F:
        raise TcrError(f"dtw_scores: templates have {int(templates.shape[1])} features, values {F}")
    out = torch.empty((*values.shape[:-1], max(tb.K, 0) + 1), dtype=torch.float32, device=dev)
    lengths = torch.empty((*values.shape[:-1], max(tb.K, 0)), dtype=torch.int32, device=dev) if return_lengths else None
    lptr = lengths.data_ptr() if return_lengths else None
    if ragged:
        soff = _offsets("dtw_scores", "offsets", step_offsets, int(values.shape[0]), int64_only=True)
        if int(values.shape[0]) > 0:
            off_dev = torch.from_numpy(soff).to(dev)
            lib.check(lib.tcr_dtw_scores_ragged(int(soff.size) - 1, off_dev.data_ptr(), int(values.shape[0]), F, values.data_ptr(), *tb.args(),
                                                out.data_ptr(), lptr, stream_of(dev)), "tcr_dtw_scores_ragged")
    else:
        lib.check(lib.tcr_dtw_scores(int(values.shape[0]), int(values.shape[1]), F, values.data_ptr(), *tb.args(), out.data_ptr(), lptr,
                                     stream_of(dev)), "tcr_dtw_scores")
    return (out, lengths) if return_lengths else out


class KeywordTemplates:
    """A named set of templates per keyword: float32 [L, F] posterior trajectories, in enrolment order (keywords in the order of their
    first template).  `enroll` cuts one from a recorded example, `add` takes rows directly; `save` / `load` keep the set as one .npz."""

    def __init__(self):
        self.keywords: Dict[str, List[np.ndarray]] = {}

    @property
    def names(self) -> List[str]:
        return list(self.keywords)

    def __len__(self) -> int:
        return sum(len(v) for v in self.keywords.values())

    def add(self, name: str, rows) -> np.ndarray:
        """A template of keyword `name`: rows float32 [L, F], L >= 1, every template of the set with the same F."""
        name = str(name)
        t = np.ascontiguousarray(rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else rows, np.float32)
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise TcrError(f"KeywordTemplates: a template is float32 [L, F] with L, F >= 1, got {t.shape}")
        if not name or name == BACKGROUND_LABEL:
            raise TcrError(f"KeywordTemplates: {name!r} cannot name a keyword")
        F = self.num_features
        if F is not None and t.shape[1] != F:
            raise TcrError(f"KeywordTemplates: template of {t.shape[1]} features in a set of {F}")
        self.keywords.setdefault(name, []).append(t)
        return t

    @property
    def num_features(self) -> Optional[int]:
        for v in self.keywords.values():
            return int(v[0].shape[1])
        return None

    def enroll(self, scanner, name: str, signal, start_ms: Optional[float] = None, end_ms: Optional[float] = None, on: str = "smoothed",
               max_frames: Optional[int] = None) -> np.ndarray:
        """Scans one example (a 1-D float32 signal, longer than the model's clip; samples behind its last whole step are not read) with
        `scanner` and keeps, as a template of keyword `name`, the `on` ("smoothed", or "probs") rows of the steps whose end times lie in
        [start_ms, end_ms] (default: all rows); of more than max_frames rows every r-th, r the smallest integer that fits (default: the
        largest template the library takes).  Returns the template."""
        check_on("KeywordTemplates.enroll", on)
        st = scanner.stage
        x = signal if isinstance(signal, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(signal, np.float32))
        if x.dim() != 1 or x.dtype != torch.float32:
            raise TcrError(f"KeywordTemplates.enroll: the example is a 1-D float32 signal, got {x.dtype} {tuple(x.shape)}")
        if int(x.shape[0]) <= st.clip_samples:
            raise TcrError(f"KeywordTemplates.enroll: the example has {int(x.shape[0])} samples, it must be longer than the model's clip of "
                           f"{st.clip_samples}")
        steps = int(x.shape[0]) // st.step_samples
        x = x[:steps * st.step_samples].to(scanner.device).contiguous()
        rows = getattr(scanner.scan(x[None]), on)[0].cpu().numpy()
        first = 0 if start_ms is None else int(_first_steps(np.array([float(start_ms)]), st.step_samples, st.sample_rate)[0])
        last = steps - 1 if end_ms is None else min(steps - 1, int(_last_steps(np.array([float(end_ms)]), st.step_samples, st.sample_rate)[0]))
        if last < first:
            raise TcrError(f"KeywordTemplates.enroll: no step of the example ends in [{start_ms}, {end_ms}] ms ({steps} steps of {st.step_ms:g} ms)")
        rows = rows[first:last + 1]
        limit = scanner.lib.tcr_dtw_frames_max(int(rows.shape[1])) if max_frames is None else int(max_frames)
        if limit < 1:
            raise TcrError(f"KeywordTemplates.enroll: max_frames must be >= 1 (got {limit})")
        r = -(-rows.shape[0] // limit)
        return self.add(name, rows[::r])

    def save(self, path: str) -> None:
        """One .npz: `names`, `counts` (templates per keyword) and the templates t0, t1, .. in keyword order."""
        flat = [t for v in self.keywords.values() for t in v]
        np.savez(path, names=np.array(self.names, dtype=np.str_), counts=np.array([len(v) for v in self.keywords.values()], np.int32),
                 **{f"t{i}": t for i, t in enumerate(flat)})

    @classmethod
    def load(cls, path: str) -> "KeywordTemplates":
        self = cls()
        with np.load(path, allow_pickle=False) as z:
            i = 0
            for name, count in zip(z["names"], z["counts"]):
                for _ in range(int(count)):
                    self.add(str(name), z[f"t{i}"])
                    i += 1
        return self


class TemplateDetector(PhraseDetector):
    """Enrolled keywords detected from a scan's posteriors on the device (tcr_dtw_scores): keyword k's score at a step is the best
    confidence of its templates, a template's confidence 1 - its subsequence-DTW cost to the rows that end at the step, the cost the
    mean over the template's frames of the total variation between template frame and row (scale[q] = 0.5 / L_q), in [0, 1].  The
    scores are posteriors over the keywords and a background class, so the keyword stages apply with K + 1 classes: `detect` is the
    detector rule over them, `sweep`, `tune` and `mine` are `PhraseDetector`'s.

    scanner: the `KeywordScanner` whose outputs are matched (a cascade: its second scanner); templates: `KeywordTemplates` of the
    scanner's classes.  A match of more than max_stretch x the longest template's frames scores 0 (the summed cost prefers short
    paths; max_stretch <= 0: no limit).  detection_threshold / suppression_ms: None takes the scanner's; on: the rows `scores`,
    `detect` and the streaming form read by default.  `labels` are the keyword names and "_background_" last."""
    _noun = "template"

    def __init__(self, scanner, templates: KeywordTemplates, detection_threshold: Optional[float] = None, suppression_ms: Optional[float] = None,
                 max_stretch: float = 3.0, on: str = "smoothed"):
        check_on("TemplateDetector", on)
        ncls = scanner.net.num_classes
        if not isinstance(templates, KeywordTemplates) or len(templates) == 0:
            raise TcrError("TemplateDetector: templates is a KeywordTemplates with at least one template")
        if templates.num_features != ncls:
            raise TcrError(f"TemplateDetector: the templates have {templates.num_features} features, the scanner {ncls} classes")
        if len(templates) > _lib.DTW_MAX_TEMPLATES:
            raise TcrError(f"TemplateDetector: {len(templates)} templates (1..{_lib.DTW_MAX_TEMPLATES})")
        self.scanner, self.lib, self.device = scanner, scanner.lib, scanner.device
        self.templates, self.on = templates, on
        self.names = templates.names
        self.labels = self.names + [BACKGROUND_LABEL]
        flat = [t for v in templates.keywords.values() for t in v]
        l_max = self.lib.tcr_dtw_frames_max(ncls)
        for t in flat:
            if t.shape[0] > l_max:
                raise TcrError(f"TemplateDetector: a template of {t.shape[0]} frames is above tcr_dtw_frames_max({ncls}) = {l_max}")
        frame_off = np.zeros(len(flat) + 1, np.int32)
        np.cumsum([t.shape[0] for t in flat], out=frame_off[1:])
        kw_off = np.zeros(len(self.names) + 1, np.int32)
        np.cumsum([len(v) for v in templates.keywords.values()], out=kw_off[1:])
        scale = np.array([np.float32(0.5 / t.shape[0]) for t in flat], np.float32)
        longest = max(t.shape[0] for t in flat)
        self.max_stretch = float(max_stretch)
        self.max_steps = int(math.ceil(self.max_stretch * longest)) if self.max_stretch > 0 else 0
        packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(flat), np.float32)).to(self.device)
        self.tables = _Tables("TemplateDetector", packed, frame_off, kw_off, scale, self.max_steps)
        self._make_stage(detection_threshold, suppression_ms)

    def scores(self, out, on: Optional[str] = None, return_lengths: bool = False):
        """The keyword posteriors of `out` (a `ScanOutput`, `RaggedScanOutput` or `CascadeOutput` of the scanner): float32 shaped like
        out.probs with K + 1 columns, from out's `on`; with return_lengths also the int32 lengths, K columns."""
        v, tb = self._values(out, on), self.tables
        return dtw_scores(v, tb.templates, tb.frame_off, tb.kw_off, tb.scale, self.max_steps,
                          out.offsets if isinstance(out, RaggedScanOutput) else None, return_lengths, self.lib)

    def streaming(self, n_streams: int) -> "StreamingTemplateDetector":
        """This detector over the pushes of a `StreamingDetector` of n_streams streams (`StreamingTemplateDetector`)."""
        return StreamingTemplateDetector(self, n_streams)

    def detect(self, out, on: Optional[str] = None, return_lengths: bool = False):
        """The keyword detections of a scan: the same kind of output object over K + 1 classes -- logits None, probs and smoothed the
        keyword posteriors (one tensor), top / score / is_new the detector rule over them (tcr_detect_redetect with average_steps =
        min_count = 1 and this detector's threshold and suppression): a keyword fires when it is on top above the threshold, and again
        only after the background (or another keyword) has been.  With return_lengths: (that output, the lengths)."""
        ph, lengths = self.scores(out, on, return_lengths=True)
        det = self._detect(out, ph)
        return (det, lengths) if return_lengths else det


class StreamingTemplateDetector(_PosteriorStream):
    """`TemplateDetector.detect` over live streams (tcr_dtw_stream_push): `push` takes what a `StreamingDetector` of the same streams
    returned from `push`, `push_many` or `push_ragged` and returns the keyword detections of those steps.  The DTW column of every
    (stream, template) and the detector's integers stay on the device, so however the streams are cut into pushes, every stream's rows
    are bitwise `detector.detect` of one scan of everything pushed to it since its start or last `reset`; the three forms mix freely.
    Build it with `TemplateDetector.streaming(n_streams)`.

    The outputs have `TemplateDetector.detect`'s form over K + 1 classes, and `lengths` holds the lengths of the last push (the same
    leading shape, K columns).  A `StreamOutput` (one step) gives this object's own [S, ..] tensors, overwritten by the next one-step
    push (copy what must survive it); a `ScanOutput` / `RaggedScanOutput` gives new ones."""
    _entry, _has_lengths = "tcr_dtw_stream", True

    def _tables(self):
        return self.detector.tables.args()

    def push(self, out, on: Optional[str] = None):
        """The keyword detections of the steps in `out`, what the `StreamingDetector` returned: a `StreamOutput` (`push`: one step ->
        this object's own `StreamOutput`), a `ScanOutput` (`push_many` -> a new `ScanOutput`) or a `RaggedScanOutput` (`push_ragged` ->
        a new `RaggedScanOutput` with out's offsets), read from out's `on`; `lengths` is set to the call's lengths.  Pending `reset`s
        apply before a stream's first row of the call.  The call only enqueues kernels."""
        return super().push(out, on)
