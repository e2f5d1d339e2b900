"""The detection stage (tcresnet_amd.detection.DetectionStage): built by hand, with no model anywhere, it redetects, sweeps and tunes
bitwise like a `KeywordScanner` with the same settings; `PhraseDetector.detect` is its `redetect` without a smoothed vector over the
phrase posteriors; and every name of `scanning` / `streaming` is the object of its new home.  Emulator (`-m "not gpu"`) and MI355X
(`-m gpu`)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_streaming import setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP, RATE, CLIP = 320, 16000, 16000                       # a 20 ms step, one second of clip
STEP_MS = 1000.0 * STEP / RATE
THRESHOLDS = (-np.inf, 0.4, 0.7, np.inf)
RAGGED_STEPS = (5, 0, 9)                                   # (a signal without steps in the middle)


def softmax_rows(lib, shape, seed):
    z = np.random.RandomState(seed).randn(*shape) * 2.0
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return Cm.to_dev(lib, e / e.sum(axis=-1, keepdims=True))


def outputs(lib, ncls):
    """Posteriors-only outputs, dense [2, 12, ncls] and ragged over RAGGED_STEPS, and per signal its steps."""
    from tcresnet_amd.detection import RaggedScanOutput, ScanOutput
    dense = ScanOutput(None, softmax_rows(lib, (2, 12, ncls), 5), None, None, None, None)
    off = np.concatenate([[0], np.cumsum(RAGGED_STEPS)]).astype(np.int64)
    ragged = RaggedScanOutput(None, softmax_rows(lib, (int(off[-1]), ncls), 6), None, None, None, None, off)
    return (dense, [12, 12]), (ragged, list(RAGGED_STEPS))


def events_of(det, steps):
    """Two events per signal with steps (none for one without): steps 1..2 and the last two steps, so the second ends on the signal's
    last step; each labelled with the detector's top at its end (class 0 before min_count).  Times in ms: step i ends at (i + 1) * 20."""
    events = []
    for n, m in enumerate(steps):
        top = (det.signal(n).top[0] if hasattr(det, "offsets") else det.top[n]).cpu().numpy()
        spans = [(1, 2), (m - 2, m - 1)] if m else []
        events.append([((a + 1) * STEP_MS, (b + 1) * STEP_MS, max(int(top[b]), 0)) for a, b in spans])
    return events


def same_fields(got, want, fields):
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        if isinstance(w, torch.Tensor):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f
        else:
            assert np.array_equal(g, w, equal_nan=True), f


def check_stage_equals_scanner(lib):
    from tcresnet_amd.detection import DetectionStage
    from tcresnet_amd.scanning import KeywordScanner
    fe, net, _, _, _ = setup(lib)
    sc = KeywordScanner(net, fe, average_window_ms=3 * STEP_MS, min_count=2, detection_threshold=0.3, suppression_ms=4 * STEP_MS)
    ncls = net.num_classes
    assert isinstance(sc.stage, DetectionStage) and sc.stage.det is sc.det
    assert (sc.step_samples, sc.det.average_steps, sc.det.min_count, sc.det.suppression_steps) == (STEP, 3, 2, 4)
    del fe, net                                           # the stage below is told numbers, never a model
    stage = DetectionStage(lib, Cm.device_of(lib), ncls, STEP, RATE, CLIP, T._lib.DetectCfg(3, 2, 4, 0.3))
    assert stage.step_ms == sc.step_ms == STEP_MS
    for out, steps in outputs(lib, ncls):
        # redetect: the own settings (in steps), and others given in ms
        for kw in ({}, dict(average_window_ms=2 * STEP_MS, min_count=1, detection_threshold=0.2, suppression_ms=1 * STEP_MS)):
            got, want = stage.redetect(out, **kw), sc.redetect(out, **kw)
            assert type(got) is type(want) and got.probs is out.probs and got.logits is None and got.smoothed is not got.probs
            same_fields(got, want, ("smoothed", "top", "score", "is_new"))
        got, want = stage.redetect(out), sc.redetect(out)
        assert int(want.is_new.sum()) > 0
        # sweep: an event that ends on the signal's last step, a signal without steps
        events = events_of(want, steps)
        a = stage.sweep(got, THRESHOLDS, events=events, tolerance_ms=0.0, return_fired=True)
        b = sc.sweep(want, THRESHOLDS, events=events, tolerance_ms=0.0, return_fired=True)
        same_fields(a, b, a._fields)
        assert int(b.hits.sum()) > 0 and int(b.fired[0].sum()) > int(b.fired[-1].sum()) == 0
        assert stage.event_steps(want, events, None, 0.0)[2][0][1].tolist()[:2] == [steps[0] - 2, steps[0] - 1]
        # tune: 2 windows x 2 min_count x 2 suppressions; min_count 2 does not fit the one-step window
        grid = dict(average_window_ms=(1 * STEP_MS, 3 * STEP_MS), min_count=(1, 2), suppression_ms=(0, 4 * STEP_MS), events=events,
                    tolerance_ms=0.0)
        a, b = stage.tune(out, THRESHOLDS, **grid), sc.tune(out, THRESHOLDS, **grid)
        assert a.points == b.points and a.dropped == b.dropped and len(b.points) == 6
        assert [p.steps for p in b.dropped] == [(1, 2, 0), (1, 2, 4)]
        same_fields(a, b, ("detections", "hits", "duplicates", "thresholds", "events", "hours"))
        assert int(b.detections.sum()) > 0


def check_phrase_detect_is_the_stages_redetect(lib):
    from tcresnet_amd.detection import CascadeOutput, DetectionStage, RaggedScanOutput, ScanOutput
    from tcresnet_amd.scanning import KeywordScanner, PhraseDetector
    fe, net, _, _, _ = setup(lib)
    sc = KeywordScanner(net, fe, average_window_ms=3 * STEP_MS, min_count=2, detection_threshold=0.3, suppression_ms=4 * STEP_MS)
    ph = PhraseDetector(sc, [[2, 3], [3, 2]], window_ms=5 * STEP_MS, detection_threshold=0.05, suppression_ms=3 * STEP_MS)
    assert isinstance(ph.stage, DetectionStage) and ph.stage is not sc.stage and ph.stage.num_classes == 3 and ph.stage.det is ph.det
    stage = DetectionStage(lib, Cm.device_of(lib), 3, STEP, RATE, CLIP, T._lib.DetectCfg(1, 1, 3, 0.05))
    (dense, _), (ragged, _) = outputs(lib, net.num_classes)
    dense = ScanOutput(None, dense.probs, dense.probs, None, None, None)
    r = (None, ragged.probs, ragged.probs, None, None, None, ragged.offsets)
    ragged = RaggedScanOutput(*r)
    cascade = CascadeOutput(*r, torch.zeros(0, dtype=torch.int64), ragged)
    fired = 0
    for out in (dense, ragged, cascade):
        det = ph.detect(out)
        assert type(det) is type(out) and det.logits is None and det.probs is det.smoothed
        post = ph.scores(out)
        assert torch.equal(det.probs, post)
        bare = ScanOutput(None, post, None, None, None, None) if out is dense else RaggedScanOutput(None, post, None, None, None, None, out.offsets)
        want = stage.redetect(bare, smoothed=False)
        assert want.probs is post and want.smoothed is post and want.logits is None
        same_fields(det, want, ("top", "score", "is_new"))
        fired += int(det.is_new.sum())
    assert fired > 0
    assert det.selected is cascade.selected and det.first is ragged and np.array_equal(det.offsets, ragged.offsets)
    # no rows in all: empty tensors and no call (the library refuses one, as the scanner's and the stage's redetect show)
    probs = torch.empty((0, net.num_classes), dtype=torch.float32, device=Cm.device_of(lib))
    empty = RaggedScanOutput(None, probs, probs, None, None, None, np.zeros(3, np.int64))
    det = ph.detect(empty)
    assert isinstance(det, RaggedScanOutput) and det.logits is None and det.probs is det.smoothed and tuple(det.probs.shape) == (0, 3)
    assert [(tuple(t.shape), t.dtype) for t in (det.top, det.score, det.is_new)] == [((0,), torch.int32), ((0,), torch.float32), ((0,), torch.int32)]
    with pytest.raises(T.TcrError):
        stage.redetect(RaggedScanOutput(None, det.probs, None, None, None, None, empty.offsets), smoothed=False)
    with pytest.raises(T.TcrError):
        sc.redetect(empty)


# ---- emulator --------------------------------------------------------------------------------------------------------------------
def test_stage_built_by_hand_equals_scanner(emu_lib):
    check_stage_equals_scanner(emu_lib)


def test_phrase_detect_is_the_stages_redetect(emu_lib):
    check_phrase_detect_is_the_stages_redetect(emu_lib)


# ---- CPU only, no library --------------------------------------------------------------------------------------------------------
# the public names of scanning.py and streaming.py before the split, by the module each lives in now
HOMES = {
    "scanning": {"detection": ["DEFAULT_MAX_WINDOWS", "ScanOutput", "RaggedScanOutput", "CascadeOutput", "ms_to_steps"],
                 "scoring": ["SweepResult", "detection_sweep", "GridPoint", "GridResult", "detection_grid"],
                 "mining": ["MINE_KINDS", "MinedDetections", "mine_detections", "MinedPeaks", "mine_peaks", "select_top", "gather_clips",
                            "MinedClips"],
                 "phrases": ["BACKGROUND_LABEL", "PHRASE_COMBINERS", "phrase_scores", "PhraseSweepResult", "PhraseGridResult", "PhraseDetector"],
                 "scanning": ["DEFAULT_MAX_SIGNALS", "KeywordScanner", "select_steps", "CascadeScanner"],
                 "streaming": ["Network"], "engine": ["Frontend"], "_lib": ["TcrError"]},
    "streaming": {"detection": ["ms_to_steps"], "streaming": ["StreamOutput", "StreamingDetector", "Network"],
                  "engine": ["Frontend", "TCResNet", "DSCNN", "Graph2D"], "_lib": ["TcrError", "ModelRef", "padded_len"]},
}


def test_every_name_is_its_new_homes_object():
    import importlib
    mod = lambda name: importlib.import_module(f"tcresnet_amd.{name}")
    for old, homes in HOMES.items():
        for home, names in homes.items():
            for name in names:
                assert getattr(mod(old), name) is getattr(mod(home), name), (old, home, name)
    for gone in ("_PhraseView", "_PhraseClasses"):
        assert not hasattr(mod("scanning"), gone) and not hasattr(mod("phrases"), gone)
    assert not hasattr(mod("streaming")._Detection, "_sweep_inputs")


def test_streaming_imports_without_scanning():
    code = ("import sys, tcresnet_amd.streaming as St; St.StreamingDetector.sweep; "
            "print(sorted(m for m in sys.modules if m.startswith('tcresnet_amd.')))")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "tcresnet_amd.detection" in run.stdout and "tcresnet_amd.streaming" in run.stdout
    assert "tcresnet_amd.scanning" not in run.stdout and "tcresnet_amd.phrases" not in run.stdout


# ---- MI355X ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_stage_built_by_hand_equals_scanner(hip_lib):
    check_stage_equals_scanner(hip_lib)


@pytest.mark.gpu
def test_gpu_phrase_detect_is_the_stages_redetect(hip_lib):
    check_phrase_detect_is_the_stages_redetect(hip_lib)
