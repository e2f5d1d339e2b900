"""Detector tuning from one scan (tcr_detect_redetect, tcr_detect_grid, KeywordScanner.redetect / tune, tune_audio.py): the detector
tail run again on stored probabilities is bitwise the scan with those settings, and a grid's counts are the per-point sweeps'.
Emulator (`-m "not gpu"`) and MI355X (`-m gpu`): the checks against the NumPy rule are functions of `lib` and run on both."""
import csv
import ctypes as C
import io
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import scanning
from tests.test_streaming import frozen_artifact, segment_audio, setup, write_wav
from tests.test_sweep import fast_sweep, random_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = T._lib.GRID_TILE


def w_max(ncls):
    """The largest window of the LDS-staged kernel (include/tcresnet_hip.h, tcr_detect_grid)."""
    return 16128 // ncls - (TILE - 1)


# ---- the rule, restated (include/tcresnet_hip.h, tcr_stream_step) ------------------------------------------------------------------
def np_detect(probs, W, mc, supp, thr):
    """probs [steps, C] float32 of one signal -> smoothed, top, score, is_new of a fresh detector."""
    steps, ncls = probs.shape
    i = np.arange(steps)
    count = np.minimum(i + 1, W)
    acc = np.zeros((steps, ncls), np.float32)
    for q in range(min(W, steps)):                      # float32 adds, oldest to newest
        m = q < count
        acc[m] = acc[m] + probs[(i - count + 1 + q)[m]]
    sm = acc * (np.float32(1) / count.astype(np.float32))[:, None]
    best = np.argmax(sm, axis=1).astype(np.int32)       # (the lowest index on ties)
    warm = count >= mc
    top = np.where(warm, best, -1).astype(np.int32)
    score = np.where(warm, sm[i, best], np.float32(0)).astype(np.float32)
    new = np.zeros(steps, np.int32)
    prev, pstep = -1, 0
    for s in range(steps):
        if top[s] >= 0 and score[s] > np.float32(thr) and top[s] != prev and (prev == -1 or s - pstep > supp):
            prev, pstep, new[s] = int(top[s]), s, 1
    return sm, top, score, new


def softmax_rows(rng, steps, ncls, runs=False):
    """Random softmax rows; runs: a dominant class that changes every 10 .. 80 steps, so that the smoothed top moves."""
    x = rng.randn(steps, ncls).astype(np.float32)
    if runs:
        pos = 0
        while pos < steps:
            m = int(rng.randint(10, 80))
            x[pos:pos + m, rng.randint(ncls)] += rng.uniform(1.0, 4.0)
            pos += m
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def rows_with_events(rng, steps, ncls):
    """Softmax rows whose dominant class goes a, b, a (b for a short while) and then rests, and for most such triples an event of
    label a over all of it (inclusive steps, disjoint, sorted): a hit, a false accept inside an event and a duplicate are all there
    for a detector that follows the dominant class."""
    x = rng.randn(steps, ncls).astype(np.float32)
    events, pos = [], 0
    while pos < steps:
        a, b = (int(c) for c in rng.choice(ncls, 2, replace=False))
        la, lb, start = int(rng.randint(20, 60)), int(rng.randint(12, 30)), pos
        for c, m in ((a, la), (b, lb), (a, la)):
            x[pos:pos + m, c] += rng.uniform(2.0, 4.0)
            pos += m
        if rng.rand() < 0.7 and start + 1 < steps:
            events.append((start + 1, min(pos, steps) - 1, a))
        pos += int(rng.randint(5, 30))
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), events


def redetect_lib(lib, probs, det, offsets=None, smoothed=True):
    """tcr_detect_redetect(_ragged) on host arrays -> (smoothed or None, top, score, is_new) as NumPy."""
    dev = Cm.device_of(lib)
    p = torch.from_numpy(np.ascontiguousarray(probs)).to(dev)
    ncls = p.shape[-1]
    rows = p.shape[:-1]
    sm = torch.full(p.shape, -7.0, device=dev)
    top, new = torch.full(rows, -9, dtype=torch.int32, device=dev), torch.full(rows, -9, dtype=torch.int32, device=dev)
    sc = torch.full(rows, -7.0, device=dev)
    d = T._lib.DetectCfg(*det)
    smp = sm.data_ptr() if smoothed else None
    if offsets is None:
        rc = lib.tcr_detect_redetect(p.shape[0], p.shape[1], ncls, p.data_ptr(), C.byref(d), smp, top.data_ptr(), sc.data_ptr(), new.data_ptr(),
                                     None)
    else:
        off = torch.from_numpy(np.asarray(offsets, np.int64)).to(dev)
        rc = lib.tcr_detect_redetect_ragged(len(offsets) - 1, off.data_ptr(), p.shape[0], ncls, p.data_ptr(), C.byref(d), smp, top.data_ptr(),
                                            sc.data_ptr(), new.data_ptr(), None)
    lib.check(rc, "redetect")
    return sm.cpu().numpy(), top.cpu().numpy(), sc.cpu().numpy(), new.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))


# ---- 1. redetect against the rule ------------------------------------------------------------------------------------------------------
def check_redetect_equals_numpy_rule(lib, ncls):
    N, steps = 3, 70
    rng = np.random.RandomState(100 + ncls)
    probs = np.stack([softmax_rows(rng, steps, ncls, runs=True) for _ in range(N)])
    thr = 1.2 / ncls
    for W in (1, 3, 50):
        for mc in sorted({1, W}):
            for supp in (0, 7):
                want = [np.stack(x) for x in zip(*(np_detect(probs[n], W, mc, supp, thr) for n in range(N)))]
                got = redetect_lib(lib, probs, (W, mc, supp, thr))
                for name, g, w in zip(("smoothed", "top", "score", "is_new"), got, want):
                    assert_same(g, w, (name, W, mc, supp))
                assert want[3].sum() >= N
                nov = redetect_lib(lib, probs, (W, mc, supp, thr), smoothed=False)
                assert (nov[0] == -7.0).all()                                    # smoothed == NULL: not written
                for g, w in zip(nov[1:], want[1:]):
                    assert_same(g, w, ("no smoothed", W, mc, supp))


@pytest.mark.parametrize("ncls", [3, 5, 12])
def test_redetect_equals_numpy_rule(emu_lib, ncls):
    check_redetect_equals_numpy_rule(emu_lib, ncls)


# ---- 2. redetect of a real scan -------------------------------------------------------------------------------------------------------
DET_A = dict(average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=200)
DET_B = dict(average_window_ms=240, min_count=3, detection_threshold=0.1, suppression_ms=60)
REDETECTED = ("smoothed", "top", "score", "is_new")


def check_redetect_of_scan(lib, fe, net, audio, k, ragged_steps):
    Sc = scanning()
    a, b = Sc.KeywordScanner(net, fe, frames_per_step=k, **DET_A), Sc.KeywordScanner(net, fe, frames_per_step=k, **DET_B)
    x = Cm.to_dev(lib, audio)
    out_a, want = a.scan(x), b.scan(x)
    got = a.redetect(out_a, **DET_B)
    assert isinstance(got, Sc.ScanOutput) and got.probs is out_a.probs and got.logits is out_a.logits
    assert torch.equal(out_a.probs, want.probs)
    for f in REDETECTED:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
        assert getattr(got, f) is not getattr(out_a, f)
    same = a.redetect(out_a)                                                     # None: the scanner's own settings
    for f in REDETECTED:
        assert torch.equal(getattr(same, f), getattr(out_a, f)), f
    step = a.step_samples
    sig = [x[n % x.shape[0], :m * step].contiguous() for n, m in enumerate(ragged_steps)]
    rag_a, rag_want = a.scan_ragged(sig), b.scan_ragged(sig)
    rag = a.redetect(rag_a, **DET_B)
    assert isinstance(rag, Sc.RaggedScanOutput) and rag.probs is rag_a.probs and np.array_equal(rag.offsets, rag_a.offsets)
    for f in REDETECTED:
        assert torch.equal(getattr(rag, f), getattr(rag_want, f)), f
    return want, rag_want


@pytest.mark.parametrize("k", [1, 3])
def test_redetect_of_scan_equals_other_scan_4020(emu_lib, k):
    fe, net, _, _, _ = setup(emu_lib)
    audio = segment_audio(2, 24960, 41)                   # 78 steps at k = 1, 26 at k = 3
    want, rag = check_redetect_of_scan(emu_lib, fe, net, audio, k, [20 // k + 5, 0, 1, 2, 26])     # 2 < min_count = 3
    assert int(want.is_new.sum()) >= 1 and int(rag.is_new.sum()) >= 1
    assert int((rag.signal(3).top == -1).sum()) == 2


# ---- 3. ragged isolation ---------------------------------------------------------------------------------------------------------------
def grid_lib(lib, probs, points, thr, offsets=None, events=None, valid=None, ws=None):
    Sc = scanning()
    p = torch.from_numpy(np.ascontiguousarray(probs)).to(Cm.device_of(lib))
    d, h, u = Sc.detection_grid(p, points, thr, p.shape[-1], events=events, step_offsets=offsets, valid_steps=valid, lib=lib,
                                workspace_bytes=ws)[:3]
    return d.cpu().numpy(), h.cpu().numpy(), u.cpu().numpy()


def check_ragged_signal_never_reads_its_predecessor(lib):
    ncls, W = 12, 9
    rng = np.random.RandomState(7)
    lens = [TILE + 30, TILE + 5]
    probs = np.concatenate([softmax_rows(rng, m, ncls, runs=True) for m in lens])
    probs[lens[0] - W:lens[0]] = np.nan
    off = [0, lens[0], sum(lens)]
    det, thr = (W, 2, 5, 0.2), [0.1, 0.2, 0.3]
    points = [(W, 2, 5), (W, 1, 0), (3, 1, 5)]
    got = redetect_lib(lib, probs, det, offsets=off)
    alone = redetect_lib(lib, probs[None, lens[0]:], det)
    for g, a in zip(got, alone):
        assert not np.isnan(g[lens[0]:].astype(np.float64)).any()
        assert_same(g[lens[0]:], a[0])
    assert np.isnan(got[0][lens[0] - 1]).all()            # (the poison is where it was put)
    grid = grid_lib(lib, probs, points, thr, offsets=off)
    grid_alone = grid_lib(lib, probs[None, lens[0]:], points, thr)
    for g, a in zip(grid, grid_alone):
        assert np.array_equal(g[:, 1], a[:, 0])
    assert grid_alone[0].sum() > 0


def test_ragged_signal_never_reads_its_predecessor(emu_lib):
    check_ragged_signal_never_reads_its_predecessor(emu_lib)


# ---- 4. the grid equals the per-point sweeps -------------------------------------------------------------------------------------------
def reference_tables(sigs, points, thr, events):
    """Per point, the NumPy rule's top / score and the reference sweep over them: [J] of (detections, hits, duplicates) [N, T, C]."""
    ncls = sigs[0].shape[1]
    longest = max(len(s) for s in sigs)
    out = []
    for W, mc, supp in points:
        top, score = np.full((len(sigs), longest), -1, np.int32), np.zeros((len(sigs), longest), np.float32)
        for n, s in enumerate(sigs):
            if len(s):
                _, top[n, :len(s)], score[n, :len(s)], _ = np_detect(s, W, mc, supp, np.inf)
        out.append(fast_sweep(top, score, thr, supp, ncls, [len(s) for s in sigs], events, want_fired=False)[:3])
    return out


def assert_inputs_discriminate(points, tables):
    """The conditions on the inputs, on the reference side: the tables differ between points, every count occurs, and suppression and
    min_count each change a table on their own."""
    flat = [np.concatenate([x.ravel() for x in t]) for t in tables]
    assert len({f.tobytes() for f in flat}) >= 3
    for q in range(3):
        assert sum(int(t[q].sum()) for t in tables) > 0
    only = lambda axis: any(flat[a].tobytes() != flat[b].tobytes() for a in range(len(points)) for b in range(len(points))
                            if all((points[a][x] == points[b][x]) != (x == axis) for x in range(3)))
    assert only(2) and only(1)


def check_grid(lib, ncls, windows, seed, lens_ragged, thr, steps=2 * TILE + 1):
    rng = np.random.RandomState(seed)
    points = [p for p in itertools.product(windows, (1, 3), (0, 25)) if p[1] <= p[0]]
    # dense with valid_steps (its edges 0, 1 and steps among them)
    valid = [0, 1, TILE - 1, TILE, TILE + 1, steps]
    made = [rows_with_events(rng, steps, ncls) for _ in valid]
    dense, events = np.stack([m[0] for m in made]), [m[1] for m in made]
    want = reference_tables([dense[n, :v] for n, v in enumerate(valid)], points, thr, events)
    assert_inputs_discriminate(points, want)
    got = grid_lib(lib, dense, points, thr, events=events, valid=valid)
    Sc = scanning()
    for j, (W, mc, supp) in enumerate(points):
        for q in range(3):
            assert np.array_equal(got[q][j], want[j][q]), (j, q)
        _, top, score, _ = redetect_lib(lib, dense, (W, mc, supp, 0.5))
        dev = Cm.device_of(lib)
        res = Sc.detection_sweep(torch.from_numpy(top).to(dev), torch.from_numpy(score).to(dev), thr, supp, ncls, events=events,
                                 valid_steps=valid, lib=lib)
        for q, r in enumerate((res.detections, res.hits, res.duplicates)):
            assert np.array_equal(got[q][j], r.cpu().numpy()), (j, q)
    # ragged
    made = [rows_with_events(rng, m, ncls) for m in lens_ragged]
    sigs, events = [m[0] for m in made], [m[1] for m in made]
    off = np.concatenate([[0], np.cumsum(lens_ragged)])
    want = reference_tables(sigs, points, thr, events)
    assert_inputs_discriminate(points, want)
    packed = np.concatenate(sigs)
    got = grid_lib(lib, packed, points, thr, offsets=off, events=events)
    for j, (W, mc, supp) in enumerate(points):
        for q in range(3):
            assert np.array_equal(got[q][j], want[j][q]), (j, q)
        _, top, score, _ = redetect_lib(lib, packed, (W, mc, supp, 0.5), offsets=off)
        dev = Cm.device_of(lib)
        res = Sc.detection_sweep(torch.from_numpy(top).to(dev), torch.from_numpy(score).to(dev), thr, supp, ncls, events=events,
                                 step_offsets=off, lib=lib)
        for q, r in enumerate((res.detections, res.hits, res.duplicates)):
            assert np.array_equal(got[q][j], r.cpu().numpy()), (j, q)


RAGGED_LENS = [TILE - 1, 0, TILE, 1, TILE + 1, 2 * TILE + 1]
GRID_THR = [0.1, 0.2, 0.3, 0.45, 2.0]


def check_grid_at_the_lds_limit_and_above(lib):
    """60 classes: W = 13 is the last window the LDS-staged kernel takes, W = 14 the first of the per-pair path."""
    assert w_max(60) == 13 and w_max(12) == 1089
    check_grid(lib, 60, (13, 14), 22, RAGGED_LENS, [0.02, 0.05, 0.1, 0.2])


def check_grid_eight_wide_body_and_long_halo(lib):
    """Windows around the eight-at-a-time body of smooth_mean, and one whose halo (W - 1 = 256 rows) is longer than a tile."""
    check_grid(lib, 12, (7, 8, 9, 257), 23, RAGGED_LENS + [3 * TILE + 1], GRID_THR, steps=3 * TILE + 1)


def test_grid_equals_per_point_sweeps(emu_lib):
    check_grid(emu_lib, 12, (3, 50), 21, RAGGED_LENS, GRID_THR)


def test_grid_at_the_lds_limit_and_above(emu_lib):
    check_grid_at_the_lds_limit_and_above(emu_lib)


def test_grid_eight_wide_body_and_long_halo(emu_lib):
    check_grid_eight_wide_body_and_long_halo(emu_lib)


# ---- 5. workspace batching ---------------------------------------------------------------------------------------------------------------
def check_grid_workspace_batches(lib):
    ncls = 12
    rng = np.random.RandomState(5)
    probs = np.stack([softmax_rows(rng, TILE + 40, ncls, runs=True) for _ in range(2)])
    points = [(3, 1, 0), (3, 3, 0), (20, 1, 9), (20, 3, 9), (50, 3, 0)]
    thr = [0.1, 0.25]
    total = probs.shape[0] * probs.shape[1]
    full, one = lib.tcr_detect_grid_workspace_bytes(total, len(points)), lib.tcr_detect_grid_workspace_bytes(total, 1)
    assert full == len(points) * one and one >= 8 * total
    a, b, c = grid_lib(lib, probs, points, thr, ws=full), grid_lib(lib, probs, points, thr, ws=one), grid_lib(lib, probs, points, thr, ws=2 * one)
    assert a[0].sum() > 0
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    with pytest.raises(T.TcrError, match="status -3.*workspace"):
        grid_lib(lib, probs, points, thr, ws=one - 1)
    assert lib.tcr_detect_grid_workspace_bytes(0, 1) == 0 and lib.tcr_last_error()
    assert lib.tcr_detect_grid_workspace_bytes(10, 0) == 0 and lib.tcr_last_error()


def test_grid_workspace_batches(emu_lib):
    check_grid_workspace_batches(emu_lib)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_redetect_and_grid_refusals(emu_lib):
    lib = emu_lib
    inp = torch.full((1 << 12,), 0.25)
    out = torch.full((1 << 14,), -3.0)
    off = torch.tensor([0, 16], dtype=torch.int64)
    p, o = inp.data_ptr(), out.data_ptr()
    P = T._lib.DetectPoint

    def refused(rc, msg, kw):
        assert rc == -1, kw
        assert msg in lib.tcr_last_error() and lib.tcr_last_error(), (kw, lib.tcr_last_error())
        assert bool((out == -3.0).all()), kw                  # nothing was launched

    def redetect(n=1, steps=16, ncls=4, probs=p, det=(4, 2, 0, 0.5), top=o, score=o, new=o, ragged=False, offs=off.data_ptr()):
        d = C.byref(T._lib.DetectCfg(*det)) if det is not None else None
        if ragged:
            return lib.tcr_detect_redetect_ragged(n, offs, steps, ncls, probs, d, o, top, score, new, None)
        return lib.tcr_detect_redetect(n, steps, ncls, probs, d, o, top, score, new, None)

    cases = [(dict(probs=None), b"null argument"), (dict(det=None), b"null argument"), (dict(top=None), b"null argument"),
             (dict(score=None), b"null argument"), (dict(new=None), b"null argument"), (dict(n=0), b"number of signals must be positive"),
             (dict(steps=0), b"number of steps must be positive"), (dict(ncls=0), b"num_classes 0 outside"),
             (dict(ncls=257), b"num_classes 257 outside"), (dict(det=(0, 1, 0, 0.5)), b"average_steps"),
             (dict(det=(4, 0, 0, 0.5)), b"min_count 0 outside"), (dict(det=(4, 5, 0, 0.5)), b"min_count 5 outside"),
             (dict(det=(4, 2, -1, 0.5)), b"suppression_steps must be >= 0"), (dict(steps=1 << 29, ncls=4), b"too large")]
    for ragged in (False, True):
        for kw, msg in cases:
            refused(redetect(ragged=ragged, **kw), msg, (ragged, kw))
    refused(redetect(ragged=True, offs=None), b"null argument", "offsets")
    refused(redetect(n=1 << 10, steps=1 << 19, ncls=4), b"too large", "dense product")

    def grid(n=1, steps=16, offs=None, total=None, ncls=4, probs=p, valid=None, pts=((4, 2, 0),), npts=None, nthr=1, thr=p, ev=None, det=o,
             hits=o, ws=o, ws_bytes=1 << 15):
        arr = (P * max(len(pts), 1))(*(P(*x) for x in pts)) if pts is not None else None
        total = (16 if offs is not None else n * steps) if total is None else total
        return lib.tcr_detect_grid(n, steps, offs, total, ncls, probs, valid, len(pts) if npts is None else npts, arr, nthr, thr, ev, p, p, p, det,
                                   hits, o, ws, ws_bytes, None)

    gcases = [(dict(probs=None), b"null argument"), (dict(pts=None, npts=1), b"null argument"), (dict(ws=None), b"null argument"),
              (dict(thr=None), b"null argument"), (dict(det=None), b"null argument"), (dict(npts=0), b"number of points must be positive"),
              (dict(n=0), b"number of signals must be positive"), (dict(steps=0), b"number of steps must be positive"),
              (dict(nthr=0), b"number of thresholds must be positive"), (dict(ncls=0), b"num_classes 0 outside"),
              (dict(ncls=257), b"num_classes 257 outside"), (dict(ev=p, hits=None), b"events need"),
              (dict(pts=((4, 2, 0), (0, 1, 0))), b"average_steps"), (dict(pts=((4, 2, 0), (4, 5, 0))), b"min_count 5 outside"),
              (dict(pts=((4, 0, 0),)), b"min_count 0 outside"), (dict(pts=((4, 2, -1),)), b"suppression_steps must be >= 0"),
              (dict(steps=1 << 29), b"too large"), (dict(pts=((4, 2, 0),) * 1024, n=1 << 10, nthr=1 << 10, ncls=4), b"too large"),
              (dict(n=1 << 12, nthr=1 << 12, ncls=200), b"too large")]
    for kw, msg in gcases:
        refused(grid(**kw), msg, kw)
        if "n" not in kw and "steps" not in kw:
            refused(grid(offs=off.data_ptr(), **kw), msg, ("ragged", kw))
    refused(grid(offs=off.data_ptr(), valid=p), b"valid_steps given together with step_offsets", "valid + offsets")
    refused(grid(total=17), b"total_steps 17 is not", "total")
    refused(grid(offs=off.data_ptr(), total=0), b"number of steps must be positive", "ragged total")
    assert grid() == 0 and redetect() == 0 and grid(offs=off.data_ptr()) == 0 and redetect(ragged=True) == 0
    assert not bool((out == -3.0).all())


# ---- 7. KeywordScanner.tune ----------------------------------------------------------------------------------------------------------------
def test_scanner_tune_best_equals_brute_force(emu_lib):
    Sc = scanning()
    fe, net, _, _, _ = setup(emu_lib)
    sc = Sc.KeywordScanner(net, fe, average_window_ms=100, min_count=2, detection_threshold=0.3, suppression_ms=200)     # 20 ms steps
    rng = np.random.RandomState(12)
    N, steps, ncls = 2, 700, 12
    made = [rows_with_events(rng, steps, ncls) for _ in range(N)]
    probs = torch.from_numpy(np.stack([m[0] for m in made]))
    out = Sc.ScanOutput(None, probs, None, None, None, None)
    events = [[(20.0 * (f + 1), 20.0 * (l + 1), c) for f, l, c in m[1] if f < 600] for m in made]     # step i ends at 20 (i + 1) ms
    thr = np.arange(0.1, 0.6, 0.05)
    axes = dict(average_window_ms=(40, 100, 1000), min_count=(1, 3), suppression_ms=(0, 500))
    kw = dict(events=events, lengths=[steps * 320, 600 * 320 + 17], tolerance_ms=100.0)
    res = sc.tune(out, thr, **axes, **kw)
    dropped = [(40.0, 3, 0.0), (40.0, 3, 500.0)]                                  # a window of 2 steps
    assert [(p.average_window_ms, p.min_count, p.suppression_ms) for p in res.dropped] == dropped
    want_points = [p for p in itertools.product(*axes.values()) if p not in dropped]
    assert [(p.average_window_ms, p.min_count, p.suppression_ms) for p in res.points] == want_points and len(res) == 10
    assert [p.steps for p in res.points[:2]] == [(2, 1, 0), (2, 1, 25)] and res.points[-1].steps == (50, 3, 25)
    brute = []
    for j, (w, mc, sp) in enumerate(want_points):
        # (sweep walks with its scanner's own suppression: a scanner of the point's settings does the point's walk)
        pt = Sc.KeywordScanner(net, fe, average_window_ms=w, min_count=mc, suppression_ms=sp)
        one = pt.sweep(pt.redetect(out), thr, **kw)
        r = res.result(j)
        for f in ("detections", "hits", "duplicates"):
            assert torch.equal(getattr(r, f), getattr(one, f)), (j, f)
        assert np.array_equal(r.events, one.events) and np.allclose(r.hours, one.hours) and r.fired is None
        brute.append(one)
    assert int(res.hits.sum()) > 0 and len({res.result(j).detections.numpy().tobytes() for j in range(len(res))}) >= 3
    for budget, classes in ((1e9, None), (20000.0, None), (3000.0, [1, 2, 3, 5, 7])):
        best = None
        for j, one in enumerate(brute):
            op = one.operating_point(budget, classes)
            if op is not None and (best is None or (op["frr"], op["fa_per_hour"]) < (best[1]["frr"], best[1]["fa_per_hour"])):
                best = (j, op)
        got = res.best(budget, classes)
        assert best is not None and got is not None
        assert got["index"] == best[0] and got["point"] == res.points[best[0]]
        assert {k: got[k] for k in best[1]} == best[1]
    assert res.best(-1.0) is None
    rag = Sc.RaggedScanOutput(None, probs.reshape(-1, ncls), None, None, None, None, np.array([0, steps, 2 * steps]))
    with pytest.raises(T.TcrError, match="lengths given with a ragged scan"):
        sc.tune(rag, thr, lengths=[1, 2], **axes)
    r2 = sc.tune(rag, thr, events=events, tolerance_ms=100.0, **axes)
    d2 = sc.tune(out, thr, events=events, tolerance_ms=100.0, **axes)
    assert torch.equal(r2.detections, d2.detections) and torch.equal(r2.hits, d2.hits) and torch.equal(r2.duplicates, d2.duplicates)
    with pytest.raises(T.TcrError, match="every point of the grid"):
        sc.tune(out, thr, average_window_ms=(20,), min_count=(2,))


# ---- MI355X -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ncls", [3, 5, 12])
def test_gpu_redetect_equals_numpy_rule(hip_lib, ncls):
    check_redetect_equals_numpy_rule(hip_lib, ncls)


@pytest.mark.gpu
def test_gpu_ragged_signal_never_reads_its_predecessor(hip_lib):
    check_ragged_signal_never_reads_its_predecessor(hip_lib)


@pytest.mark.gpu
def test_gpu_grid_equals_per_point_sweeps(hip_lib):
    check_grid(hip_lib, 12, (3, 50), 21, RAGGED_LENS, GRID_THR)


@pytest.mark.gpu
def test_gpu_grid_at_the_lds_limit_and_above(hip_lib):
    check_grid_at_the_lds_limit_and_above(hip_lib)


@pytest.mark.gpu
def test_gpu_grid_eight_wide_body_and_long_halo(hip_lib):
    check_grid_eight_wide_body_and_long_halo(hip_lib)


@pytest.mark.gpu
def test_gpu_grid_workspace_batches(hip_lib):
    check_grid_workspace_batches(hip_lib)


@pytest.mark.gpu
def test_gpu_redetect_and_grid_equal_device_scans(hip_lib):
    """4 x 30 s at 4020 (1500 steps: six tiles a signal), a 2 x 2 x 2 grid, 16 thresholds; dense, and ragged with an empty signal."""
    Sc = scanning()
    fe, net, _, _, _ = setup(hip_lib)
    audio = segment_audio(4, 30 * 16000, 51)
    x = Cm.to_dev(hip_lib, audio)
    base = Sc.KeywordScanner(net, fe, average_window_ms=1000, min_count=3, detection_threshold=0.5, suppression_ms=1500)
    out = base.scan(x)
    step = base.step_samples
    sig = [x[0], x[1, :700 * step].contiguous(), x[2, :0].contiguous(), x[3, :(TILE + 1) * step].contiguous()]
    rag = base.scan_ragged(sig)
    thr = np.quantile(out.score[out.top >= 0].cpu().numpy(), np.linspace(0.0, 1.0, 16)).astype(np.float32)
    axes = dict(average_window_ms=(200, 1000), min_count=(1, 3), suppression_ms=(300, 1500))
    rng = np.random.RandomState(52)
    ev_steps = [random_events(1500, 12, rng, 40) for _ in range(4)]
    events = [[(20.0 * (f + 1), 20.0 * (l + 1), c) for f, l, c in evs] for evs in ev_steps]
    lens = [int(s.shape[0]) for s in sig]
    rag_events = [[e for e in evs if e[0] <= 1000.0 * lens[n] / 16000] for n, evs in enumerate(events)]
    grid = base.tune(out, thr, events=events, tolerance_ms=0.0, **axes)
    rgrid = base.tune(rag, thr, events=rag_events, tolerance_ms=0.0, **axes)
    assert len(grid) == 8 and not grid.dropped
    for j, (w, mc, sp) in enumerate(itertools.product(*axes.values())):
        pt = Sc.KeywordScanner(net, fe, average_window_ms=w, min_count=mc, detection_threshold=0.4, suppression_ms=sp)
        want, got = pt.scan(x), base.redetect(out, average_window_ms=w, min_count=mc, detection_threshold=0.4, suppression_ms=sp)
        rwant, rgot = pt.scan_ragged(sig), base.redetect(rag, average_window_ms=w, min_count=mc, detection_threshold=0.4, suppression_ms=sp)
        assert got.probs is out.probs and torch.equal(want.probs, out.probs) and torch.equal(rwant.probs, rag.probs)
        for f in REDETECTED:
            assert torch.equal(getattr(got, f), getattr(want, f)), (j, f)
            assert torch.equal(getattr(rgot, f), getattr(rwant, f)), (j, "ragged", f)
        one, rone = pt.sweep(want, thr, events=events, tolerance_ms=0.0), pt.sweep(rwant, thr, events=rag_events, tolerance_ms=0.0)
        for f in ("detections", "hits", "duplicates"):
            assert torch.equal(getattr(grid.result(j), f), getattr(one, f)), (j, f)
            assert torch.equal(getattr(rgrid.result(j), f), getattr(rone, f)), (j, "ragged", f)
    assert int(grid.detections.sum()) > 0 and int(grid.hits.sum()) > 0 and int(rgrid.detections[:, 2].sum()) == 0
    assert len({grid.result(j).detections.cpu().numpy().tobytes() for j in range(8)}) >= 3


@pytest.mark.gpu
def test_gpu_tune_audio_cli(hip_lib, tmp_path, capsys):
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    audio = segment_audio(2, 20 * 16000, 53)
    pcm = [np.clip(audio[0] * 32767, -32768, 32767).astype(np.int16), np.clip(audio[1, :13234 * 16] * 32767, -32768, 32767).astype(np.int16)]
    wavs = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    labels = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(10)]
    rows = [(wavs[0], 1000, 2000, "w0"), (wavs[0], 5000, 6500, "w3"), (wavs[0], 12000, 13000, "w0"), (wavs[1], 2000, 3000, "w7")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{a},{b},{c}\n" for f, a, b, c in rows))
    args = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), "--events", str(ev_csv), "--thresholds", "0:0.9:0.1",
            "--tolerance_ms", "500", "--target_fa_per_hour", "5000"]
    from tcresnet_amd import sweep_audio, tune_audio

    def call(mod, *extra):                                # the tool's parse + main in this process (one interpreter start-up spared each)
        capsys.readouterr()
        assert mod.main(mod.parse_arguments([*args, *extra])) == 0
        return capsys.readouterr().out.splitlines()

    single = ["--average_window_ms", "400", "--min_count", "2", "--suppression_ms", "700"]
    for extra in ((), ("--per_label",), ("--ragged",)):
        sw_lines, tu_lines = call(sweep_audio, *single, *extra), call(tune_audio, *single, *extra)
        assert len(tu_lines) == len(sw_lines) >= 11
        assert tu_lines[0] == "average_window_ms,min_count,suppression_ms," + sw_lines[0]
        assert tu_lines[1:] == ["400,2,700," + line for line in sw_lines[1:]]
    with pytest.raises(SystemExit, match="--chunk_seconds and --ragged_chunk_seconds are not supported"):
        tune_audio.parse_arguments([*args, "--chunk_seconds", "5"])
    with pytest.raises(SystemExit, match="--chunk_seconds and --ragged_chunk_seconds are not supported"):
        tune_audio.parse_arguments([*args, "--ragged_chunk_seconds", "5"])
    grid = subprocess.run([sys.executable, os.path.join(ROOT, "tc-resnet_amd", "tune_audio.py"), *args, "--average_window_ms", "200,1000",
                           "--min_count", "2", "--suppression_ms=300,1500"], capture_output=True, text=True, timeout=600)
    assert grid.returncode == 0, grid.stderr
    got = list(csv.DictReader(io.StringIO(grid.stdout)))
    assert len(got) == 4 * 10 and [g["average_window_ms"] for g in got[::10]] == ["200", "200", "1000", "1000"]
    info = json.loads(grid.stderr.strip().splitlines()[-1])
    from tcresnet_amd.deploy import FrozenModel
    sc = FrozenModel.load(path).scanner()
    host = np.zeros((2, 20 * 16000), np.float32)
    lens = []
    for n, x in enumerate(pcm):
        x = x.astype(np.float32) * (1.0 / 32768.0)
        x = x[:len(x) // sc.step_samples * sc.step_samples]
        host[n, :len(x)] = x
        lens.append(len(x))
    ev = [[(a, b, c) for f, a, b, c in rows if f == w] for w in wavs]
    res = sc.tune(sc.scan(torch.from_numpy(host).cuda()), np.arange(0, 0.9 + 1e-9, 0.1), average_window_ms=(200, 1000), min_count=(2,),
                  suppression_ms=(300, 1500), events=ev, lengths=lens, tolerance_ms=500, labels=labels)
    best = res.best(5000, list(range(2, 12)))
    assert info["dropped"] == [] and info["hours"] == pytest.approx(sum(lens) / 16000 / 3600)
    assert best is not None and info["best"] is not None
    pt = best.pop("point")
    assert info["best"] == {"average_window_ms": pt.average_window_ms, "min_count": pt.min_count, "suppression_ms": pt.suppression_ms, **best}
