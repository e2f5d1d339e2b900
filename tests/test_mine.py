"""Mining hard examples from a scan (tcr_mine_detections / _peaks / _select / _gather, KeywordScanner.mine, mine_audio.py).  Every
reference is existing project code (`redetect`, `sweep`, `scan`, `WavFile`, the augmentation stage) or a direct NumPy statement of the
rule in include/tcresnet_hip.h; nothing compares against the code under test.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import csv
import io
import json
import os

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan_ragged import cli_files, cut_signals, run_all, scanning
from tests.test_streaming import frozen_artifact, segment_audio, setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = T._lib.MINE_TILE
_CACHE = {}
STEPS = [1, 30, 0, 50, 7, 200]
DET = dict(average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=40)     # two steps of suppression: labels re-fire
THRESHOLDS = [0.0, 0.45, 0.55]


def dev_t(lib, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(Cm.device_of(lib))


# ---- 1. detections against sweep -------------------------------------------------------------------------------------------------
def det_case(lib, steps=STEPS, seed=31):
    """A TCResNet8 scanner with a short suppression, a ragged scan, and events placed from the scan's own detections at threshold 0
    in the longest signal: one event of label A over its first three detections (labels A, B, A: a hit, a false accept inside an
    event, a duplicate) and one of a label that never fires over the fourth (a miss, and a false accept inside it); one more over the
    first detection of another signal.  Times in ms; the sweep's tolerance is 0."""
    key = ("det", lib.kind, tuple(steps), seed)
    if key not in _CACHE:
        Sc = scanning()
        fe, net, _, _, _ = setup(lib)
        sc = Sc.KeywordScanner(net, fe, **DET)
        signals = cut_signals(lib, segment_audio(len(steps), max(steps) * 320, seed), steps, 320)
        out = sc.scan_ragged(signals)
        long = int(np.argmax(steps))
        a, b = int(out.offsets[long]), int(out.offsets[long + 1])
        fired = np.flatnonzero(out.is_new[a:b].cpu().numpy())
        top = out.top[a:b].cpu().numpy()
        assert fired.size >= 4, fired
        la, lb = int(top[fired[0]]), int(top[fired[1]])
        assert la != lb and int(top[fired[2]]) == la
        quiet = next(c for c in range(2, 12) if c not in (la, lb))
        t = lambda i: 20.0 * (i + 1)
        events = [[] for _ in steps]
        events[long] = [(t(fired[3]) - 10, t(fired[3]) + 10, quiet), (t(fired[0]) - 10, t(fired[2]) + 10, la)]       # (unsorted on purpose)
        other = next(n for n in range(len(steps)) if n != long and int(out.is_new[out.offsets[n]:out.offsets[n + 1]].sum()))
        o0 = int(out.offsets[other])
        f0 = int(np.flatnonzero(out.is_new[o0:int(out.offsets[other + 1])].cpu().numpy())[0])
        events[other] = [(t(f0) - 10, t(f0) + 30, int(out.top[o0 + f0]))]
        _CACHE[key] = dict(sc=sc, signals=signals, out=out, events=events, fe=fe, net=net)
    return _CACHE[key]


def np_rule(top, is_new, offsets, ev_steps, ncls):
    """The rule, walked: (candidate steps, kinds, covering events, event_hit) with events numbered over the signals' sorted lists."""
    steps = np.flatnonzero((is_new != 0) & (top >= 0) & (top < ncls))
    ev = [] if ev_steps is None else [(n, *row) for n, rows in enumerate(ev_steps) for row in sorted(map(tuple, np.asarray(rows).tolist()))]
    hit = np.full(len(ev), -1, np.int64)
    kind, event = np.zeros(steps.size, np.uint8), np.full(steps.size, -1, np.int32)
    for j, p in enumerate(steps):
        n = int(np.searchsorted(offsets, p, side="right") - 1)
        i = p - offsets[n]
        for e, (m, first, last, label) in enumerate(ev):
            if m == n and first <= i <= last:
                event[j] = e
                if label == top[p]:
                    kind[j] = 1 if hit[e] < 0 else 2
                    if hit[e] < 0:
                        hit[e] = p
    return steps, kind, event, hit


def check_detections(lib, c, thresholds=THRESHOLDS):
    Sc = scanning()
    sc, out, events = c["sc"], c["out"], c["events"]
    off, ncls = out.offsets, 12
    _, _, ev_steps = sc.stage.event_steps(out, events, None, 0.0, None)
    seen = set()
    for t in thresholds:
        r = sc.redetect(out, detection_threshold=t)
        top, is_new = r.top.cpu().numpy(), r.is_new.cpu().numpy()
        md = Sc.mine_detections(r.top, r.score, r.is_new, off, ncls, ev_steps, sc.lib)
        steps, kind, event, hit = np_rule(top, is_new, off, ev_steps, ncls)
        assert md.step.cpu().numpy().tolist() == np.flatnonzero(is_new).tolist() == steps.tolist()
        assert md.kind.cpu().numpy().tolist() == kind.tolist() and md.event.cpu().numpy().tolist() == event.tolist()
        assert md.event_hit.cpu().numpy().tolist() == hit.tolist()
        assert np.array_equal(md.label.cpu().numpy(), top[steps]) and torch.equal(md.value, r.score[md.step])
        sw = sc.sweep(out, [t], events=events, tolerance_ms=0.0)
        sig = np.searchsorted(off, steps, side="right") - 1
        got = np.zeros((3, len(off) - 1, ncls), np.int64)
        np.add.at(got, (md.kind.cpu().numpy().astype(np.int64), sig, top[steps]), 1)
        det, hits, dup = (x[:, 0].cpu().numpy() for x in (sw.detections, sw.hits, sw.duplicates))
        assert np.array_equal(got[1], hits) and np.array_equal(got[2], dup) and np.array_equal(got.sum(0), det)
        ev_label = np.concatenate([e[:, 2] for e in ev_steps])
        assert np.array_equal(np.bincount(ev_label[hit >= 0], minlength=ncls), hits.sum(0))
        if t == thresholds[0]:      # the inputs hold every case (in the reference)
            assert set(kind.tolist()) == {0, 1, 2} and (hit < 0).any() and (hit >= 0).any()
            assert ((kind == 0) & (event >= 0)).any() and ((kind == 0) & (event < 0)).any()
        seen.add(steps.size)
        # no events: every candidate is a false accept outside any event
        md0 = Sc.mine_detections(r.top, r.score, r.is_new, off, ncls, None, sc.lib)
        assert md0.event_hit is None and md0.step.tolist() == steps.tolist()
        assert not md0.kind.any() and (md0.event == -1).all()
    assert len(seen) >= 2, seen         # the thresholds change the detections


def check_dense_mine(lib, c):
    """A dense ScanOutput without events: the k best-scored detections, each a false accept."""
    sc = c["sc"]
    x = Cm.to_dev(lib, segment_audio(2, 100 * 320, 33))
    out = sc.scan(x)
    fired = np.flatnonzero(out.is_new.reshape(-1).cpu().numpy())
    assert fired.size >= 3
    score = out.score.reshape(-1).cpu().numpy()[fired]
    k = fired.size - 1
    want = np.sort(fired[np.lexsort((np.arange(fired.size), -score))[:k]])
    m = sc.mine(out, x, k=k)
    assert (m.signal.astype(np.int64) * 100 + m.step).tolist() == want.tolist() and len(m) == k
    assert set(m.kind_names()) == {"false_accept"} and (m.event == -1).all() and m.pcm is None
    assert np.array_equal(m.value, out.score.reshape(-1).cpu().numpy()[want]) and np.array_equal(m.time_ms, 20.0 * (m.step + 1))
    assert np.array_equal(m.label, out.top.reshape(-1).cpu().numpy()[want])
    assert len(sc.mine(out, x, k=0)) == 0 and tuple(sc.mine(out, x, k=0).clips.shape) == (0, 16000)


# ---- 2. peaks against the rule ---------------------------------------------------------------------------------------------------
def np_peaks(values, offsets, classes, floor, R, exclude):
    out = []
    for n in range(len(offsets) - 1):
        a, b = int(offsets[n]), int(offsets[n + 1])
        for p in range(a, b):
            if exclude is not None and any(f <= p - a <= l for f, l in exclude[n]):
                continue
            for c in classes:
                v = values[p, c]
                if not v >= floor:
                    continue
                before, after = values[max(a, p - R):p, c], values[p + 1:min(b, p + R + 1), c]
                if all(v > q for q in before[~np.isnan(before)]) and all(v >= q for q in after[~np.isnan(after)]):
                    out.append((p, c, v))
    return out


def peak_values(total, ncls, offsets, seed, floor):
    """Quantised values (plateaus and equal neighbours), NaNs, values at exactly `floor`, and at every signal boundary a peak with a
    larger value just across it."""
    rng = np.random.RandomState(seed)
    v = (np.round(rng.rand(total, ncls) * 8) / 8).astype(np.float32)
    v[rng.rand(total, ncls) < 0.05] = np.nan
    v[rng.rand(total, ncls) < 0.05] = floor
    for b in offsets[1:-1]:
        if 0 < b < total:
            v[b - 1], v[b] = 0.875, 1.0
    return v


PEAK_TOTALS = [TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


def check_peaks(lib, total, R, seed, ncls=5):
    Sc = scanning()
    short = min(3, total - 2)
    offsets = np.array([0, short, short, short + (total - short) // 3, total, total], np.int64)     # a zero-length signal inside and at the end
    floor = 0.5
    v = peak_values(total, ncls, offsets, seed, floor)
    classes = [0, 2, ncls - 1]
    lens = np.diff(offsets)
    # exclusion ranges that end and start at the first tile's edges (where the signals reach them)
    exclude = []
    for n in range(len(lens)):
        a, rs = int(offsets[n]), []
        for f, l in ((TILE - 3 - a, TILE - 1 - a), (TILE + 1 - a, TILE + 2 - a)):
            if 0 <= f and l < lens[n]:
                rs.append((f, l))
        exclude.append(rs)
    for ex in (None, exclude):
        want = np_peaks(v, offsets, classes, floor, R, ex)
        got = Sc.mine_peaks(dev_t(lib, v), offsets, floor, R, classes, ex, None, lib)
        assert got.count == len(want) > 0
        assert got.step.tolist() == [w[0] for w in want] and got.label.tolist() == [w[1] for w in want]
        assert np.array_equal(got.value.cpu().numpy(), np.array([w[2] for w in want], np.float32))
    cap = len(want) // 2
    few = Sc.mine_peaks(dev_t(lib, v), offsets, floor, R, classes, exclude, cap, lib)
    assert few.count == len(want) and few.step.tolist() == [w[0] for w in want[:cap]] and few.label.tolist() == [w[1] for w in want[:cap]]
    none = Sc.mine_peaks(dev_t(lib, v), offsets, floor, R, classes, exclude, 0, lib)
    assert none.count == len(want) and none.step.numel() == 0


# ---- 3. select against lexsort ---------------------------------------------------------------------------------------------------
def np_select(value, k, eligible=None):
    idx = np.arange(value.size)
    if eligible is not None:
        idx = idx[eligible]
    order = idx[np.lexsort((idx, -value[idx]))]        # (-(-0.0) and -(0.0) compare equal)
    return np.sort(order[:k])


def select_values(n, seed):
    """Quantised values with many ties, negatives, both zeros, and a stretch that differs in the lowest byte only (every histogram
    pass has to split it)."""
    rng = np.random.RandomState(seed)
    v = (np.round(rng.randn(n) * 4) / 4).astype(np.float32)
    v[rng.rand(n) < 0.1] = -0.0
    v[rng.rand(n) < 0.1] = 0.0
    close = rng.rand(n) < 0.3
    v[close] = (np.float32(3.0) + rng.randint(0, 40, int(close.sum())).astype(np.float32) * np.float32(2.0 ** -22)).astype(np.float32)
    return v


SELECT_SIZES = [1, 255, 256, 257, 5000]


def check_select(lib, n, seed):
    Sc = scanning()
    v = select_values(n, seed)
    dv = dev_t(lib, v)
    rng = np.random.RandomState(seed + 1)
    kind = rng.randint(0, 3, n).astype(np.uint8)
    ks = sorted({0, 1, n // 3, n // 2, n - 1, n, n + 5} - {-1})
    for k in ks:
        assert Sc.select_top(dv, k, lib=lib).tolist() == np_select(v, k).tolist(), (n, k)
        got = Sc.select_top(dv, k, dev_t(lib, kind), [0, 2], lib)
        assert got.tolist() == np_select(v, k, kind != 1).tolist(), (n, k)
    assert Sc.select_top(dv, n, dev_t(lib, kind), [5], lib).numel() == 0            # a mask that leaves nothing
    assert Sc.select_top(dv, n, dev_t(lib, kind), [], lib).numel() == 0
    if n >= 255:                    # ties straddling the k-th place: the lowest indices win
        vals, counts = np.unique(v, return_counts=True)
        tie = vals[np.argmax(counts)]
        above = int((v > tie).sum())
        k = above + int(counts.max()) // 2
        got = Sc.select_top(dv, k, lib=lib).cpu().numpy()
        assert got.tolist() == np_select(v, k).tolist()
        assert (v[got] == tie).sum() == k - above and 0 < k - above < counts.max()


def test_select_zeros_compare_equal(emu_lib):
    Sc = scanning()
    v = np.array([-0.0, 0.0, -0.0, -1.0, 0.0], np.float32)
    assert Sc.select_top(dev_t(emu_lib, v), 3, lib=emu_lib).tolist() == [0, 1, 2]
    assert Sc.select_top(dev_t(emu_lib, -v), 2, lib=emu_lib).tolist() == [0, 3]


# ---- 4. gather -------------------------------------------------------------------------------------------------------------------
def np_gather(packed, offsets, sig, first, m):
    out = np.zeros((len(sig), m), np.float32)
    for i, (n, f) in enumerate(zip(sig, first)):
        x = packed[offsets[n]:offsets[n + 1]]
        lo, hi = max(f, 0), min(f + m, len(x))
        if hi > lo:
            out[i, lo - f:hi - f] = x[lo:hi]
    return out


def np_pcm(x):
    y = np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767)      # (np.rint: ties to even)
    return np.where(np.isnan(x), 0, y).astype(np.int16)


def check_gather(lib, lengths, m, seed, shift=0):
    """`shift`: the packed tensor starts that many floats past a 16-byte boundary."""
    Sc = scanning()
    rng = np.random.RandomState(seed)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    packed = rng.randn(int(offsets[-1])).astype(np.float32)
    packed[rng.randint(0, packed.size, 5)] = np.nan
    sig, first = [], []
    for n, length in enumerate(lengths):
        for f in [-m - 2, -5, -1, 0, 1, 2, 3, 4, 5, length - m - 1, length - m, length - m + 1, length - 2, length, length + 3]:
            sig.append(n)
            first.append(f)
    sig, first = np.array(sig, np.int32), np.array(first, np.int64)
    whole = dev_t(lib, np.concatenate([np.zeros(shift, np.float32), packed]))
    out, pcm = Sc.gather_clips(whole[shift:], offsets, sig, first, m, True, True, lib)
    want = np_gather(packed, offsets, sig, first, m)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(pcm.cpu().numpy(), np_pcm(want))
    only, none = Sc.gather_clips(whole[shift:], offsets, dev_t(lib, sig), dev_t(lib, first), m, False, True, lib)
    assert only is None and torch.equal(none, pcm)


def check_pcm_rounding(lib):
    Sc = scanning()
    j = np.arange(-40, 40, dtype=np.float64)
    x = np.concatenate([(j + 0.5) / 32768, [1.0, -1.0, 0.99999, -1.00001, 2.0, -3.0, np.nan, np.inf, -np.inf, 32766.5 / 32768, 32767.5 / 32768,
                                            -32767.5 / 32768, -32768.5 / 32768]]).astype(np.float32)
    ints = np.arange(-32768, 32768, dtype=np.int16)
    x = np.concatenate([x, ints.astype(np.float32) * np.float32(1.0 / 32768.0)])
    offsets = np.array([0, x.size], np.int64)
    _, pcm = Sc.gather_clips(dev_t(lib, x), offsets, np.zeros(1, np.int32), np.zeros(1, np.int64), x.size, False, True, lib)
    got = pcm.cpu().numpy()[0]
    assert np.array_equal(got, np_pcm(x))
    assert np.array_equal(got[-65536:], ints)                       # the decode's inverse
    assert got[:80].tolist() == [int(v) if int(v) % 2 == 0 else int(v) + 1 for v in j]      # (j + 0.5 rounds to the even neighbour)
    assert got[80:89].tolist() == [32767, -32768, 32767, -32768, 32767, -32768, 0, 32767, -32768]


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def check_end_to_end(lib, c, k=8):
    from tcresnet_amd.datasets import augmentation_factory as F
    sc, out, signals, events = c["sc"], c["out"], c["signals"], c["events"]
    m = sc.mine(out, signals, events, k=k, lead_ms=0, tolerance_ms=0.0, kinds=("false_accept", "hit", "duplicate", "miss"), pcm=True)
    names = m.kind_names()
    assert len(m) == k + 1 and names.count("miss") == 1 and names[-1] == "miss"
    assert tuple(m.clips.shape) == (len(m), 16000) and m.pcm.dtype == torch.int16
    packed = out.offsets[m.signal] + m.step
    for i in range(len(m)):
        solo = sc.scan(m.clips[i][None])
        assert torch.equal(solo.probs[0, 16000 // 320 - 1], out.probs[int(packed[i])]), i
    miss = names.index("miss")
    assert np.isnan(m.value[miss]) and m.event[miss] >= 0 and m.event_start_ms[miss] == events[int(m.signal[miss])][0][0]
    keep = np.array(names) != "miss"
    assert np.array_equal(m.value[keep], out.score.cpu().numpy()[packed[keep]])
    assert np.array_equal(m.label[keep], out.top.cpu().numpy()[packed[keep]])
    pool = m.to_pool()
    assert len(pool) == len(m)
    batch = F.no_augmentation_audio(pool, list(range(len(m))), 16000, "wav", 16000)
    assert torch.equal(batch[..., 0], m.pcm.to(torch.float32) / 32768.0)
    # peaks: outside every window that overlaps an event, the k highest local maxima of the keyword classes
    near = sc.mine(out, signals, events, k=5, source="peaks", floor=0.05, radius_ms=100, tolerance_ms=0.0)
    assert len(near) == 5 and set(near.kind_names()) == {"peak"} and (near.label >= 2).all() and (near.value >= 0.05).all()
    probs = out.probs.cpu().numpy()
    assert np.array_equal(near.value, probs[out.offsets[near.signal] + near.step, near.label])
    for n, evs in enumerate(events):
        for s, e, _ in evs:
            inside = (near.signal == n) & (near.time_ms >= s) & (near.time_ms <= e + 1000.0)
            assert not inside.any()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    Sc = scanning()
    dev = Cm.device_of(lib)
    err = lambda: lib.tcr_last_error().decode()
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    f32 = lambda *n: torch.zeros(*n, dtype=torch.float32, device=dev)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
    off, top, score, new, ws = i64(2), i32(8), f32(8), i32(8), i32(4096)
    tabs = [i64(8), i32(8), f32(8), u8(8), i32(8), i64(1), i64(1)]
    p = lambda t: None if t is None else t.data_ptr()

    def det(n=1, total=8, ncls=12, off_=off, ev=(None, None, None, None), ne=0, tabs_=tabs, wsb=4096 * 4):
        return lib.tcr_mine_detections(n, p(off_), total, ncls, p(top), p(score), p(new), *ev, ne, p(ws), wsb, *(p(t) for t in tabs_), None)

    assert det(off_=None) == -1 and "tcr_mine_detections: null argument" in err()
    assert det(tabs_=[None] + tabs[1:]) == -1 and "null argument" in err()
    assert det(n=0) == -1 and "number of signals must be positive" in err()
    assert det(total=0) == -1 and "number of steps must be positive" in err()
    assert det(ncls=257) == -1 and "num_classes 257 outside 1..256" in err()
    assert det(ev=(p(i32(2)), None, None, None)) == -1 and "events need event_first" in err()
    assert det(wsb=16) != 0 and "workspace 16 bytes" in err()
    assert lib.tcr_mine_workspace_bytes(0, 0) == 0 and "outside 1..2^31 - 1" in err()
    vals, mask = f32(8, 12), u8(12)

    def peaks(n=1, ncls=12, floor=0.5, R=3, cap=8, vals_=vals, ex=(None, None, None), step=tabs[0]):
        return lib.tcr_mine_peaks(n, p(off), 8, ncls, p(vals_), p(mask), floor, R, *ex, p(ws), 4096 * 4, cap, p(step), p(tabs[1]), p(tabs[2]),
                                  p(tabs[5]), None)

    assert peaks(vals_=None) == -1 and "tcr_mine_peaks: null argument" in err()
    assert peaks(n=0) == -1 and "number of signals must be positive" in err()
    assert peaks(ncls=300) == -1 and "num_classes 300 outside 1..256" in err()
    assert peaks(floor=float("nan")) == -1 and "floor is NaN" in err()
    assert peaks(R=0) == -1 and f"radius 0 outside 1..{T._lib.MINE_RADIUS_MAX}" in err()
    assert peaks(R=T._lib.MINE_RADIUS_MAX + 1) == -1 and f"outside 1..{T._lib.MINE_RADIUS_MAX}" in err()
    assert peaks(cap=-1) == -1 and "capacity must be >= 0" in err()
    assert peaks(step=None) == -1 and "null candidate tables" in err()
    assert peaks(ex=(p(i32(2)), None, None)) == -1 and "exclusion ranges need" in err()
    sel = lambda n=8, k=3, v=score, out=tabs[0], cnt=tabs[5]: lib.tcr_mine_select(n, p(v), None, 0, k, p(ws), 4096 * 4, p(out), p(cnt), None)
    assert sel(k=-1) == -1 and "k must be >= 0 (got -1)" in err()
    assert sel(n=-2) == -1 and "n_cand -2 outside" in err()
    assert sel(cnt=None) == -1 and "tcr_mine_select: null argument" in err()
    assert sel(v=None) == -1 and "null argument" in err()
    assert sel(n=0) == 0 and sel(k=0) == 0
    soff, sig, first = i64(2), i32(1), i64(1)
    gat = lambda n=1, m=4, out=score, pcm=None, so=soff: lib.tcr_mine_gather(n, p(so), p(score), 1, p(sig), p(first), m, p(out), p(pcm), None)
    assert gat(out=None) == -1 and "out and out_pcm are both null" in err()
    assert gat(n=0) == -1 and "number of signals must be positive" in err()
    assert gat(m=0) == -1 and "n_samples must be positive" in err()
    assert gat(so=None) == -1 and "tcr_mine_gather: null argument" in err()
    # the tables' types (checked before any call)
    x = f32(16)
    with pytest.raises(T.TcrError, match="int32 clip_signal, got int64"):
        Sc.gather_clips(x, np.array([0, 16]), np.zeros(1, np.int64), np.zeros(1, np.int64), 4, lib=lib)
    with pytest.raises(T.TcrError, match="int64 clip_first, got int32"):
        Sc.gather_clips(x, np.array([0, 16]), i32(1), i32(1), 4, lib=lib)
    with pytest.raises(T.TcrError, match="int64 offsets, got int32"):
        Sc.gather_clips(x, np.array([0, 16], np.int32), i32(1), i64(1), 4, lib=lib)
    with pytest.raises(T.TcrError, match="int64 offsets, got torch.int32"):
        Sc.mine_peaks(vals, torch.tensor([0, 8], dtype=torch.int32), 0.5, 3, [2], lib=lib)
    with pytest.raises(T.TcrError, match="offsets must run from 0 to 8"):
        Sc.mine_detections(top, score, new, np.array([0, 9]), 12, lib=lib)
    with pytest.raises(T.TcrError, match="contiguous uint8 kinds"):
        Sc.select_top(score, 3, i32(8), [0], lib)
    with pytest.raises(T.TcrError, match="radius 3000 outside"):
        Sc.mine_peaks(vals, np.array([0, 8]), 0.5, 3000, [2], lib=lib)


# ---- emulator --------------------------------------------------------------------------------------------------------------------
def test_detections_equal_sweep_and_rule(emu_lib):
    check_detections(emu_lib, det_case(emu_lib))


def test_mine_dense_scan_without_events(emu_lib):
    check_dense_mine(emu_lib, det_case(emu_lib))


@pytest.mark.parametrize("total", PEAK_TOTALS)
def test_peaks_equal_rule(emu_lib, total):
    for R in (1, 4, 300):                               # 300: past every signal but the longest one of the largest case
        check_peaks(emu_lib, total, R, total + R)


def test_peaks_class_chunks(emu_lib):
    """A radius whose staged steps no longer hold the five classes at once: the classes go through LDS in chunks."""
    check_peaks(emu_lib, 3 * TILE + 5, 700, 9)


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_equals_lexsort(emu_lib, n):
    check_select(emu_lib, n, n)


@pytest.mark.parametrize("m", [10, 16])
def test_gather_equals_slices(emu_lib, m):
    for shift in range(4):
        check_gather(emu_lib, [37, 0, 101], m, 5 + shift, shift)


def test_gather_pcm_rounding(emu_lib):
    check_pcm_rounding(emu_lib)


def test_mine_end_to_end(emu_lib):
    check_end_to_end(emu_lib, det_case(emu_lib))


def test_mine_refusals(emu_lib):
    check_refusals(emu_lib)
    sc, c = det_case(emu_lib)["sc"], det_case(emu_lib)
    with pytest.raises(T.TcrError, match="source must be"):
        sc.mine(c["out"], c["signals"], source="misses")
    with pytest.raises(T.TcrError, match="unknown kinds \\['peak'\\]"):
        sc.mine(c["out"], c["signals"], kinds=("peak",))
    with pytest.raises(T.TcrError, match="k must be >= 0"):
        sc.mine(c["out"], c["signals"], k=-1)
    with pytest.raises(T.TcrError, match="are not the scan's"):
        sc.mine(c["out"], c["signals"][:-1] + [c["signals"][-1][:320]])
    with pytest.raises(T.TcrError, match="without pcm=True"):
        sc.mine(c["out"], c["signals"], k=1).to_pool()


def test_mine_launches_only_its_own_kernels(emu_lib):
    from tests.test_net_configs import Log, kernel_of
    c = det_case(emu_lib)
    shared = {"select_count_kernel", "select_scan_kernel", "select_prefix_kernel", "select_compact_kernel"}
    with Log(emu_lib) as g:
        c["sc"].mine(c["out"], c["signals"], c["events"], k=4, tolerance_ms=0.0, kinds=("false_accept", "miss"), pcm=True)
    names = {kernel_of(e) for e in g.entries}
    assert names == shared | {"mine_det_flag_kernel", "mine_event_kernel", "mine_classify_kernel", "mine_hist_kernel", "mine_digit_kernel",
                              "mine_pick_kernel", "mine_gather_kernel"}, names
    with Log(emu_lib) as g:
        c["sc"].mine(c["out"], c["signals"], c["events"], k=4, source="peaks", floor=0.05, tolerance_ms=0.0)
    names = {kernel_of(e) for e in g.entries}
    assert names == shared | {"mine_peak_kernel", "mine_peak_emit_kernel", "mine_hist_kernel", "mine_digit_kernel", "mine_pick_kernel",
                              "mine_gather_kernel"}, names


def test_mine_audio_flags_are_refused():
    """The argument checks come before any model is opened."""
    from tcresnet_amd import mine_audio
    base = ["--frozen", "a.npz", "--wav", "a.wav", "--out_dir", "d"]
    for extra, msg in [(["--chunk_seconds", "1"], "--chunk_seconds"), (["--ragged_chunk_seconds", "1"], "--ragged_chunk_seconds"),
                       (["--source", "peaks", "--kinds", "hit"], "--kinds"), (["--kinds", "hit,nothing"], "unknown kind"),
                       (["--top", "-1"], "--top")]:
        with pytest.raises(SystemExit, match=msg):
            mine_audio.check_arguments(mine_audio.parse_arguments(base + extra))
    args = mine_audio.check_arguments(mine_audio.parse_arguments(base))
    assert args.top == 1000 and args.source == "detections" and args.kinds == ["false_accept"] and args.as_label == "_unknown_"


# ---- MI355X ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_detections_equal_sweep_and_rule(hip_lib):
    c = det_case(hip_lib)
    check_detections(hip_lib, c)
    check_dense_mine(hip_lib, c)


@pytest.mark.gpu
@pytest.mark.parametrize("total", PEAK_TOTALS)
def test_gpu_peaks_equal_rule(hip_lib, total):
    for R in (1, 4, 300):
        check_peaks(hip_lib, total, R, total + R)
    if total == PEAK_TOTALS[-1]:
        check_peaks(hip_lib, total, 700, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SELECT_SIZES)
def test_gpu_select_equals_lexsort(hip_lib, n):
    check_select(hip_lib, n, n)


@pytest.mark.gpu
def test_gpu_gather_equals_slices(hip_lib):
    for m in (10, 16):
        for shift in range(4):
            check_gather(hip_lib, [37, 0, 101], m, 5 + shift, shift)
    check_pcm_rounding(hip_lib)


@pytest.mark.gpu
def test_gpu_mine_end_to_end_and_refusals(hip_lib):
    check_end_to_end(hip_lib, det_case(hip_lib))
    check_refusals(hip_lib)


def np_peaks_fast(v, steps, classes, floor, R):
    """np_peaks for signals of equal length without NaNs or exclusions, by sliding maxima (the same rule, vectorised)."""
    out = []
    for n in range(v.shape[0] // steps):
        x = v[n * steps:(n + 1) * steps][:, classes]
        pad = np.full((R, x.shape[1]), -np.inf, np.float32)
        y = np.concatenate([pad, x, pad])
        win = np.lib.stride_tricks.sliding_window_view(y, R, axis=0)           # win[i] = y[i : i + R]
        before, after = win[:steps].max(-1), win[R + 1:R + 1 + steps].max(-1)
        ok = (x >= floor) & (x > before) & (x >= after)
        for p, j in zip(*np.nonzero(ok)):
            out.append((n * steps + p, classes[j], x[p, j]))
    return out


@pytest.mark.gpu
def test_gpu_synthetic_3_x_5000_x_12(hip_lib):
    """Several workgroups in flight in every kernel: peaks, select and gather over 3 signals x 5000 steps x 12 classes."""
    Sc = scanning()
    rng = np.random.RandomState(7)
    steps, ncls, R = 5000, 12, 25
    v = (np.round(rng.rand(3 * steps, ncls) * 64) / 64).astype(np.float32)
    offsets = np.arange(4, dtype=np.int64) * steps
    classes = list(range(2, 12))
    want = np_peaks_fast(v, steps, classes, 0.75, R)
    got = Sc.mine_peaks(dev_t(hip_lib, v), offsets, 0.75, R, classes, None, None, hip_lib)
    assert got.count == len(want) > 1000
    assert got.step.tolist() == [w[0] for w in want] and got.label.tolist() == [w[1] for w in want]
    value = got.value.cpu().numpy()
    assert np.array_equal(value, np.array([w[2] for w in want], np.float32))
    k = 500
    picked = Sc.select_top(got.value, k, lib=hip_lib)
    assert picked.tolist() == np_select(value, k).tolist()
    packed = rng.randn(3 * steps * 320).astype(np.float32)
    sig = (got.step[picked] // steps).to(torch.int32)
    first = ((got.step[picked] % steps + 1) * 320 - 16000)
    out, pcm = Sc.gather_clips(dev_t(hip_lib, packed), offsets * 320, sig, first, 16000, True, True, hip_lib)
    ref = np_gather(packed, offsets * 320, sig.cpu().numpy(), first.cpu().numpy(), 16000)
    assert np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32)) and np.array_equal(pcm.cpu().numpy(), np_pcm(ref))


@pytest.mark.gpu
def test_gpu_mine_audio_cli(hip_lib, tmp_path):
    from tcresnet_amd import audio_input, deploy
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    lengths = [8 * 16000, 5 * 16000 + 77, 3 * 16000]
    wavs = cli_files(tmp_path, lengths, [16000, 16000, 16000], 75)
    labels = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(10)]
    det = ["--average_window_ms", "200", "--min_count", "2", "--detection_threshold", "0.3", "--suppression_ms", "400"]
    # the API's run, for the events and the expected rows
    model = deploy.FrozenModel.load(path)
    sc = model.scanner(average_window_ms=200, min_count=2, detection_threshold=0.3, suppression_ms=400)
    rec = audio_input.Recordings(wavs, sc)
    packed, lens = rec.packed()
    out = sc.scan_ragged((packed, lens))
    fired = np.flatnonzero(out.is_new[:int(out.offsets[1])].cpu().numpy())
    assert fired.size >= 2
    lab = labels[int(out.top[fired[0]])]
    rows = [(wavs[0], 20.0 * (fired[0] + 1) - 10, 20.0 * (fired[0] + 1) + 10, lab), (wavs[2], 100, 200, "w9" if lab != "w9" else "w8")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{a},{b},{c}\n" for f, a, b, c in rows))
    events = [[(rows[0][1], rows[0][2], lab)], [], [(100, 200, rows[1][3])]]
    kinds = ("false_accept", "hit", "miss")
    want = sc.mine(out, (packed, lens), events, k=6, kinds=kinds, tolerance_ms=0.0, labels=labels, pcm=True)
    assert {"false_accept", "hit", "miss"} == set(want.kind_names())
    script = os.path.join(ROOT, "tc-resnet_amd", "mine_audio.py")
    out_dir = tmp_path / "mined"
    cmd = lambda *extra: [script, "--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), *det, "--events", str(ev_csv), "--top", "6",
                          "--kinds", ",".join(kinds), "--tolerance_ms", "0", "--out_dir", str(out_dir), *extra]
    ok, chunked, ragged_chunked = run_all([cmd(), cmd("--chunk_seconds", "1"), cmd("--ragged_chunk_seconds", "1")])
    assert ok[0] == 0, ok[2]
    for r, flag in ((chunked, "--chunk_seconds"), (ragged_chunked, "--ragged_chunk_seconds")):
        assert r[0] != 0 and flag in r[2] and r[1] == ""
    got = list(csv.DictReader(io.StringIO(ok[1])))
    assert len(got) == len(want) >= 3 and list(got[0]) == ["path", "file", "time_ms", "label", "kind", "value", "event_start_ms"]
    pcm = want.pcm.cpu().numpy()
    for i, row in enumerate(got):
        kind = want.kind_names()[i]
        assert row["file"] == wavs[int(want.signal[i])] and row["kind"] == kind and row["label"] == labels[int(want.label[i])]
        assert float(row["time_ms"]) == want.time_ms[i]
        folder = "_unknown_" if kind == "false_accept" else labels[int(want.label[i])]
        stem = os.path.splitext(os.path.basename(row["file"]))[0]
        assert row["path"] == str(out_dir / folder / f"{stem}_{audio_input.format_time_ms(want.time_ms[i])}.wav")
        wav = audio_input.WavFile(row["path"])
        assert (wav.rate, wav.channels, wav.length) == (16000, 1, 16000)
        assert np.array_equal(wav.read_pcm(0, 16000), pcm[i])
        if kind == "miss":
            assert row["value"] == "" and float(row["event_start_ms"]) == 100.0
        else:
            assert float(row["value"]) == pytest.approx(float(want.value[i]), abs=1e-6)
    counts = json.loads(ok[2].strip().splitlines()[-1])
    assert counts["clips"] == len(want) and counts["kinds"] == {k: want.kind_names().count(k) for k in kinds}
