"""Capturing detections' audio on live streams (tcr_capture_*, capturing.StreamingRecorder, stream_audio.py --capture_dir).  The
reference is tests/capture_ref.py -- the definition of include/tcresnet_hip.h in NumPy over whole recordings -- or existing project
code (`gather_clips`, a scan); every comparison is bitwise.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.capture_ref import Reference, clip_of, delay
from tests.test_mine import np_pcm
from tests.test_streaming import frozen_artifact, segment_audio, setup, write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 777.0
NCLS = 12
CHUNKS = [1, 1, 2, 7, 8, 9, 40]             # then the rest
ROWS = 90


def up(x, m):
    return (x + m - 1) // m * m


class Raw:
    """The C entries over torch tensors: every call fills the outputs with a marker first and returns the clips it wrote as
    (stream, step, label, score bits, clip bits, pcm) tuples, after checking that nothing else was touched."""

    def __init__(self, lib, S, step, n, lead, capacity=64, classes=None, pcm=True, max_rows=4096):
        self.lib, self.dev = lib, Cm.device_of(lib)
        self.S, self.step, self.n, self.lead, self.cap, self.D = S, step, n, lead, capacity, delay(lead, step)
        self.R = up(n + max(0, -lead), 4)
        nstate = lib.tcr_capture_state_bytes(S, step, n, lead)
        assert nstate == up(16 * S, 256) + up(12 * S * self.D, 256) + 4 * S * self.R, lib.tcr_last_error()     # (the header's layout)
        self.state = torch.full((nstate // 4,), 5.0, dtype=torch.float32, device=self.dev)
        nws = lib.tcr_capture_workspace_bytes(max_rows)
        assert nws > 0
        self.ws = torch.zeros(nws // 4 + 1, dtype=torch.int32, device=self.dev)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        self.out, self.pcm = z((capacity, n), torch.float32), z((capacity, n), torch.int16) if pcm else None
        self.stream, self.row, self.label, self.score = z(capacity, torch.int32), z(capacity, torch.int64), z(capacity, torch.int32), \
            z(capacity, torch.float32)
        self.count = z(2, torch.int32)
        self.cmask = None
        if classes is not None:
            m = np.zeros(NCLS, np.uint8)
            m[list(classes)] = 1
            self.cmask = torch.from_numpy(m).to(self.dev)
        lib.check(lib.tcr_capture_init(S, step, n, lead, self.state.data_ptr(), None), "tcr_capture_init")

    def _mark(self):
        for t in (self.out, self.pcm, self.stream, self.row, self.label, self.score, self.count):
            if t is not None:
                t.fill_(MARK)

    def _tail(self):
        return (self.state.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 4, self.cap, self.out.data_ptr(),
                None if self.pcm is None else self.pcm.data_ptr(), self.stream.data_ptr(), self.row.data_ptr(), self.label.data_ptr(),
                self.score.data_ptr(), self.count.data_ptr(), None)

    def _read(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        n, due = (int(v) for v in self.count.cpu().numpy())
        assert 0 <= n <= self.cap and n == min(due, self.cap), (n, due)
        for t in (self.out, self.pcm, self.stream, self.row, self.label, self.score):      # untouched rows keep the marker
            assert t is None or bool((t[n:] == MARK).all())
        out = self.out.cpu().numpy()
        pcm = None if self.pcm is None else self.pcm.cpu().numpy()
        stream, row, label, score = (t[:n].cpu().numpy() for t in (self.stream, self.row, self.label, self.score))
        clips = [(int(stream[i]), int(row[i]), int(label[i]), score.view(np.int32)[i], out[i].view(np.int32).copy(),
                  None if pcm is None else pcm[i].copy()) for i in range(n)]
        return clips, due

    def push(self, samples, top, score, is_new, reset=None, ragged=False):
        """Per stream: samples [rows_s * step] and rows [rows_s].  Dense needs equal counts."""
        dev, lib = self.dev, self.lib
        cat = lambda xs, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(x, dt) for x in xs]))).to(dev)
        x, t, sc, nw = cat(samples, np.float32), cat(top, np.int32), cat(score, np.float32), cat(is_new, np.int32)
        rs = None if reset is None else torch.from_numpy(np.asarray(reset, np.uint8)).to(dev)
        rows = [len(v) for v in top]
        head = (self.step, self.n, self.lead, x.data_ptr(), t.data_ptr(), sc.data_ptr(), nw.data_ptr(),
                None if self.cmask is None else self.cmask.data_ptr(), NCLS, None if rs is None else rs.data_ptr())
        self._mark()
        if ragged:
            off = torch.from_numpy(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)).to(dev)
            lib.check(lib.tcr_capture_push_ragged(self.S, off.data_ptr(), int(sum(rows)), *head, *self._tail()), "tcr_capture_push_ragged")
        else:
            assert len(set(rows)) == 1
            lib.check(lib.tcr_capture_push(self.S, rows[0], *head, *self._tail()), "tcr_capture_push")
        return self._read()

    def flush(self, mask=None):
        m = None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).to(self.dev)
        self._mark()
        self.lib.check(self.lib.tcr_capture_flush(self.S, None if m is None else m.data_ptr(), self.step, self.n, self.lead, *self._tail()),
                       "tcr_capture_flush")
        return self._read()

    def stream_state(self, s):
        """The bytes of stream s's state, by the header's layout: its integers, its tail and its ring."""
        b = self.state.cpu().numpy().view(np.uint8)
        S, D, R = self.S, self.D, self.R
        t0 = up(16 * S, 256)
        r0 = t0 + up(12 * S * D, 256)
        parts = [b[16 * s:16 * s + 16]] + [b[t0 + 4 * (k * S * D + s * D):t0 + 4 * (k * S * D + s * D + D)] for k in range(3)]
        return np.concatenate(parts + [b[r0 + 4 * s * R:r0 + 4 * (s + 1) * R]]).copy()


def same(got, want):
    """Clips of the code under test (Raw's tuples) against the reference's, bitwise and in order."""
    assert [(g[0], g[1], g[2]) for g in got] == [(w.stream, w.step, w.label) for w in want]
    for g, w in zip(got, want):
        assert g[3] == np.float32(w.score).view(np.int32), (g[:3], "score")
        assert np.array_equal(g[4], w.clip.view(np.int32)), (g[:3], "clip")
        if g[5] is not None:
            assert np.array_equal(g[5], np_pcm(w.clip)), (g[:3], "pcm")


def rows_case(S, rows, step, seed, planted):
    """Random audio (with NaN, infinities and both zeros) and rows with triggers at `planted` and a few random rows per stream."""
    rng = np.random.RandomState(seed)
    audio = rng.randn(S, rows * step).astype(np.float32)
    audio.reshape(-1)[rng.randint(0, audio.size, 6)] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-30]
    top = rng.randint(0, NCLS, (S, rows)).astype(np.int32)
    score = rng.rand(S, rows).astype(np.float32)
    is_new = np.zeros((S, rows), np.int32)
    for s in range(S):
        is_new[s, [r for r in planted if 0 <= r < rows]] = 1
        is_new[s, rng.randint(0, rows, 3 + s)] = 1
    is_new[1, 0] = 0                                # (not every stream starts with a trigger)
    return audio, top, score, is_new


def cut(rows, chunks=CHUNKS):
    bounds, at = [], 0
    for c in chunks:
        bounds.append((at, at + c))
        at += c
    return bounds + [(at, rows)]


def check_split(lib, step, n, lead, ragged):
    """Any split equals the whole: the chunks of CHUNKS against the reference fed the same chunks, whose clips are cut from the
    whole recording so far."""
    S, D = 3, delay(lead, step)
    bounds = cut(ROWS)
    ends = [b - 1 for _, b in bounds]
    planted = [0, 1, 4, 5, 6] + ends + [e - D for e in ends] + [a + D for a, _ in bounds]     # (the last: emitted by a chunk's first row, from the ring)
    audio, top, score, is_new = rows_case(S, ROWS, step, 7 + lead, planted)
    raw, ref = Raw(lib, S, step, n, lead), Reference(S, step, n, lead)
    seen = dict(before_start=0, overlap=0, wrapped=0, total=0)
    assert any((b - a) * step > raw.R for a, b in bounds)              # one call is longer than the ring
    last = {}
    for a, b in bounds:
        args = ([audio[s, a * step:b * step] for s in range(S)], [top[s, a:b] for s in range(S)], [score[s, a:b] for s in range(S)],
                [is_new[s, a:b] for s in range(S)])
        want = ref.push(*args)
        got, due = raw.push(*args, ragged=ragged)
        assert due == len(want)
        same(got, want)
        for w in want:
            seen["total"] += 1
            seen["before_start"] += w.first < 0
            seen["overlap"] += last.get(w.stream, -10) == w.step - 1
            # the clip's samples that the ring held when the call began straddle the ring's end
            lo, hi = max(w.first, 0), min(w.first + n, a * step)
            seen["wrapped"] += hi > lo and lo // raw.R != (hi - 1) // raw.R
            last[w.stream] = w.step
    assert seen["before_start"] >= 2 and seen["overlap"] >= 4 and seen["wrapped"] >= 4 and seen["total"] >= 30, seen
    assert (ref.carried > 0) == (D > 0), (ref.carried, D)
    if D > 0:                                       # the triggers of the last D rows are still pending
        want = ref.flush()
        got, due = raw.flush()
        assert due == len(want) >= 1
        same(got, want)
    return seen


LEADS = [0, 3, 5, 12, -4]


def check_ragged(lib, lead):
    """Streams advance by 0, 1 and many rows per call; a stream without rows keeps its state bytes and its reset stays pending."""
    S, step, n, rows = 4, 5, 37, 60
    audio, top, score, is_new = rows_case(S, rows, step, 40 + lead, [0, 1, 9, 10, 30])
    raw, ref = Raw(lib, S, step, n, lead), Reference(S, step, n, lead)
    rng = np.random.RandomState(3)
    at = np.zeros(S, np.int64)
    idle_checked = resets_kept = emitted = 0
    pending = np.zeros(S, bool)
    call = 0
    while (at < rows).any():
        take = np.array([[0, 1, 11, 2][(s + call) % 4] if rng.rand() < 0.8 else 0 for s in range(S)])
        take = np.minimum(take, rows - at)
        if call == 0:
            take[:] = [0, 1, 11, 0]
        if take.sum() == 0:
            call += 1
            continue
        if call in (3, 6):                          # a reset for every stream: it applies only where rows arrive
            pending[:] = True
        args = ([audio[s, at[s] * step:(at[s] + take[s]) * step] for s in range(S)], [top[s, at[s]:at[s] + take[s]] for s in range(S)],
                [score[s, at[s]:at[s] + take[s]] for s in range(S)], [is_new[s, at[s]:at[s] + take[s]] for s in range(S)])
        before = [raw.stream_state(s) for s in range(S)]
        want = ref.push(*args, reset=pending)
        got, due = raw.push(*args, reset=pending.astype(np.uint8), ragged=True)
        same(got, want)
        emitted += len(want)
        for s in range(S):
            if take[s] == 0:
                assert np.array_equal(raw.stream_state(s), before[s]), (call, s)
                idle_checked += 1
                resets_kept += bool(pending[s])
            else:
                pending[s] = False
        at += take
        call += 1
    assert idle_checked >= 5 and resets_kept >= 1 and emitted >= 10, (idle_checked, resets_kept, emitted)


def check_reset_flush(lib):
    S, step, n, lead = 2, 8, 40, 20                 # D = 3
    D = delay(lead, step)
    assert D == 3
    audio, top, score, is_new = rows_case(S, 40, step, 5, [])
    is_new[:] = 0
    is_new[0, [9, 10, 19, 21]] = 1                  # 9: pending at the reset (dropped); 19: flushed; 21: after the flush
    is_new[1, [8, 19, 30]] = 1
    raw, ref = Raw(lib, S, step, n, lead), Reference(S, step, n, lead)

    def push(a, b, reset=None):
        args = ([audio[s, a * step:b * step] for s in range(S)], [top[s, a:b] for s in range(S)], [score[s, a:b] for s in range(S)],
                [is_new[s, a:b] for s in range(S)])
        want = ref.push(*args, reset=reset)
        got, _ = raw.push(*args, reset=None if reset is None else np.asarray(reset, np.uint8))
        same(got, want)
        return want

    assert push(0, 10) == []                        # (stream 0's row 9 and stream 1's row 8 are pending)
    w = push(10, 20, reset=[1, 0])                  # stream 0 starts afresh: its row 9 is gone, row 10 is its row 0
    assert [(c.stream, c.step) for c in w] == [(0, 0), (1, 8)]
    assert w[0].first < 0 and not w[0].clip[:-w[0].first].any() and w[0].clip[-w[0].first:].any()      # zeros before the reset
    want = ref.flush([1, 0])
    got, due = raw.flush([1, 0])
    same(got, want)
    assert [(c.stream, c.step) for c in want] == [(0, 9)] and due == 1        # stream 0's row 19 (its row 9), the future as zeros
    future = (9 + 1) * step + lead - 10 * step
    assert future > 0 and not want[0].clip[-future:].any() and want[0].clip[:-future].any()
    got, due = raw.flush([1, 0])                    # once only
    assert got == [] and due == 0
    w = push(20, 40)                                # stream 0 goes on: row 21 (its 11); stream 1's row 19 was not flushed
    assert [(c.stream, c.step) for c in w] == [(0, 11), (1, 19), (1, 30)]
    want = ref.flush()
    got, due = raw.flush()
    assert want == [] and got == [] and due == 0


def check_mask_capacity_refusals(lib):
    S, step, n, lead = 3, 8, 40, 0
    audio, top, score, is_new = rows_case(S, 20, step, 9, list(range(20)))
    is_new[:] = 1
    args = ([audio[s] for s in range(S)], [top[s] for s in range(S)], [score[s] for s in range(S)], [is_new[s] for s in range(S)])
    classes = [2, 5, 7]
    want = Reference(S, step, n, lead, classes).push(*args)
    assert 3 <= len(want) < 60 and {w.label for w in want} <= set(classes)
    got, due = Raw(lib, S, step, n, lead, classes=classes).push(*args)
    assert due == len(want)
    same(got, want)
    cap = len(want) // 2                            # overflow: the first `capacity` in order, n_clips = (capacity, due)
    got, due = Raw(lib, S, step, n, lead, capacity=cap, classes=classes).push(*args)
    assert due == len(want) and len(got) == cap
    same(got, want[:cap])
    everything = Reference(S, step, n, lead).push(*args)
    got, due = Raw(lib, S, step, n, lead, capacity=4, pcm=False).push(*args, ragged=True)
    assert due == 60 == len(everything)
    same(got, everything[:4])
    # refusals
    err = lambda: lib.tcr_last_error().decode()
    assert lib.tcr_capture_state_bytes(2, 8, 0, 0) == 0 and "n_samples must be positive" in err()
    assert lib.tcr_capture_state_bytes(2, 0, 40, 0) == 0 and "step_samples must be positive" in err()
    assert lib.tcr_capture_state_bytes(0, 8, 40, 0) == 0 and "streams must be positive" in err()
    assert lib.tcr_capture_state_bytes(2 ** 31 - 1, 8, 2 ** 28, 0) == 0 and "size overflow" in err()
    assert lib.tcr_capture_state_bytes(2, 8, 2 ** 29, 0) == 0 and "outside" in err()
    assert lib.tcr_capture_workspace_bytes(0) == 0 and "outside 1..2^31 - 1" in err()
    assert lib.tcr_capture_state_bytes(4096, 320, 16000, 0) == 65536 + 4096 * 64000            # 262 MB
    r = Raw(lib, S, step, n, lead)
    x, t, sc, nw = (torch.zeros(S * 20 * (step if i == 0 else 1), dtype=d, device=r.dev)
                    for i, d in enumerate((torch.float32, torch.int32, torch.float32, torch.int32)))
    p = lambda v: None if v is None else v.data_ptr()

    def call(S_=S, steps=20, step_=step, n_=n, x_=x, state=r.state, wsb=r.ws.numel() * 4, cap=r.cap, count=r.count):
        return lib.tcr_capture_push(S_, steps, step_, n_, lead, p(x_), p(t), p(sc), p(nw), None, NCLS, None, p(state), p(r.ws), wsb, cap,
                                    p(r.out), p(r.pcm), p(r.stream), p(r.row), p(r.label), p(r.score), p(count), None)

    r._mark()
    assert call(n_=0) == -1 and "n_samples must be positive" in err()
    assert call(step_=0) == -1 and "step_samples must be positive" in err()
    assert call(steps=0) == -1 and "number of steps must be positive" in err()
    assert call(x_=None) == -1 and "null argument" in err()
    assert call(state=None) == -1 and "null argument" in err()
    assert call(count=None) == -1 and "null argument" in err()
    assert call(cap=-1) == -1 and "capacity -1 outside" in err()
    assert call(wsb=64) != 0 and "workspace 64 bytes" in err()
    assert lib.tcr_capture_flush(0, None, step, n, lead, *r._tail()) == -1 and "streams must be positive" in err()
    assert bool((r.count == int(MARK)).all()) and bool((r.out == MARK).all())          # a refused call touches nothing
    assert call() == 0


def check_many_clips(lib):
    """Thousands of clips in one call: several tiles of the compaction, a gather grid far wider than the device."""
    S, step, n, rows = 3, 5, 37, 700
    audio, top, score, is_new = rows_case(S, rows, step, 21, [])
    is_new[:] = 1
    args = ([audio[s] for s in range(S)], [top[s] for s in range(S)], [score[s] for s in range(S)], [is_new[s] for s in range(S)])
    want = Reference(S, step, n, 0).push(*args)
    assert len(want) == S * rows > 8 * 256
    got, due = Raw(lib, S, step, n, 0, capacity=S * rows, pcm=False).push(*args)
    assert due == len(want)
    same(got, want)


def check_pcm(lib):
    """out_pcm is test_mine.np_pcm of the float clips, over the rounding edge values of test_mine.check_pcm_rounding."""
    j = np.arange(-40, 40, dtype=np.float64)
    x = np.concatenate([(j + 0.5) / 32768, [1.0, -1.0, 0.99999, -1.00001, 2.0, -3.0, np.nan, np.inf, -np.inf, 32766.5 / 32768, 32767.5 / 32768,
                                            -32767.5 / 32768, -32768.5 / 32768]]).astype(np.float32)
    ints = np.arange(-32768, 32768, 257, dtype=np.int16)
    x = np.concatenate([x, ints.astype(np.float32) * np.float32(1.0 / 32768.0)])
    step, n = 5, 37
    rows = len(x) // step
    x = x[:rows * step]
    raw, ref = Raw(lib, 1, step, n, 0, capacity=rows), Reference(1, step, n, 0)
    args = ([x], [np.full(rows, 3, np.int32)], [np.zeros(rows, np.float32)], [np.ones(rows, np.int32)])
    want = ref.push(*args)
    got, _ = raw.push(*args)
    assert len(want) == rows
    same(got, want)
    pcm = np.concatenate([g[5][-step:] for g in got])       # every sample once: the last step of every clip
    assert np.array_equal(pcm, np_pcm(x))
    assert pcm[:80].tolist() == [int(v) if int(v) % 2 == 0 else int(v) + 1 for v in j]
    assert pcm[80:89].tolist() == [32767, -32768, 32767, -32768, 32767, -32768, 0, 32767, -32768]


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
DET = dict(average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=40)
_CACHE = {}


def live_case(lib):
    """A detector and a recorder over 3 streams fed 130 rows through push, push_many and push_ragged mixed; the outputs stacked per
    stream and everything the recorder returned."""
    if lib.kind in _CACHE:
        return _CACHE[lib.kind]
    from tcresnet_amd import capturing, scanning as Sc, streaming as St
    fe, net, _, _, _ = setup(lib)
    S, rows, step = 3, 130, 320
    det = St.StreamingDetector(net, fe, S, **DET)
    rec = capturing.StreamingRecorder(det, classes=range(NCLS), capacity=64, pcm=True)      # (the random net's labels are any two)
    audio = Cm.to_dev(lib, segment_audio(S, rows * step, 61))
    at = np.zeros(S, np.int64)
    plan = [("push", 1), ("push", 1), ("many", 30), ("ragged", [5, 0, 17]), ("ragged", [0, 12, 1]), ("push", 1), ("many", 60)]
    got = []
    cols = {k: [[] for _ in range(S)] for k in ("top", "score", "is_new", "probs")}

    def take(out_rows, s, o):
        if out_rows == 0:
            return
        for k in cols:
            cols[k][s].append(getattr(o, k).reshape(out_rows, -1).clone())

    def collect(c):
        h = c.host()
        assert c.due == len(c) == len(h.stream)
        for i in range(len(h.stream)):
            got.append((int(h.stream[i]), int(h.step[i]), int(h.label[i]), h.score[i], h.clips[i].copy(), h.pcm[i].copy(), h.time_ms[i]))

    for kind, m in plan:
        if kind == "push":
            x = torch.stack([audio[s, at[s] * step:(at[s] + 1) * step] for s in range(S)]).contiguous()
            out = det.push(x)
            for s in range(S):
                take(1, s, St.StreamOutput(*(t[s] for t in out)))
            collect(rec.push(x, out))
            at += 1
        elif kind == "many":
            x = torch.stack([audio[s, at[s] * step:(at[s] + m) * step] for s in range(S)]).contiguous()
            out = det.push_many(x)
            for s in range(S):
                take(m, s, Sc.ScanOutput(*(t[s] for t in out)))
            collect(rec.push(x, out))
            at += m
        else:
            xs = [audio[s, at[s] * step:(at[s] + m[s]) * step].contiguous() for s in range(S)]
            out = det.push_ragged(xs)
            for s in range(S):
                take(m[s], s, out.signal(s))
            collect(rec.push(xs, out))
            at += np.array(m)
    stacked = {k: [torch.cat(v[s]) for s in range(S)] for k, v in cols.items()}
    _CACHE[lib.kind] = dict(fe=fe, net=net, det=det, rec=rec, audio=audio, at=at, got=got, stacked=stacked, S=S, step=step)
    return _CACHE[lib.kind]


def check_live(lib):
    """The captured clips and their tables equal `gather_clips` of the concatenated audio at the stacked outputs' detections; a captured
    clip scanned alone reproduces its step's posteriors."""
    from tcresnet_amd import scanning as Sc
    c = live_case(lib)
    S, step, audio, got, st = c["S"], c["step"], c["audio"], c["got"], c["stacked"]
    want = []
    for s in range(S):
        top, new, score = (st[k][s].reshape(-1).cpu().numpy() for k in ("top", "is_new", "score"))
        for i in np.flatnonzero((new != 0) & (top >= 0)):
            want.append((s, int(i), int(top[i]), score[i]))
    assert len(want) >= 6 and len({w[0] for w in want}) == S
    key = lambda r: (r[0], r[1])
    assert sorted([g[:3] for g in got]) == sorted([w[:3] for w in want])
    by = {key(g): g for g in got}
    sig = np.array([w[0] for w in want], np.int32)
    first = np.array([(w[1] + 1) * step - 16000 for w in want], np.int64)
    lens = c["at"] * step
    packed = torch.cat([audio[s, :lens[s]] for s in range(S)]).contiguous()
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    clips, pcm = Sc.gather_clips(packed, offsets, sig, first, 16000, True, True, lib)
    clips, pcm = clips.cpu().numpy(), pcm.cpu().numpy()
    for j, w in enumerate(want):
        g = by[key(w)]
        assert g[3].view(np.int32) == w[3].view(np.int32) and g[6] == 20.0 * (w[1] + 1)
        assert np.array_equal(g[4].view(np.int32), clips[j].view(np.int32)) and np.array_equal(g[5], pcm[j]), w[:3]
    sc = Sc.KeywordScanner(c["net"], c["fe"], **DET)
    for w in (want[0], want[len(want) // 2], want[-1]):
        solo = sc.scan(torch.from_numpy(by[key(w)][4])[None].to(audio.device))
        assert torch.equal(solo.probs[0, 16000 // step - 1], st["probs"][w[0]][w[1]]), w[:3]


def check_live_phrases(lib):
    """The same streams through a StreamingPhraseDetector's outputs: the recorder takes them unchanged."""
    from tcresnet_amd import capturing, scanning as Sc, streaming as St
    c = live_case(lib)
    S, step, audio = c["S"], c["step"], c["audio"]
    sc = Sc.KeywordScanner(c["net"], c["fe"], **DET)
    base = sc.scan(audio[:, :60 * step].contiguous())
    order = np.argsort(-base.smoothed.cpu().numpy().reshape(-1, NCLS).mean(axis=0))
    words = [[int(order[0]), int(order[0])], [int(order[0]), int(order[1])], [int(order[1]), int(order[0])]]
    ph = Sc.PhraseDetector(sc, words, window_ms=8 * sc.step_ms, detection_threshold=0.05, suppression_ms=2 * sc.step_ms)
    det = St.StreamingDetector(c["net"], c["fe"], S, **DET)
    live = ph.streaming(S)
    rec = capturing.StreamingRecorder(live, capacity=64)
    got, rows = [], []
    for a, b in [(0, 1), (1, 20), (20, 60)]:
        x = audio[:, a * step:b * step].contiguous()
        out = live.push(det.push(x) if b - a == 1 else det.push_many(x))
        rows.append(tuple(getattr(out, k).reshape(S, b - a).clone() for k in ("top", "is_new")))
        h = rec.push(x, out).host()
        got += [(int(s), int(i), int(l), clip.copy()) for s, i, l, clip in zip(h.stream, h.step, h.label, h.clips)]
    top, new = (torch.cat([r[k] for r in rows], dim=1).cpu().numpy() for k in (0, 1))
    want = [(s, int(i), int(top[s, i])) for s in range(S) for i in np.flatnonzero((new[s] != 0) & (top[s] >= 0) & (top[s] < 3))]
    assert len(want) >= 2 and sorted(g[:3] for g in got) == sorted(want)
    host = audio.cpu().numpy()
    for g in got:
        assert np.array_equal(g[3].view(np.int32), clip_of(host[g[0]], g[1], step, 16000, 0).view(np.int32)), g[:3]


def check_python_reset_flush(lib):
    """`StreamingRecorder.reset` / `flush` through dense and ragged pushes of made-up outputs: a reset stays pending for a stream
    without rows, a flush takes `reset`'s argument forms."""
    from tcresnet_amd import capturing, scanning, streaming
    c = live_case(lib)
    S, step, n, dev = c["S"], c["step"], 800, Cm.device_of(lib)
    rec = capturing.StreamingRecorder(c["det"], lead_ms=30.0, classes=range(NCLS), capacity=16, n_samples=n)
    assert rec.delay_steps == 2 and rec.lead == 480
    ref = Reference(S, step, n, 480)
    rng = np.random.RandomState(8)
    pending = np.zeros(S, bool)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    emitted = 0

    def push(rows, dense=False):
        nonlocal emitted
        x = [rng.randn(r * step).astype(np.float32) for r in rows]
        top = [rng.randint(0, NCLS, r).astype(np.int32) for r in rows]
        score = [rng.rand(r).astype(np.float32) for r in rows]
        new = [(rng.rand(r) < 0.6).astype(np.int32) for r in rows]
        want = ref.push(x, top, score, new, reset=pending.copy())
        pending[np.array(rows) > 0] = False
        if dense:
            out = streaming.StreamOutput(None, None, None, t(np.concatenate(top)), t(np.concatenate(score)), t(np.concatenate(new)))
            h = rec.push(t(np.stack(x)), out).host()
        else:
            out = scanning.RaggedScanOutput(None, None, None, t(np.concatenate(top)), t(np.concatenate(score)), t(np.concatenate(new)),
                                            np.concatenate([[0], np.cumsum(rows)]))
            h = rec.push([t(v) for v in x], out).host()
        compare(h, want)
        emitted += len(want)

    def compare(h, want):
        assert [(int(a), int(b), int(l)) for a, b, l in zip(h.stream, h.step, h.label)] == [(w.stream, w.step, w.label) for w in want]
        for i, w in enumerate(want):
            assert np.array_equal(h.clips[i].view(np.int32), w.clip.view(np.int32)) and h.time_ms[i] == 20.0 * (w.step + 1)

    push([2, 0, 1])
    push([3, 3, 3])
    rec.reset([1, 2])
    pending[[1, 2]] = True
    push([1, 0, 3])                                 # stream 1 brings no row: its reset waits
    assert rec._pending is not None and rec._pending.tolist() == [False, True, False]
    push([1, 1, 1], dense=True)                     # ... until here
    assert rec._pending is None
    push([4, 2, 0])
    compare(rec.flush(np.array([True, False, False])).host(), ref.flush([1, 0, 0]))
    compare(rec.flush([1]).host(), ref.flush([0, 1, 0]))
    push([2, 2, 2])
    last = ref.flush()
    compare(rec.flush().host(), last)
    assert emitted >= 5 and len(last) >= 1           # (clips compared from pushes; the flushes come on top)


def check_python_refusals(lib):
    from tcresnet_amd import capturing, scanning, streaming
    c = live_case(lib)
    det, rec, S, step = c["det"], c["rec"], c["S"], c["step"]
    dev = Cm.device_of(lib)
    x = torch.zeros((S, step), dtype=torch.float32, device=dev)
    with pytest.raises(T.TcrError, match="samples \\(3, 319\\)"):
        rec.push(x[:, :-1].contiguous(), det.out)
    with pytest.raises(T.TcrError, match="samples \\(2, 320\\)"):
        rec.push(x[:2].contiguous(), det.out)
    bad = streaming.StreamOutput(*(t[:2] if t is not None else None for t in det.out))
    with pytest.raises(T.TcrError, match="is not contiguous"):
        rec.push(x, bad)
    wide = streaming.StreamOutput(det.out.logits, torch.zeros((S, 5), device=dev), det.out.smoothed, det.out.top, det.out.score, det.out.is_new)
    with pytest.raises(T.TcrError, match="over 5 classes"):
        rec.push(x, wide)
    with pytest.raises(T.TcrError, match="capacity must be >= 1"):
        capturing.StreamingRecorder(det, capacity=0)
    with pytest.raises(T.TcrError, match="without pcm=True"):
        capturing.StreamingRecorder(det, capacity=2).flush().to_pool()
    with pytest.raises(T.TcrError, match="no detection stage"):
        capturing.StreamingRecorder(object())
    pool = rec.flush().to_pool()
    assert len(pool.lengths) == 0
    assert scanning.StreamingRecorder is streaming.StreamingRecorder is capturing.StreamingRecorder
    assert scanning.CapturedClips is streaming.CapturedClips is capturing.CapturedClips


# ---- emulator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("lead", LEADS)
def test_any_split_equals_the_whole_scalar_append(emu_lib, lead, ragged):
    check_split(emu_lib, 5, 37, lead, ragged)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("lead", LEADS)
def test_any_split_equals_the_whole_16_byte_append(emu_lib, lead, ragged):
    check_split(emu_lib, 8, 40, lead, ragged)


@pytest.mark.parametrize("lead", [0, 12])
def test_ragged_idle_streams_keep_state_and_reset(emu_lib, lead):
    check_ragged(emu_lib, lead)


def test_reset_and_flush(emu_lib):
    check_reset_flush(emu_lib)


def test_class_mask_capacity_and_refusals(emu_lib):
    check_mask_capacity_refusals(emu_lib)


def test_pcm_is_minings_rounding(emu_lib):
    check_pcm(emu_lib)


def test_thousands_of_clips_in_one_call(emu_lib):
    check_many_clips(emu_lib)


def test_recorder_next_to_a_real_detector(emu_lib):
    check_live(emu_lib)
    check_python_refusals(emu_lib)
    check_python_reset_flush(emu_lib)


def test_recorder_next_to_a_phrase_detector(emu_lib):
    check_live_phrases(emu_lib)


def test_recorder_launches_only_its_own_kernels(emu_lib):
    from tests.test_net_configs import Log, kernel_of
    from tcresnet_amd import capturing, scanning
    c = live_case(emu_lib)
    det, S, step = c["det"], c["S"], c["step"]
    rec = capturing.StreamingRecorder(det, lead_ms=30.0, capacity=8, pcm=True)
    x = torch.zeros((S, step), dtype=torch.float32, device=Cm.device_of(emu_lib))
    shared = {"select_count_kernel", "select_scan_kernel"}
    with Log(emu_lib) as g:
        rec.push(x, det.out)
    assert [kernel_of(e) for e in g.entries] == ["capture_flag_kernel", "select_count_kernel", "select_scan_kernel", "capture_emit_kernel",
                                                 "capture_gather_kernel", "capture_append_kernel"], g.entries
    with Log(emu_lib) as g:
        rec.push([x[s] for s in range(S)], scanning.RaggedScanOutput(None, None, None, det.out.top, det.out.score, det.out.is_new,
                                                                       np.arange(S + 1)))
        rec.flush()
    names = {kernel_of(e) for e in g.entries}
    assert names == shared | {"capture_flag_kernel", "capture_emit_kernel", "capture_gather_kernel", "capture_append_kernel",
                              "capture_clear_kernel"}, names


# ---- MI355X ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lead", LEADS)
def test_gpu_any_split_equals_the_whole(hip_lib, lead):
    for step, n in ((5, 37), (8, 40)):
        for ragged in (False, True):
            check_split(hip_lib, step, n, lead, ragged)


@pytest.mark.gpu
def test_gpu_ragged_reset_flush_mask_capacity_pcm(hip_lib):
    for lead in (0, 12):
        check_ragged(hip_lib, lead)
    check_reset_flush(hip_lib)
    check_mask_capacity_refusals(hip_lib)
    check_pcm(hip_lib)
    check_many_clips(hip_lib)


@pytest.mark.gpu
def test_gpu_recorder_next_to_real_detectors(hip_lib):
    check_live(hip_lib)
    check_python_refusals(hip_lib)
    check_python_reset_flush(hip_lib)
    check_live_phrases(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("lead_ms", [0, 500])
def test_gpu_mid_size_64_streams(hip_lib, lead_ms):
    """S = 64, one-second clips, about 1 % random triggers, 40 mixed calls (one row, many rows, ragged with idle streams)."""
    S, step, n, lead = 64, 320, 16000, lead_ms * 16
    rng = np.random.RandomState(100 + lead_ms)
    raw, ref = Raw(hip_lib, S, step, n, lead, capacity=128, max_rows=S * 64), Reference(S, step, n, lead)
    emitted = wraps = 0
    heard = np.zeros(S, np.int64)
    for call in range(40):
        kind = call % 4
        rows = np.full(S, 1 if kind in (0, 1) else int(rng.randint(2, 64)))
        if kind == 3:
            rows = rng.randint(0, 40, S)
            rows[rng.rand(S) < 0.3] = 0
        samples = [rng.uniform(-1, 1, r * step).astype(np.float32) for r in rows]
        top = [rng.randint(0, NCLS, r).astype(np.int32) for r in rows]
        score = [rng.rand(r).astype(np.float32) for r in rows]
        is_new = [(rng.rand(r) < 0.01).astype(np.int32) for r in rows]
        reset = (rng.rand(S) < 0.05).astype(np.uint8) if call % 7 == 6 else None
        want = ref.push(samples, top, score, is_new, reset=reset)
        got, due = raw.push(samples, top, score, is_new, reset=reset, ragged=kind == 3)
        assert due == len(want)
        same(got, want)
        emitted += len(want)
        heard += rows
    want = ref.flush()
    got, due = raw.flush()
    same(got, want)
    assert emitted >= 60 and heard.max() * step > 2 * raw.R and due == len(want)
    assert lead > 0 or due == 0


@pytest.mark.gpu
def test_gpu_stream_audio_capture_dir(hip_lib, tmp_path):
    """stream_audio.py --capture_dir: the files named in mine_audio.py's layout hold the int16 slices of the input, and stdout is the
    run's without the flag."""
    from tcresnet_amd.audio_input import WavFile, format_time_ms
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    audio = segment_audio(2, 64000, 11)
    pcm = [np.clip(audio[0] * 32767, -32768, 32767).astype(np.int16), np.clip(audio[1, :41234] * 32767, -32768, 32767).astype(np.int16)]
    wavs = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    labels = [f"c{i}" for i in range(12)]
    cmd = [sys.executable, os.path.join(ROOT, "tc-resnet_amd", "stream_audio.py"), "--frozen", path, "--wav", *wavs, "--labels", ",".join(labels),
           "--frames_per_step", "2", "--average_window_ms", "200", "--min_count", "2", "--detection_threshold", "0.3", "--suppression_ms", "400"]
    out_dir = tmp_path / "clips"
    lead_ms = 100
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    cap = subprocess.run(cmd + ["--capture_dir", str(out_dir), "--capture_lead_ms", str(lead_ms)], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and cap.returncode == 0, cap.stderr
    assert cap.stdout == plain.stdout
    lines = [ln.split(",") for ln in plain.stdout.strip().splitlines()]
    kept = [ln for ln in lines if labels.index(ln[2]) >= 2]
    assert len(kept) >= 2
    files = sorted(str(p) for p in out_dir.rglob("*.wav"))
    expect = {}
    for f, t, lab, _ in kept:
        stem = os.path.splitext(os.path.basename(f))[0]
        end = int(round(float(t) * 16)) + lead_ms * 16
        x = pcm[wavs.index(f)]
        src = np.concatenate([x[:len(x) // 640 * 640], np.zeros(64000 + 16000, np.int16)])       # (whole steps; then zeros)
        clip = np.zeros(16000, np.int16)
        lo = max(end - 16000, 0)
        clip[16000 - (end - lo):] = src[lo:end]
        expect[str(out_dir / lab / f"{stem}_{format_time_ms(float(t))}.wav")] = clip
    assert files == sorted(expect)
    for f, clip in expect.items():
        wav = WavFile(f)
        assert (wav.rate, wav.channels, wav.length) == (16000, 1, 16000)
        assert np.array_equal(wav.read_pcm(0, 16000), clip), f
