"""Streaming template matching (tcr_dtw_stream_push / _push_ragged, tcresnet_amd.scanning.StreamingTemplateDetector): however a
stream's rows are cut into pushes -- one step at a time, dense, ragged with streams that sit a call out, resets in between -- its
posteriors, lengths and detections are bitwise the whole scan's: tests/dtw_ref.py's `scores` and tests/phrase_ref.py's `detect_rule`
over everything pushed to the stream since its start or reset.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`).  Every comparison
is bitwise, on all five outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests import dtw_ref as DR
from tests import phrase_ref as PR
from tests.test_phrases import DET, planted_rows, same
from tests.test_scan import scanning
from tests.test_streaming import segment_audio, setup, streaming
from tests.test_templates import MARK, at_rate, walk_rows

SUPP, THR = 3, 0.6
S = 5
# The schedules: rows per stream and call.  One-step pushes, many-step pushes and ragged pushes with streams that bring nothing, mixed;
# the same amounts for every stream go through the dense entry (call 8: through the ragged one all the same).
CALLS = [[1] * S, [4] * S, [0, 3, 9, 1, 0], [5] * S, [1] * S, [70, 0, 2, 6, 1], [2] * S, [1] * S, [7] * S, [0, 0, 0, 0, 3], [1] * S, [66] * S]
RAGGED_ANYWAY = 8
RESETS = {3: [0], 5: [1, 3], 6: [1], 10: [4]}              # call -> the streams asked to restart (call 5: stream 1 brings no rows: it stays pending)


def templates_for(F, seed=5):
    """Four templates, one, two and three frames a lane among them; the middle keyword has two."""
    rng = np.random.RandomState(seed)
    tm = [walk_rows(rng, L, F) for L in (1, 3, 65, 130)]
    return tm, np.array([0, 1, 3, 4], np.int32), np.array([np.float32(0.5 / len(t)) for t in tm], np.float32)


class Carried:
    """A template stream state of the library and its push calls on host arrays."""

    def __init__(self, lib, n_streams, F, tm, kw_off, scale, max_steps=0, supp=SUPP, thr=THR):
        self.lib, self.dev, self.S, self.F = lib, Cm.device_of(lib), n_streams, F
        self.flat = torch.from_numpy(np.concatenate(tm)).to(self.dev)
        self.fo = np.concatenate([[0], np.cumsum([len(t) for t in tm])]).astype(np.int32)
        self.kw, self.scale = np.ascontiguousarray(kw_off, np.int32), np.ascontiguousarray(scale, np.float32)
        self.K = len(self.kw) - 1
        self.cfg, self.det = T._lib.DtwCfg(max_steps), T._lib.DetectCfg(1, 1, supp, thr)
        n = lib.tcr_dtw_stream_state_bytes(n_streams, F, *self.tables())
        assert n > 0 and n % 4 == 0, lib.tcr_last_error()
        self.state = torch.empty(n // 4, dtype=torch.float32, device=self.dev)
        lib.check(lib.tcr_dtw_stream_init(n_streams, F, *self.tables(), self.state.data_ptr(), None), "tcr_dtw_stream_init")

    def tables(self):
        return len(self.fo) - 1, self.flat.data_ptr(), self.fo.ctypes.data, self.K, self.kw.ctypes.data, self.scale.ctypes.data, C.byref(self.cfg)

    def outputs(self, rows):
        i32 = dict(dtype=torch.int32, device=self.dev)
        return (torch.full((rows, self.K + 1), MARK, device=self.dev), torch.full((rows, self.K), int(MARK), **i32),
                torch.full((rows,), int(MARK), **i32), torch.full((rows,), MARK, device=self.dev), torch.full((rows,), int(MARK), **i32))

    def stream_state(self, s):
        """The bytes of stream s in the state (include/tcresnet_hip.h): its five integers, its D and n of every template."""
        raw = self.state.view(torch.int32).cpu().numpy()
        ints = -(-self.S * 5 * 4 // 256) * 256 // 4
        total = int(self.fo[-1])
        parts = [raw[:5 * self.S].reshape(5, self.S)[:, s]]
        for base in (ints, ints + total * self.S):
            for q in range(len(self.fo) - 1):
                L = int(self.fo[q + 1] - self.fo[q])
                at = base + int(self.fo[q]) * self.S + s * L
                parts.append(raw[at:at + L])
        assert ints + 2 * total * self.S == raw.size
        return np.concatenate(parts).copy()

    def push(self, chunks, reset=None, ragged=None):
        """chunks: per stream its new rows [m_s, F] -> per stream (post, lengths, top, score, is_new) of those rows; dense when every
        stream brings the same number of rows (ragged=True: the ragged entry all the same)."""
        m = [len(c) for c in chunks]
        ragged = len(set(m)) > 1 if ragged is None else ragged
        v = torch.from_numpy(np.ascontiguousarray(np.concatenate([c for c in chunks if len(c)]), np.float32)).to(self.dev)
        outs = self.outputs(sum(m))
        rs = None if reset is None else torch.from_numpy(np.asarray(reset, np.uint8)).to(self.dev)
        tail = (*self.tables(), C.byref(self.det), None if rs is None else rs.data_ptr(), self.state.data_ptr(), *(t.data_ptr() for t in outs), None)
        off = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
        if ragged:
            so = torch.from_numpy(off).to(self.dev)
            self.lib.check(self.lib.tcr_dtw_stream_push_ragged(self.S, so.data_ptr(), sum(m), self.F, v.data_ptr(), *tail), "push_ragged")
        else:
            self.lib.check(self.lib.tcr_dtw_stream_push(self.S, m[0], self.F, v.data_ptr(), *tail), "push")
        host = [t.cpu().numpy() for t in outs]
        return [tuple(t[a:b] for t in host) for a, b in zip(off[:-1], off[1:])]


def whole(rows, tm, kw_off, scale, max_steps=0, supp=SUPP, thr=THR):
    """The reference of one stream: the whole scan of its rows -> (post, lengths, top, score, is_new)."""
    post, lengths = DR.scores(rows, [0, len(rows)], tm, kw_off, scale, max_steps)
    return (post, lengths, *PR.detect_rule(post, supp, thr))


def same5(got, want, at, what):
    n = len(got[0])
    for g, r, name in zip(got, want, ("post", "lengths", "top", "score", "is_new")):
        same(g, r[at:at + n], (*what, name, at))


# ---- 1. any schedule equals the whole ---------------------------------------------------------------------------------------------------
def check_schedule(lib, F=12, max_steps=0):
    """S = 5 streams through CALLS with RESETS: every push's rows are the whole scan's of the stream's rows since its last reset; a
    stream that sits a call out keeps every byte of its state, whatever its reset flag says."""
    rng = np.random.RandomState(40 + F)
    tm, kw_off, scale = templates_for(F)
    total = np.sum(CALLS, axis=0)
    streams = []
    for s in range(S):
        rows = planted_rows(rng, int(total[s]), F)
        pos = 2 + s
        for piece in (at_rate(tm[1], 1), at_rate(tm[2], 2), at_rate(tm[1], 0.5), at_rate(tm[3], 2), at_rate(tm[2], 1)):
            if pos + len(piece) <= len(rows):
                rows[pos:pos + len(piece)] = piece
            pos += len(piece) + s % 3
        streams.append(rows)
    st = Carried(lib, S, F, tm, kw_off, scale, max_steps)
    at, since, pending = [0] * S, [0] * S, np.zeros(S, np.uint8)
    fired = skipped = 0
    for j, m in enumerate(CALLS):
        pending[RESETS.get(j, [])] = 1
        idle = [s for s in range(S) if m[s] == 0]
        before = {s: st.stream_state(s) for s in idle}
        got = st.push([streams[s][at[s]:at[s] + m[s]] for s in range(S)], reset=pending.copy() if pending.any() else None,
                      ragged=True if j == RAGGED_ANYWAY else None)
        for s in idle:
            assert np.array_equal(st.stream_state(s), before[s]), (j, s)
            skipped += 1
        for s in range(S):
            if m[s] == 0:
                continue
            if pending[s]:
                since[s], pending[s] = at[s], 0
            want = whole(streams[s][since[s]:at[s] + m[s]], tm, kw_off, scale, max_steps)
            same5(got[s], want, at[s] - since[s], ("schedule", F, j, s))
            fired += int(got[s][4].sum())
            at[s] += m[s]
    assert fired >= 8 and skipped >= 5 and since == [5, 14, 0, 12, 25], (fired, skipped, since)


def test_any_schedule_equals_the_whole(emu_lib):
    check_schedule(emu_lib)
    check_schedule(emu_lib, F=3, max_steps=60)


def check_single_rows(lib, n_streams, n=24, F=12):
    """One-step pushes only, more streams than a wave has lanes or a single one."""
    rng = np.random.RandomState(5 * n_streams)
    tm, kw_off, scale = templates_for(F)
    tm, kw_off, scale = tm[:3], np.array([0, 1, 3], np.int32), scale[:3]
    streams = [planted_rows(rng, n, F) for _ in range(n_streams)]
    for rows in streams[::2]:
        rows[4:7] = tm[1]
    want = [whole(rows, tm, kw_off, scale) for rows in streams]
    st = Carried(lib, n_streams, F, tm, kw_off, scale)
    for i in range(n):
        got = st.push([rows[i:i + 1] for rows in streams])
        for s in range(n_streams):
            same5(got[s], want[s], i, ("single rows", n_streams, s))


@pytest.mark.parametrize("n_streams", [65, 1])
def test_many_single_row_pushes(emu_lib, n_streams):
    check_single_rows(emu_lib, n_streams)


# ---- 2. end to end on a small real model ------------------------------------------------------------------------------------------------
def check_real_streams(lib, k=2):
    """S = 5 streams of a real `StreamingDetector` through `StreamingTemplateDetector.push`: one-step pushes, `push_many` and ragged
    pushes with streams that bring nothing, and a reset that stays pending over such a push; every stream's rows and lengths are
    `TemplateDetector.detect` of one scan of its audio since its reset."""
    Sc, St = scanning(), streaming()
    fe, net, _, _, _ = setup(lib)
    scanner = Sc.KeywordScanner(net, fe, frames_per_step=k, **DET)
    live = St.StreamingDetector(net, fe, S, frames_per_step=k, **DET)
    step, n = scanner.step_samples, 36
    audio = Cm.to_dev(lib, segment_audio(S, n * step, 43))
    scan = scanner.scan(audio)
    sm = scan.smoothed.cpu().numpy()
    kt = Sc.KeywordTemplates()
    kt.add("a", sm[0, 6:14])
    kt.add("b", sm[1, 20:31])
    kt.add("a", sm[3, 2:7])
    td = Sc.TemplateDetector(scanner, kt, detection_threshold=0.8, suppression_ms=2 * scanner.step_ms)
    sp = td.streaming(S)
    assert isinstance(sp, Sc.StreamingTemplateDetector) and sp.labels == ["a", "b", "_background_"] and sp.num_classes == 3
    fields = ("probs", "top", "score", "is_new")
    parts = [{f: [] for f in (*fields, "lengths")} for _ in range(S)]

    def keep(s, out, sl, lengths):
        for f in fields:
            parts[s][f].append(getattr(out, f)[sl].clone())
        parts[s]["lengths"].append(lengths[sl].clone())
    at = [0] * S
    for i in range(3):                                      # one step at a time: the detector's own tensors, overwritten by the next
        one = sp.push(live.push(audio[:, i * step:(i + 1) * step].contiguous()))
        assert one is sp.out and one.logits is None and one.smoothed is one.probs and one.probs.shape == (S, 3) and sp.lengths.shape == (S, 2)
        for s in range(S):
            keep(s, one, slice(s, s + 1), sp.lengths)
            at[s] += 1
    many = sp.push(live.push_many(audio[:, 3 * step:12 * step].contiguous()))
    assert isinstance(many, Sc.ScanOutput) and many.probs.shape == (S, 9, 3) and sp.lengths.shape == (S, 9, 2)
    for s in range(S):
        keep(s, many, s, sp.lengths)
        at[s] += 9
    since = [0] * S
    for j, m in enumerate(([3, 0, 2, 0, 1], [4, 5, 0, 6, 2], [17, 19, 22, 18, 21])):
        if j == 0:                                          # stream 1 brings nothing in this push: its reset waits for its next row
            live.reset([1, 2])
            sp.reset([1, 2])
        out = live.push_ragged([audio[s, at[s] * step:(at[s] + m[s]) * step].contiguous() for s in range(S)])
        rag = sp.push(out)
        assert isinstance(rag, Sc.RaggedScanOutput) and rag.logits is None and rag.smoothed is rag.probs and np.array_equal(rag.offsets, out.offsets)
        if j == 0:
            assert sp._pending is not None and sp._pending.tolist() == [False, True, False, False, False]
            since[2] = at[2]
        if j == 1:
            assert sp._pending is None
            since[1] = at[1]
        for s in range(S):
            if m[s] and since[s] == at[s] and since[s] > 0:  # the stream starts again here
                for f in parts[s]:
                    parts[s][f] = []
            keep(s, rag, slice(int(rag.offsets[s]), int(rag.offsets[s + 1])), sp.lengths)
            at[s] += m[s]
    assert at == [n] * S and since == [0, 12, 12, 0, 0]
    fired = 0
    for s in range(S):
        want, wlen = td.detect(scanner.scan(audio[s:s + 1, since[s] * step:].contiguous()), return_lengths=True)
        for f in fields:
            assert torch.equal(torch.cat(parts[s][f]), getattr(want, f)[0]), (s, f)
        assert torch.equal(torch.cat(parts[s]["lengths"]), wlen[0]), s
        fired += int((want.is_new[0] != 0).sum())
    assert fired >= 4
    whole_det = td.detect(scan)
    assert float(whole_det.probs[0, 13, 0]) == 1.0 and float(whole_det.probs[1, 30, 1]) == 1.0
    return Sc, scanner, td, audio, scan


def test_real_streams_equal_the_scan(emu_lib):
    check_real_streams(emu_lib)


def check_recorder(lib):
    """A `StreamingRecorder` next to the template detector: the clips of its detections are `TemplateDetector.mine`'s."""
    from tcresnet_amd import capturing
    Sc, St = scanning(), streaming()
    fe, net, _, _, _ = setup(lib)
    scanner = Sc.KeywordScanner(net, fe, **DET)
    det = St.StreamingDetector(net, fe, S, **DET)
    step, n = scanner.step_samples, 70
    audio = Cm.to_dev(lib, segment_audio(S, n * step, 44))
    scan = scanner.scan(audio)
    sm = scan.smoothed.cpu().numpy()
    kt = Sc.KeywordTemplates()
    kt.add("a", sm[0, 10:22])
    kt.add("b", sm[1, 40:55])
    td = Sc.TemplateDetector(scanner, kt, detection_threshold=0.7, suppression_ms=2 * scanner.step_ms)
    live = td.streaming(S)
    rec = capturing.StreamingRecorder(live, capacity=256)
    got = []
    for a, b in [(0, 1), (1, 20), (20, n)]:
        x = audio[:, a * step:b * step].contiguous()
        out = live.push(det.push(x) if b - a == 1 else det.push_many(x))
        h = rec.push(x, out).host()
        got += [(int(s), int(i), int(l), clip.copy()) for s, i, l, clip in zip(h.stream, h.step, h.label, h.clips)]
    mined = td.mine(scan, audio, k=1000)                    # no events: every keyword detection is a false accept
    want = {(int(s), int(i), int(l)): c for s, i, l, c in zip(mined.signal, mined.step, mined.label, mined.clips.cpu().numpy())}
    assert len(want) >= 2 and sorted(g[:3] for g in got) == sorted(want)
    for g in got:
        assert np.array_equal(g[3].view(np.int32), want[g[:3]].view(np.int32)), g[:3]


def test_recorder_clips_equal_mine(emu_lib):
    check_recorder(emu_lib)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------
def test_c_refusals_touch_nothing(emu_lib):
    lib, F, n_streams, steps = emu_lib, 4, 2, 6
    rng = np.random.RandomState(2)
    tm = [walk_rows(rng, 5, F), walk_rows(rng, 3, F)]
    kw, sc = np.array([0, 1, 2], np.int32), np.array([0.1, 0.2], np.float32)
    st = Carried(lib, n_streams, F, tm, kw, sc)
    rows = planted_rows(rng, n_streams * steps, F)
    st.push([rows[:steps], rows[steps:]])                    # a state with history in it
    v = torch.from_numpy(rows).to(st.dev)
    so = torch.from_numpy(np.array([0, 5, 12], np.int64)).to(st.dev)
    state0 = st.state.clone()

    def call(msg, n=n_streams, m=steps, F_=F, fo=st.fo, kw=kw, sc=sc, max_steps=0, det=(1, 1, 3, 0.2), hole=None, ragged=False, Q=None, K=None):
        fo, kw, sc = np.ascontiguousarray(fo, np.int32), np.ascontiguousarray(kw, np.int32), np.ascontiguousarray(sc, np.float32)
        cfg, d = T._lib.DtwCfg(max_steps), T._lib.DetectCfg(*det)
        outs = st.outputs(n_streams * steps)
        args = [v.data_ptr(), len(fo) - 1 if Q is None else Q, st.flat.data_ptr(), fo.ctypes.data, len(kw) - 1 if K is None else K, kw.ctypes.data,
                sc.ctypes.data, C.byref(cfg), C.byref(d), None, st.state.data_ptr(), *(t.data_ptr() for t in outs), None]
        if isinstance(hole, int):
            args[hole] = None
        if ragged:
            rc = lib.tcr_dtw_stream_push_ragged(n, None if hole == "offsets" else so.data_ptr(), m, F_, *args)
        else:
            rc = lib.tcr_dtw_stream_push(n, m, F_, *args)
        name = "tcr_dtw_stream_push_ragged: " if ragged else "tcr_dtw_stream_push: "
        err = lib.tcr_last_error().decode()
        assert rc == -1 and name in err and msg in err, (msg, rc, err)
        assert all(bool((t == MARK).all()) for t in outs), msg
        assert st.state.view(torch.int32).equal(state0.view(torch.int32)), msg

    for ragged, m in ((False, steps), (True, 12)):
        kwargs = dict(ragged=ragged, m=m)
        for hole in (0, 2, 3, 5, 6, 7, 8, 10, 11, 13, 14, 15):      # values, the tables, cfg, det, state, post, top, score, is_new (not lengths)
            call("null argument", hole=hole, **kwargs)
        call("n_features must be positive (got 0)", F_=0, **kwargs)
        call("n_features 65 above TCR_DTW_MAX_FEATURES = 64", F_=65, **kwargs)
        call("n_templates 0 outside 1..64", Q=0, **kwargs)
        call("n_templates 65 outside 1..64", Q=65, **kwargs)
        call("n_keywords 0 outside 1..2", K=0, **kwargs)
        call("n_keywords 3 outside 1..2", K=3, **kwargs)
        call("frame_offsets must start at 0 (got 1)", fo=[1, 5, 8], **kwargs)
        call("frame_offsets decrease at template 1 (4 after 5)", fo=[0, 5, 4], **kwargs)
        call("template 0 has 0 frames", fo=[0, 0, 8], **kwargs)
        call("template 0 has 257 frames (1..tcr_dtw_frames_max(4) = 256)", fo=[0, 257, 260], **kwargs)
        call("keyword_offsets must start at 0 (got 1)", kw=[1, 2, 2], **kwargs)
        call("keyword_offsets decrease at keyword 1 (0 after 1)", kw=[0, 1, 0], **kwargs)
        call("keyword 1 has no template", kw=[0, 2, 2], **kwargs)
        call("keyword_offsets must end at n_templates = 2 (got 1)", kw=[0, 1], **kwargs)
        for bad in (0.0, -1.0, np.inf, np.nan):
            call("scale[0] = ", sc=[bad, 0.2], **kwargs)
        call("max_steps must be >= 0 (got -2)", max_steps=-2, **kwargs)
        call("average_steps and min_count must be 1 (got 2, 1)", det=(2, 1, 3, 0.2), **kwargs)
        call("average_steps and min_count must be 1 (got 1, 0)", det=(1, 0, 3, 0.2), **kwargs)
        call("suppression_steps must be >= 0 (got -1)", det=(1, 1, -1, 0.2), **kwargs)
        call("the number of streams must be positive (got 0)", n=0, **kwargs)
        call("the number of steps must be positive (got 0)", ragged=ragged, m=0)
        call("the number of steps must be positive (got -3)", ragged=ragged, m=-3)
        call("is too large", ragged=ragged, m=(1 << 31) // 4)
    call("null argument", hole="offsets", ragged=True, m=12)
    # the size query and the init
    assert st.state.numel() * 4 == 256 + 8 * 8 * n_streams     # the integers' 256 bytes, then D and n of 8 frames a stream
    cfg = T._lib.DtwCfg(0)
    tables = lambda fo=st.fo, cfg=cfg: (2, st.flat.data_ptr(), np.ascontiguousarray(fo, np.int32).ctypes.data, 2, kw.ctypes.data, sc.ctypes.data,
                                        None if cfg is None else C.byref(cfg))
    assert lib.tcr_dtw_stream_state_bytes(n_streams, F, *tables()) == st.state.numel() * 4
    assert lib.tcr_dtw_stream_state_bytes(0, F, *tables()) == 0
    assert "tcr_dtw_stream_state_bytes: the number of streams must be positive" in lib.tcr_last_error().decode()
    assert lib.tcr_dtw_stream_state_bytes(n_streams, F, *tables(cfg=None)) == 0
    bad_fo = np.array([0, 0, 8], np.int32)
    assert lib.tcr_dtw_stream_state_bytes(n_streams, F, *tables(fo=bad_fo)) == 0 and "template 0 has 0 frames" in lib.tcr_last_error().decode()
    assert lib.tcr_dtw_stream_init(n_streams, F, *tables(), None, None) == -1
    assert lib.tcr_dtw_stream_init(n_streams, F, *tables(fo=bad_fo), st.state.data_ptr(), None) == -1
    assert st.state.view(torch.int32).equal(state0.view(torch.int32))
    # and the state still works
    more = planted_rows(np.random.RandomState(3), 4, F)
    got = st.push([more[:2], more[2:]])
    want = whole(np.concatenate([rows[:steps], more[:2]]), tm, kw, sc)
    same5(got[0], want, steps, ("after the refusals",))


def test_python_refusals(emu_lib):
    Sc, St = scanning(), streaming()
    fe, net, _, _, _ = setup(emu_lib)
    scanner = Sc.KeywordScanner(net, fe, **DET)
    kt = Sc.KeywordTemplates()
    kt.add("a", walk_rows(np.random.RandomState(1), 6, 12))
    td = Sc.TemplateDetector(scanner, kt)
    sp = td.streaming(3)
    dev = Cm.device_of(emu_lib)
    sm = torch.rand(3, 5, 12, device=dev)
    good = Sc.ScanOutput(None, sm, sm, None, None, None)
    assert sp.push(good).top.shape == (3, 5) and sp.lengths.shape == (3, 5, 1)
    with pytest.raises(T.TcrError, match="on must be 'smoothed' or 'probs'"):
        sp.push(good, on="logits")
    with pytest.raises(T.TcrError, match="is not over the detector's 12 classes"):
        sp.push(Sc.ScanOutput(None, sm[..., :5].contiguous(), sm[..., :5].contiguous(), None, None, None))
    with pytest.raises(T.TcrError, match="is not a push of 3 streams"):
        sp.push(Sc.ScanOutput(None, sm[:2].contiguous(), sm[:2].contiguous(), None, None, None))
    with pytest.raises(T.TcrError, match="is not a push of 3 streams"):
        sp.push(St.StreamOutput(None, sm, sm, None, None, None))          # one step is [S, classes]
    flat = sm.reshape(15, 12)
    with pytest.raises(T.TcrError, match="is not a push of 3 streams"):
        sp.push(Sc.RaggedScanOutput(None, flat, flat, None, None, None, np.array([0, 7, 15], np.int64)))
    with pytest.raises(T.TcrError, match="reset mask must have 3 entries"):
        sp.reset(np.zeros(4, bool))
    empty = sp.push(Sc.RaggedScanOutput(None, flat[:0], flat[:0], None, None, None, np.zeros(4, np.int64)))
    assert empty.top.shape == (0,) and empty.probs.shape == (0, 2) and sp.lengths.shape == (0, 1)


# ---- MI355X -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_any_schedule_equals_the_whole(hip_lib):
    check_schedule(hip_lib)
    check_schedule(hip_lib, F=3, max_steps=60)


@pytest.mark.gpu
@pytest.mark.parametrize("n_streams", [65, 1])
def test_gpu_many_single_row_pushes(hip_lib, n_streams):
    check_single_rows(hip_lib, n_streams)


@pytest.mark.gpu
def test_gpu_real_streams_equal_the_scan(hip_lib):
    check_real_streams(hip_lib)


@pytest.mark.gpu
def test_gpu_recorder_clips_equal_mine(hip_lib):
    check_recorder(hip_lib)
