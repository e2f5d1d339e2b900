"""Streaming phrase detection (tcr_phrase_stream_push / _push_ragged, tcresnet_amd.scanning.StreamingPhraseDetector): however a
stream's rows are cut into pushes -- dense, ragged, one step at a time, with resets in between -- its posteriors and detections are
bitwise the whole scan's: tests/phrase_ref.py's `scores` and `detect_rule` over everything pushed to the stream since its start or
reset.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`).  Every comparison is bitwise, on all four outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests import phrase_ref as PR
from tests.test_phrases import (DET, MODES, PRODUCT, TILE, cli_case, in_process, phrases_for, planted_rows, same, table, top_words)
from tests.test_scan import scanning
from tests.test_streaming import segment_audio, setup, streaming

SUPP, THR = 3, 0.2              # the detector of the raw cases: phrases fire, are suppressed, and fire again on these rows
MARK = -7.0                     # what the outputs hold before a call


class Carried:
    """A phrase stream state of the library and its push calls on host arrays."""

    def __init__(self, lib, S, ncls, phrases, w, ordered, combine, supp=SUPP, thr=THR):
        self.lib, self.dev, self.S, self.ncls, self.P = lib, Cm.device_of(lib), S, ncls, len(phrases)
        self.off, self.words = table(phrases)
        self.cfg = T._lib.PhraseCfg(w, ordered, combine)
        self.det = T._lib.DetectCfg(1, 1, supp, thr)
        n = lib.tcr_phrase_stream_state_bytes(S, ncls, *self.tables())
        assert n > 0 and n % 4 == 0, lib.tcr_last_error()
        self.state = torch.empty(n // 4, dtype=torch.float32, device=self.dev)
        lib.check(lib.tcr_phrase_stream_init(S, ncls, *self.tables(), self.state.data_ptr(), None), "tcr_phrase_stream_init")

    def tables(self):
        return self.P, self.off.ctypes.data, self.words.ctypes.data, C.byref(self.cfg)

    def outputs(self, rows):
        return (torch.full((rows, self.P + 1), MARK, device=self.dev), torch.full((rows,), int(MARK), dtype=torch.int32, device=self.dev),
                torch.full((rows,), MARK, device=self.dev), torch.full((rows,), int(MARK), dtype=torch.int32, device=self.dev))

    def push(self, chunks, reset=None, ragged=None):
        """chunks: per stream its new rows [m_s, C] -> per stream (post, top, score, is_new) of those rows; dense when every stream
        brings the same number of rows (ragged=True: the ragged entry all the same)."""
        m = [len(c) for c in chunks]
        ragged = len(set(m)) > 1 if ragged is None else ragged
        v = torch.from_numpy(np.ascontiguousarray(np.concatenate([c for c in chunks if len(c)]), np.float32)).to(self.dev)
        outs = self.outputs(sum(m))
        rs = None if reset is None else torch.from_numpy(np.asarray(reset, np.uint8)).to(self.dev)
        tail = (*self.tables(), C.byref(self.det), None if rs is None else rs.data_ptr(), self.state.data_ptr(), *(t.data_ptr() for t in outs), None)
        off = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
        if ragged:
            so = torch.from_numpy(off).to(self.dev)
            self.lib.check(self.lib.tcr_phrase_stream_push_ragged(self.S, so.data_ptr(), sum(m), self.ncls, v.data_ptr(), *tail), "push_ragged")
        else:
            self.lib.check(self.lib.tcr_phrase_stream_push(self.S, m[0], self.ncls, v.data_ptr(), *tail), "push")
        host = [t.cpu().numpy() for t in outs]
        return [tuple(t[a:b] for t in host) for a, b in zip(off[:-1], off[1:])]


def whole(rows, phrases, w, ordered, combine, supp=SUPP, thr=THR):
    """The reference of one stream: the whole scan of its rows -> (post, top, score, is_new)."""
    post = PR.scores(rows, [0, len(rows)], phrases, w, ordered, combine)
    return (post, *PR.detect_rule(post, supp, thr))


def same4(got, want, at, what):
    """The four outputs of a push (one stream's rows) against rows at .. of the stream's whole scan."""
    n = len(got[0])
    for g, r, name in zip(got, want, ("post", "top", "score", "is_new")):
        same(g, r[at:at + n], (*what, name, at))


def plant_12(rows, at, ncls):
    """ "1 2" with word 1 in rows `at` + TILE - 3 and - 2 and word 2 in rows `at` + TILE and + 1: across the tile boundary of a chunk
    that starts at row `at`."""
    for a, c in ((at + TILE - 3, 1), (at + TILE, 2)):
        rows[a:a + 2] = np.float32(0.1 / (ncls - 1))
        rows[a:a + 2, c] = np.float32(0.9)


def split_sizes(w):
    return [m for m in (1, 1, 2, w - 1, w, w + 1, 255, 256, 257) if m > 0]


# ---- 1. any split equals the whole --------------------------------------------------------------------------------------------------------
def check_split(lib, ncls, w, modes=MODES):
    """Three streams pushed in chunks of 1, 1, 2, w - 1, w, w + 1, 255, 256, 257 rows and the rest (more than a tile, so that the
    streams are about 900 rows plus three windows): history shorter than w - 1, exactly w - 1, the ring wrapping, and chunks that cross
    the tile boundary with "1 2" planted across it."""
    rng = np.random.RandomState(77 * ncls + w)
    sizes, phrases, S = split_sizes(w), phrases_for(ncls), 3
    sizes.append(TILE + 44)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    streams = [planted_rows(rng, int(starts[-1]), ncls) for _ in range(S)]
    for rows in streams:
        plant_12(rows, int(starts[-2]), ncls)               # in the rest
        plant_12(rows, int(starts[-3]), ncls)               # and in the chunk of 257: word 2 is its last row
    fired = 0
    for ordered, combine in modes:
        want = [whole(rows, phrases, w, ordered, combine) for rows in streams]
        fired += sum(int(x[3].sum()) for x in want)
        st = Carried(lib, S, ncls, phrases, w, ordered, combine)
        for at, m in zip(starts, sizes):
            got = st.push([rows[at:at + m] for rows in streams])
            for s in range(S):
                same4(got[s], want[s], at, (ncls, w, ordered, combine, s))
    assert fired >= 4 * len(modes)                          # (the detector has something to carry)


@pytest.mark.parametrize("w", [1, 2, 7, 256, 300])
@pytest.mark.parametrize("ncls", [3, 12])
def test_any_split_equals_the_whole(emu_lib, ncls, w):
    check_split(emu_lib, ncls, w)


# ---- 2. many single-row pushes ------------------------------------------------------------------------------------------------------------
def check_single_rows(lib, S, w, ncls=12, n=40):
    rng = np.random.RandomState(5 * S + w)
    phrases = phrases_for(ncls)
    assert n > 2 * (w - 1)
    streams = [planted_rows(rng, n, ncls) for _ in range(S)]
    for ordered, combine in MODES:
        want = [whole(rows, phrases, w, ordered, combine) for rows in streams]
        st = Carried(lib, S, ncls, phrases, w, ordered, combine)
        for i in range(n):
            got = st.push([rows[i:i + 1] for rows in streams])
            for s in range(S):
                same4(got[s], want[s], i, (S, w, ordered, combine, s))


@pytest.mark.parametrize("S,w", [(65, 2), (65, 7), (1, 2), (1, 7)])
def test_many_single_row_pushes(emu_lib, S, w):
    check_single_rows(emu_lib, S, w)


# ---- 3. ragged ----------------------------------------------------------------------------------------------------------------------------
def check_ragged(lib, w, ncls=12):
    """Six streams advance by [0, 1, w, 0, 257, 2] rows a call, the amounts rotated from call to call so that other streams sit out;
    a reset asked for a stream that sits out applies with its next rows, not before (and not to the state it left)."""
    rng = np.random.RandomState(31 + w)
    phrases, S, calls = phrases_for(ncls), 6, 7
    adv = [0, 1, w, 0, 257, 2]
    amounts = [[adv[(s + c) % S] for s in range(S)] for c in range(calls)]
    idle_reset = {2: 1}                                      # call 2 asks to reset stream 1, which brings adv[3] = 0 rows in it
    assert amounts[2][1] == 0 and amounts[3][1] > 0
    rows_in = [[planted_rows(rng, max(m, 1), ncls)[:m] for m in amounts[c]] for c in range(calls)]
    for ordered, combine in MODES:
        st = Carried(lib, S, ncls, phrases, w, ordered, combine)
        pieces, got, pending = [[] for _ in range(S)], [[] for _ in range(S)], np.zeros(S, np.uint8)
        for c in range(calls):
            if c in idle_reset:
                pending[idle_reset[c]] = 1
            before = st.state.clone()
            out = st.push(rows_in[c], reset=pending.copy() if pending.any() else None, ragged=True)
            if c in idle_reset:                             # the idle stream's flag was ignored: the call left its integers alone
                ints = lambda t: t[:5 * S].view(torch.int32).view(5, S)[:, idle_reset[c]]
                assert torch.equal(ints(st.state), ints(before))
            for s in range(S):
                if amounts[c][s] and pending[s]:
                    pieces[s], got[s], pending[s] = [], [], 0    # the reset applied: the stream starts again
                if amounts[c][s]:
                    pieces[s].append(rows_in[c][s])
                    got[s].append(out[s])
        for s in range(S):
            want = whole(np.concatenate(pieces[s]), phrases, w, ordered, combine)
            at = 0
            for piece in got[s]:
                same4(piece, want, at, ("ragged", w, ordered, combine, s))
                at += len(piece[0])
            assert at == len(want[0]) > 0
        assert len(pieces[1]) == 3                           # stream 1 restarted at call 3 and sat call 5 out: calls 3, 4 and 6


@pytest.mark.parametrize("w", [2, 7, 300])
def test_ragged_pushes(emu_lib, w):
    check_ragged(emu_lib, w)


# ---- 4. reset -----------------------------------------------------------------------------------------------------------------------------
def check_reset(lib, w=7, ncls=12):
    rng = np.random.RandomState(44)
    phrases, S = phrases_for(ncls), 4
    sizes, marked = [3, 20, 1, 300, 9], {1: [1, 3], 3: [3], 4: [0]}      # call -> the streams reset before its rows
    starts = np.concatenate([[0], np.cumsum(sizes)])
    streams = [planted_rows(rng, int(starts[-1]), ncls) for _ in range(S)]
    for ordered, combine in MODES:
        st = Carried(lib, S, ncls, phrases, w, ordered, combine)
        since = [0] * S
        for c, (at, m) in enumerate(zip(starts, sizes)):
            flags = np.zeros(S, np.uint8)
            flags[marked.get(c, [])] = 1
            for s in marked.get(c, []):
                since[s] = int(at)
            got = st.push([rows[at:at + m] for rows in streams], reset=flags if c in marked else None)
            for s in range(S):                               # a fresh signal from the stream's last reset on; stream 2 is never reset
                want = whole(streams[s][since[s]:at + m], phrases, w, ordered, combine)
                same4(got[s], want, int(at) - since[s], ("reset", ordered, combine, c, s))


def test_reset_restarts_marked_streams_only(emu_lib):
    check_reset(emu_lib)


# ---- 5. the three forms on one state ------------------------------------------------------------------------------------------------------
def test_dense_ragged_and_one_step_calls_interleave(emu_lib):
    """One state through one-step, dense and ragged calls in turn, with 4 and 5 rows a stream (the two kernels' border) among them."""
    lib, ncls, w, S = emu_lib, 12, 7, 5
    rng = np.random.RandomState(52)
    phrases = phrases_for(ncls)
    calls = [[1] * S, [4] * S, [0, 3, 9, 1, 0], [5] * S, [1] * S, [300, 0, 2, 6, 1], [2] * S, [1] * S, [7, 7, 7, 7, 7], [260] * S]
    total = np.sum(calls, axis=0)
    streams = [planted_rows(rng, int(n), ncls) for n in total]
    for ordered, combine in MODES:
        want = [whole(rows, phrases, w, ordered, combine) for rows in streams]
        st = Carried(lib, S, ncls, phrases, w, ordered, combine)
        at = [0] * S
        for j, m in enumerate(calls):
            got = st.push([streams[s][at[s]:at[s] + m[s]] for s in range(S)], ragged=True if j == 8 else None)
            for s in range(S):
                same4(got[s], want[s], at[s], ("mixed", ordered, combine, j, s))
                at[s] += m[s]


# ---- 6. end to end on a small real model --------------------------------------------------------------------------------------------------
def check_real_streams(lib, k):
    """check_real_scan's model and audio: the outputs of `StreamingDetector.push` x 5, `push_many` and two `push_ragged` calls go
    through `StreamingPhraseDetector.push`; concatenated they are `PhraseDetector.detect` of the scan of the same audio."""
    Sc, St = scanning(), streaming()
    fe, net, _, _, _ = setup(lib)
    scanner = Sc.KeywordScanner(net, fe, frames_per_step=k, **DET)
    live = St.StreamingDetector(net, fe, 2, frames_per_step=k, **DET)
    step, n = scanner.step_samples, 30
    audio = Cm.to_dev(lib, segment_audio(2, n * step, 41))
    scan = scanner.scan(audio)
    order = np.argsort(-scan.smoothed.cpu().numpy().reshape(-1, 12).mean(axis=0))
    words = [[int(order[0]), int(order[0])], [int(order[0]), int(order[1])], [int(order[1]), int(order[0])]]    # (the first one fires on this net)
    ph = Sc.PhraseDetector(scanner, words, window_ms=8 * scanner.step_ms, detection_threshold=0.05, suppression_ms=2 * scanner.step_ms)
    want = ph.detect(scan)
    sp = ph.streaming(2)
    assert isinstance(sp, Sc.StreamingPhraseDetector) and sp.labels == ph.labels and sp.num_classes == 4
    fields = ("probs", "top", "score", "is_new")
    parts = {f: [[], []] for f in fields}

    def keep(f, s, t):
        parts[f][s].append(t.clone())
    for i in range(5):                                      # one step at a time: the detector's own tensors, overwritten by the next
        one = sp.push(live.push(audio[:, i * step:(i + 1) * step].contiguous()))
        assert one is sp.out and one.logits is None and one.smoothed is one.probs and one.probs.shape == (2, 4)
        for f in fields:
            for s in range(2):
                keep(f, s, getattr(one, f)[s:s + 1])
    many = sp.push(live.push_many(audio[:, 5 * step:15 * step].contiguous()))
    assert isinstance(many, Sc.ScanOutput) and many.logits is None and many.smoothed is many.probs and many.probs.shape == (2, 10, 4)
    for f in fields:
        for s in range(2):
            keep(f, s, getattr(many, f)[s])
    at = [15, 15]
    for m in ([3, 0], [12, 15]):
        out = live.push_ragged([audio[s, at[s] * step:(at[s] + m[s]) * step].contiguous() for s in range(2)])
        rag = sp.push(out)
        assert isinstance(rag, Sc.RaggedScanOutput) and rag.logits is None and rag.smoothed is rag.probs
        assert np.array_equal(rag.offsets, out.offsets)
        for s in range(2):
            a, b = int(rag.offsets[s]), int(rag.offsets[s + 1])
            for f in fields:
                keep(f, s, getattr(rag, f)[a:b])
            at[s] += m[s]
    cat = {f: torch.stack([torch.cat(parts[f][s]) for s in range(2)]) for f in fields}
    for f in fields:
        assert cat[f].shape == getattr(want, f).shape and torch.equal(cat[f], getattr(want, f)), (k, f)
    assert int(want.is_new.sum()) >= 2 and int((want.top[want.is_new != 0] < 3).sum()) >= 1      # phrases fire, not only the background
    assert not torch.equal(want.probs[..., 1], want.probs[..., 2])                                # and "a b" is not "b a" on this scan
    joined = Sc.ScanOutput(None, cat["probs"], cat["probs"], cat["top"], cat["score"], cat["is_new"])
    thr = [0.01, 0.05, 0.2]
    a, b = ph.sweep(joined, thr), ph.sweep(scan, thr)
    assert torch.equal(a.detections, b.detections) and int(a.detections.sum()) > 0
    on_probs = ph.streaming(2).push(scan, on="probs")
    assert torch.equal(on_probs.probs, ph.detect(scan, on="probs").probs)
    return Sc, ph, sp, live, audio, scan


@pytest.mark.parametrize("k", [1, 2])
def test_real_streams_equal_the_scan(emu_lib, k):
    check_real_streams(emu_lib, k)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_c_refusals_touch_nothing(emu_lib):
    lib, ncls, S, steps = emu_lib, 4, 2, 6
    dev = Cm.device_of(lib)
    ok = [[1, 2], [3]]
    st = Carried(lib, S, ncls, ok, 5, 1, PRODUCT)
    rows = planted_rows(np.random.RandomState(2), S * steps, ncls)
    st.push([rows[:steps], rows[steps:]])                    # a state with history in it
    v = torch.from_numpy(rows).to(dev)
    so = torch.from_numpy(np.array([0, 5, 12], np.int64)).to(dev)
    state0 = st.state.clone()

    def call(msg, n_streams=S, n=steps, C_=ncls, values=v, phrases=ok, off_words=None, w=5, ordered=1, combine=PRODUCT, det=(1, 1, 3, 0.2),
             state=True, hole=None, ragged=False, offsets=True):
        off, words = table(phrases) if off_words is None else off_words
        cfg, d = T._lib.PhraseCfg(w, ordered, combine), T._lib.DetectCfg(*det)
        outs = st.outputs(S * steps)
        args = [len(off) - 1, off.ctypes.data, words.ctypes.data, C.byref(cfg), C.byref(d), None, st.state.data_ptr() if state else None,
                *(t.data_ptr() for t in outs), None]
        if hole is not None:
            args[hole] = None
        if ragged:
            rc = lib.tcr_phrase_stream_push_ragged(n_streams, so.data_ptr() if offsets else None, n, C_, None if values is None else values.data_ptr(),
                                                   *args)
        else:
            rc = lib.tcr_phrase_stream_push(n_streams, n, C_, None if values is None else values.data_ptr(), *args)
        name = "tcr_phrase_stream_push_ragged: " if ragged else "tcr_phrase_stream_push: "
        assert rc == -1 and name in lib.tcr_last_error().decode() and msg in lib.tcr_last_error().decode(), (msg, rc, lib.tcr_last_error())
        assert all(bool((t == MARK).all()) for t in outs), msg
        assert st.state.view(torch.int32).equal(state0.view(torch.int32)), msg

    # everything tcr_phrase_scores refuses
    call("n_phrases 0 outside 1..64", phrases=[])
    call("n_phrases 65 outside 1..64", phrases=[[1]] * 65)
    call("phrase 1 has 0 words (1..8)", phrases=[[1], []])
    call("phrase 0 has 9 words (1..8)", phrases=[[1] * 9])
    call("phrase 1 word 0: class 4 outside 0..3", phrases=[[1, 2], [4]])
    call("phrase 0 word 1: class -1 outside 0..3", phrases=[[1, -1]])
    call("phrase_offsets must start at 0", off_words=(np.array([1, 2, 3], np.int32), np.array([1, 2, 3], np.int32)))
    call("phrase_offsets decrease at phrase 1", off_words=(np.array([0, 2, 1], np.int32), np.array([1, 2, 3], np.int32)))
    call("window_steps must be >= 1 (got 0)", w=0)
    wm = lib.tcr_phrase_window_max(3)
    call(f"window_steps {wm + 1} above tcr_phrase_window_max(3 distinct word classes) = {wm}", w=wm + 1)
    call("above tcr_phrase_window_max(65 distinct word classes)", C_=70, phrases=[list(range(8 * q, 8 * q + 8)) for q in range(8)] + [[64]], w=1)
    call("ordered must be 0 or 1 (got 2)", ordered=2)
    call("unknown combine 2", combine=2)
    call("num_classes must be positive (got 0)", C_=0)
    call("null argument", values=None)
    for hole in (1, 2, 3):                                   # phrase_offsets, phrase_words, cfg
        call("null argument", hole=hole)
    # the stream entries' own
    for hole in (4, 7, 8, 9, 10):                            # det, post, top, score, is_new
        call("null argument", hole=hole)
        call("null argument", hole=hole, ragged=True, n=12)
    call("null argument", state=False)
    call("null argument", ragged=True, n=12, offsets=False)
    call("average_steps and min_count must be 1 (got 2, 1)", det=(2, 1, 3, 0.2))
    call("average_steps and min_count must be 1 (got 1, 2)", det=(1, 2, 3, 0.2))
    call("average_steps and min_count must be 1 (got 1, 0)", det=(1, 0, 3, 0.2), ragged=True, n=12)
    call("suppression_steps must be >= 0 (got -1)", det=(1, 1, -1, 0.2))
    call("the number of streams must be positive (got 0)", n_streams=0)
    call("the number of streams must be positive (got -2)", n_streams=-2, ragged=True, n=12)
    call("the number of steps must be positive (got 0)", n=0)
    call("the number of steps must be positive (got -3)", n=-3)
    call("the number of steps must be positive (got 0)", ragged=True, n=0)
    call("is too large", n=(1 << 31) // 4)
    call("is too large", n_streams=2, n=1 << 30)
    call(f"{(1 << 31) // 4 + 1} steps in all x 4 columns is too large", ragged=True, n=(1 << 31) // 4 + 1)
    # the size query and the init
    off, words = table(ok)
    cfg = T._lib.PhraseCfg(5, 1, PRODUCT)
    assert lib.tcr_phrase_stream_state_bytes(S, ncls, 2, off.ctypes.data, words.ctypes.data, C.byref(cfg)) == st.state.numel() * 4
    assert st.state.numel() * 4 == 256 + 4 * 3 * S * 4          # the integers' 256 bytes, then w - 1 = 4 slots of U = 3 columns
    assert lib.tcr_phrase_stream_state_bytes(0, ncls, 2, off.ctypes.data, words.ctypes.data, C.byref(cfg)) == 0
    assert "tcr_phrase_stream_state_bytes: the number of streams must be positive" in lib.tcr_last_error().decode()
    assert lib.tcr_phrase_stream_state_bytes(S, ncls, 2, off.ctypes.data, words.ctypes.data, None) == 0
    cfg0 = T._lib.PhraseCfg(0, 1, PRODUCT)
    assert lib.tcr_phrase_stream_state_bytes(S, ncls, 2, off.ctypes.data, words.ctypes.data, C.byref(cfg0)) == 0
    assert "window_steps must be >= 1" in lib.tcr_last_error().decode()
    assert lib.tcr_phrase_stream_init(S, ncls, 2, off.ctypes.data, words.ctypes.data, C.byref(cfg), None, None) == -1
    assert lib.tcr_phrase_stream_init(S, ncls, 2, off.ctypes.data, words.ctypes.data, C.byref(cfg0), st.state.data_ptr(), None) == -1
    assert st.state.view(torch.int32).equal(state0.view(torch.int32))
    # and the state still works
    more = planted_rows(np.random.RandomState(3), 4, ncls)
    got = st.push([more[:2], more[2:]])
    want = whole(np.concatenate([rows[:steps], more[:2]]), ok, 5, 1, PRODUCT)
    same4(got[0], want, steps, ("after the refusals",))


def test_python_refusals(emu_lib):
    Sc, St = scanning(), streaming()
    fe, net, _, _, _ = setup(emu_lib)
    scanner = Sc.KeywordScanner(net, fe, **DET)
    ph = Sc.PhraseDetector(scanner, [[2, 3], [3, 2]], window_ms=300)
    with pytest.raises(T.TcrError, match="n_streams must be positive"):
        ph.streaming(0)
    sp = ph.streaming(3)
    dev = Cm.device_of(emu_lib)
    sm = torch.rand(3, 5, 12, device=dev)
    good = Sc.ScanOutput(None, sm, sm, None, None, None)
    assert sp.push(good).top.shape == (3, 5)
    with pytest.raises(T.TcrError, match="on must be 'smoothed' or 'probs'"):
        sp.push(good, on="logits")
    with pytest.raises(T.TcrError, match="is not over the detector's 12 classes"):
        sp.push(Sc.ScanOutput(None, sm[..., :5].contiguous(), sm[..., :5].contiguous(), None, None, None))
    with pytest.raises(T.TcrError, match="is not over the detector's 12 classes"):
        sp.push(Sc.ScanOutput(None, None, None, None, None, None))
    with pytest.raises(T.TcrError, match="is not a push of 3 streams"):
        sp.push(Sc.ScanOutput(None, sm[:2].contiguous(), sm[:2].contiguous(), None, None, None))
    with pytest.raises(T.TcrError, match="is not a push of 3 streams"):
        sp.push(St.StreamOutput(None, sm, sm, None, None, None))          # one step is [S, classes]
    flat = sm.reshape(15, 12)
    with pytest.raises(T.TcrError, match="is not a push of 3 streams"):
        sp.push(Sc.RaggedScanOutput(None, flat, flat, None, None, None, np.array([0, 7, 15], np.int64)))
    with pytest.raises(T.TcrError, match="expected a contiguous float32 tensor"):
        sp.push(Sc.ScanOutput(None, sm.double(), sm.double(), None, None, None))
    if dev.type == "cpu":                                    # (the emulator's "device" is the host: a meta tensor is somewhere else)
        with pytest.raises(T.TcrError, match="expected a contiguous float32 tensor on cpu"):
            sp.push(Sc.ScanOutput(None, sm.to("meta"), sm.to("meta"), None, None, None))
    with pytest.raises(T.TcrError, match="reset mask must have 3 entries"):
        sp.reset(np.zeros(4, bool))
    with pytest.raises(T.TcrError, match="stream index outside 0..2"):
        sp.reset([3])
    # a reset stays pending for a stream without rows in a ragged push, as StreamingDetector.push_ragged keeps it
    sp.reset([0, 2])
    rag = Sc.RaggedScanOutput(None, flat, flat, None, None, None, np.array([0, 7, 7, 15], np.int64))
    first = sp.push(rag)
    assert sp._pending is None and first.top.shape == (15,)
    sp.reset(np.array([0, 1, 0], np.uint8))
    sp.push(rag)
    assert sp._pending is not None and sp._pending.tolist() == [False, True, False]
    again = sp.push(Sc.RaggedScanOutput(None, flat, flat, None, None, None, np.array([0, 5, 10, 15], np.int64)))
    assert sp._pending is None
    fresh = ph.detect(Sc.RaggedScanOutput(None, flat, flat, None, None, None, np.array([0, 5, 10, 15], np.int64)))
    assert torch.equal(again.probs[5:10], fresh.probs[5:10]) and not torch.equal(again.probs[:5], fresh.probs[:5])
    empty = sp.push(Sc.RaggedScanOutput(None, flat[:0], flat[:0], None, None, None, np.zeros(4, np.int64)))
    assert empty.top.shape == (0,) and empty.probs.shape == (0, 3)


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------------
def check_cli(lib, tmp_path, capsys, monkeypatch):
    """stream_audio.py --phrases prints scan_audio.py --phrases' lines on files of equal length; without the flag its lines are the
    `StreamingDetector`'s own."""
    from tcresnet_amd import scan_audio, stream_audio
    path, wavs = cli_case(lib, tmp_path, 61, lengths=(19200, 19200))
    FrozenModel = in_process(monkeypatch, lib)
    sc, rec, out, (a, b) = top_words(FrozenModel.load(path), wavs)
    labels = [f"c{i}" for i in range(12)]
    flags = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), "--frames_per_step", "2", "--average_window_ms", "200", "--min_count",
             "2", "--detection_threshold", "0.3", "--suppression_ms", "400"]
    for extra in (["--phrases", f"c{a} c{b};c{b} c{a};c{a}", "--phrase_window_ms", "240"],
                  ["--phrases", f"c{a} c{b};c{b} c{a}", "--phrase_window_ms", "200", "--phrase_unordered", "--phrase_combine", "min"]):
        capsys.readouterr()
        assert scan_audio.main(scan_audio.parse_arguments([*flags, *extra])) == 0
        want = capsys.readouterr().out.splitlines()
        assert stream_audio.main(stream_audio.parse_arguments([*flags, *extra])) == 0
        got = capsys.readouterr().out.splitlines()
        assert got == want and len(want) >= 2
    # without the flag: the keyword detections, as before
    assert stream_audio.main(stream_audio.parse_arguments(flags)) == 0
    plain = capsys.readouterr().out.splitlines()
    det = FrozenModel.load(path).streaming(2, frames_per_step=2, average_window_ms=200, min_count=2, detection_threshold=0.3, suppression_ms=400)
    x = next(iter(rec.chunks(None)))[1]
    many = det.push_many(x)
    new, top, score = many.is_new.cpu().numpy(), many.top.cpu().numpy(), many.score.cpu().numpy()
    lines = [f"{wavs[s]},{stream_audio.format_time_ms(1000.0 * (i + 1) * 640 / 16000)},{labels[top[s, i]]},{float(score[s, i]):.6f}"
             for i in range(new.shape[1]) for s in range(2) if new[s, i]]
    assert plain == lines and len(lines) >= 1
    assert stream_audio.parse_arguments(flags).phrases is None


def test_stream_audio_phrases_cli(emu_lib, tmp_path, capsys, monkeypatch):
    check_cli(emu_lib, tmp_path, capsys, monkeypatch)


# ---- MI355X -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", [7, 256])
def test_gpu_any_split_equals_the_whole(hip_lib, w):
    check_split(hip_lib, 12, w)


@pytest.mark.gpu
@pytest.mark.parametrize("S,w", [(65, 2), (65, 7), (1, 2), (1, 7)])
def test_gpu_many_single_row_pushes(hip_lib, S, w):
    check_single_rows(hip_lib, S, w)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [2, 7, 300])
def test_gpu_ragged_pushes(hip_lib, w):
    check_ragged(hip_lib, w)


@pytest.mark.gpu
def test_gpu_reset_restarts_marked_streams_only(hip_lib):
    check_reset(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_gpu_real_streams_equal_the_scan(hip_lib, k):
    check_real_streams(hip_lib, k)


@pytest.mark.gpu
def test_gpu_stream_audio_phrases_cli(hip_lib, tmp_path, capsys, monkeypatch):
    check_cli(hip_lib, tmp_path, capsys, monkeypatch)
