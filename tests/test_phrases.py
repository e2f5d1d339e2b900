"""Phrase detection (tcr_phrase_scores, tcresnet_amd.scanning.PhraseDetector): the phrase posteriors are bitwise the NumPy definition
(tests/phrase_ref.py) for every window, combiner and order, dense and ragged; the detector, sweep, grid and mining stages run on them
with P + 1 classes.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`).  Every comparison is bitwise."""
import csv
import ctypes as C
import io
import itertools
import os

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests import phrase_ref as PR
from tests.test_scan import scanning
from tests.test_streaming import frozen_artifact, segment_audio, setup, write_wav

TILE = T._lib.PHRASE_TILE
PRODUCT, MIN = T._lib.PHRASE_PRODUCT, T._lib.PHRASE_MIN
MODES = list(itertools.product((1, 0), (PRODUCT, MIN)))         # (ordered, combine)
WINDOWS = (1, 2, 7, 255, 256, 300)


def w_max(U):
    """include/tcresnet_hip.h: tcr_phrase_window_max."""
    return 16384 // U - (TILE - 1) if U >= 1 else 0


def phrases_for(ncls):
    """One word, a pair and its reverse, a repeated word, three words, eight words."""
    long = [0, 1, 2, 0, 1, 2, 1, 1] if ncls == 3 else [2, 3, 4, 5, 6, 7, 8, 9]
    return [[1], [1, 2], [2, 1], [1, 1], [0, 1, 2], long]


def planted_rows(rng, steps, ncls):
    """Smoothed softmax rows [steps, ncls] with planted runs of the phrases' words: a run of 2 .. 6 steps of one class every 0 .. 5
    steps, then softmax and a causal mean over three rows (float32), so that every window of seven steps sees several words in
    some order; a signal of more than a tile also says "1 2" across the tile boundary."""
    x = (rng.randn(steps, ncls) * 0.5).astype(np.float32)
    pos = 0
    while pos < steps:
        m = int(rng.randint(2, 7))
        x[pos:pos + m, rng.randint(min(ncls, 4))] += rng.uniform(2.0, 4.0)
        pos += m + int(rng.randint(0, 6))
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    sm = p.copy()
    for d in (1, 2):
        sm[d:] = sm[d:] + p[:-d]
    sm[2:] = sm[2:] * np.float32(1.0 / 3.0)
    if steps > 1:
        sm[1] = sm[1] * np.float32(0.5)
    sm = np.clip(sm, 0, 1).astype(np.float32)
    if steps > TILE + 8:                                # "1 2" across the first tile boundary: word 1 ends the tile, word 2 starts the next
        for a, c in ((TILE - 3, 1), (TILE + 1, 2)):
            sm[a:a + 2] = np.float32(0.1 / (ncls - 1))
            sm[a:a + 2, c] = np.float32(0.9)
    return sm


def table(phrases):
    off = np.zeros(len(phrases) + 1, np.int32)
    np.cumsum([len(q) for q in phrases], out=off[1:])
    return off, np.array([c for q in phrases for c in q] or [0], np.int32)


def lib_scores(lib, values, phrases, w, ordered, combine, offsets=None, off_words=None, check=True):
    """tcr_phrase_scores(_ragged) on host arrays -> (status, out as NumPy; out starts as -7 everywhere)."""
    dev = Cm.device_of(lib)
    v = torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(dev)
    off, words = table(phrases) if off_words is None else off_words
    P = len(off) - 1
    out = torch.full((*v.shape[:-1], max(P, 0) + 1), -7.0, device=dev)
    cfg = T._lib.PhraseCfg(w, ordered, combine)
    if offsets is None:
        rc = lib.tcr_phrase_scores(v.shape[0], v.shape[1], v.shape[2], v.data_ptr(), P, off.ctypes.data, words.ctypes.data, C.byref(cfg),
                                   out.data_ptr(), None)
    else:
        so = torch.from_numpy(np.asarray(offsets, np.int64)).to(dev)
        rc = lib.tcr_phrase_scores_ragged(len(offsets) - 1, so.data_ptr(), v.shape[0], v.shape[1], v.data_ptr(), P, off.ctypes.data,
                                          words.ctypes.data, C.byref(cfg), out.data_ptr(), None)
    if check:
        lib.check(rc, "tcr_phrase_scores")
    return rc, out.cpu().numpy()


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


def ragged_lengths(w):
    return [0, 1, 2, max(w - 1, 0), w, w + 1, 256, 257, 517]


def check_table(lib, ncls, w, lengths, dense=(3, 261), seed=0):
    """The library against the reference for every mode, ragged over `lengths` and dense."""
    rng = np.random.RandomState(1000 * ncls + w + seed)
    phrases = phrases_for(ncls)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    packed = np.concatenate([planted_rows(rng, m, ncls) for m in lengths if m > 0])
    N, steps = dense
    cube = np.stack([planted_rows(rng, steps, ncls) for _ in range(N)])
    doff = np.arange(N + 1, dtype=np.int64) * steps
    wants = {}
    for ordered, combine in MODES:
        want = PR.scores(packed, off, phrases, w, ordered, combine)
        same(lib_scores(lib, packed, phrases, w, ordered, combine, offsets=off)[1], want, ("ragged", ncls, w, ordered, combine))
        dwant = PR.scores(cube.reshape(N * steps, ncls), doff, phrases, w, ordered, combine)
        same(lib_scores(lib, cube, phrases, w, ordered, combine)[1].reshape(N * steps, -1), dwant, ("dense", ncls, w, ordered, combine))
        wants[ordered, combine] = want
    return packed, off, phrases, wants


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_reference_dp_equals_brute_force():
    """Guards the reference: the DP, its vectorised form and the maximum over all chains are the same bits on a 40-step case."""
    rng = np.random.RandomState(5)
    v = planted_rows(rng, 40, 5)
    pairs, triples = [[1, 2], [2, 1], [1, 1], [3]], [[0, 1, 2], [1, 1, 2]]
    for ordered, combine in MODES:
        for w, phrases in ((1, pairs + triples), (2, pairs + triples), (7, pairs + triples), (12, pairs + triples), (40, pairs)):
            brute = PR.scores_signal(v, phrases, w, ordered, combine, conf=PR.conf_brute)
            same(PR.scores_signal(v, phrases, w, ordered, combine), brute, ("dp", w, ordered, combine))
            same(PR.scores_dp_fast(v, phrases, w, bool(ordered), combine), brute, ("fast dp", w, ordered, combine))
    assert brute[:, -1].tobytes() == (np.float32(1.0) - brute[:, :-1].max(axis=1)).tobytes()


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("ncls", [3, 12])
def test_scores_equal_definition(emu_lib, ncls, w):
    check_table(emu_lib, ncls, w, ragged_lengths(w))


# ---- 2. the inputs discriminate (on the reference) --------------------------------------------------------------------------------------
def test_inputs_discriminate():
    ncls, w = 12, 7
    rng = np.random.RandomState(1000 * ncls + w)
    lengths = ragged_lengths(w)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    packed = np.concatenate([planted_rows(rng, m, ncls) for m in lengths if m > 0])     # check_table's ragged input at (12, 7)
    phrases = phrases_for(ncls)
    ref = {(o, c, ww): PR.scores(packed, off, phrases, ww, o, c) for o, c in MODES for ww in (w, w + 1)}
    P = len(phrases)
    differ = lambda a, b: int((a.view(np.uint32) != b.view(np.uint32))[:, :P].any(axis=1).sum())
    assert differ(ref[1, PRODUCT, w], ref[0, PRODUCT, w]) >= 15          # ordered != unordered
    assert differ(ref[1, PRODUCT, w], ref[1, MIN, w]) >= 15              # product != min
    assert differ(ref[1, PRODUCT, w], ref[1, PRODUCT, w + 1]) >= 15      # w != w + 1
    assert differ(ref[1, MIN, w], ref[1, MIN, w + 1]) >= 15
    pair = ref[1, PRODUCT, w][:, 1], ref[1, PRODUCT, w][:, 2]            # [1, 2] against [2, 1]
    assert (pair[0] != pair[1]).sum() >= 15
    # a best chain that starts in the tile in front of its step's own tile (the 517-step signal: steps 256 .. 256 + w - 2)
    sig = packed[off[-2]:off[-1]]
    crossing = 0
    for i in range(TILE, TILE + w - 1):
        for q, words in enumerate(phrases[1:5], start=1):
            conf, chain = PR.conf_brute(sig, words, w, True, PRODUCT, i)
            assert conf.tobytes() == ref[1, PRODUCT, w][off[-2] + i, q].tobytes()
            crossing += chain[0] < TILE <= chain[-1]
    assert crossing >= 1


# ---- 3. ragged isolation ----------------------------------------------------------------------------------------------------------------
def test_ragged_signal_never_reads_its_predecessor(emu_lib):
    ncls, w = 12, 40
    rng = np.random.RandomState(9)
    lens = [TILE + 30, TILE + 5]
    first, second = planted_rows(rng, lens[0], ncls), planted_rows(rng, lens[1], ncls)
    first[-w:] = np.float32(0.02)
    first[-w:, 1] = np.float32(0.97)                     # the predecessor ends in a run of word 1
    second[:5] = np.float32(0.02)
    second[:5, 2] = np.float32(0.95)                     # and the signal starts with word 2: "1 2" if the rows were one signal's
    packed, off = np.concatenate([first, second]), [0, lens[0], sum(lens)]
    phrases = phrases_for(ncls)
    for ordered, combine in MODES:
        got = lib_scores(emu_lib, packed, phrases, w, ordered, combine, offsets=off)[1]
        alone = lib_scores(emu_lib, second[None], phrases, w, ordered, combine)[1][0]
        same(got[lens[0]:], alone, (ordered, combine))
        joined = PR.scores(packed, [0, sum(lens)], phrases, w, ordered, combine)       # (what reading the predecessor would give)
        assert joined[lens[0]:lens[0] + 5].tobytes() != alone[:5].tobytes()


# ---- 4. the detector over phrase posteriors ---------------------------------------------------------------------------------------------
NAMES = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(2, 12)]
DET = dict(average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=200)


def word_rows(steps, runs, ncls=12, high=0.9):
    """Posteriors [steps, ncls]: `high` on class 0 except in `runs` (first, last, class), where it is on that class."""
    v = np.full((steps, ncls), (1.0 - high) / (ncls - 1), np.float32)
    v[:, 0] = high
    for a, b, c in runs:
        v[a:b + 1] = (1.0 - high) / (ncls - 1)
        v[a:b + 1, c] = high
    return v


def phrase_case(lib, **kw):
    """A scanner, a phrase detector over "w2 w3" and "w3 w2" and a dense `ScanOutput` of two planted signals (no audio behind it):
    signal 0 says "w2 w3", pauses, and says it again; signal 1 says "w3 w2" once and "w2 w3" once."""
    Sc = scanning()
    fe, net, _, _, _ = setup(lib)
    scanner = Sc.KeywordScanner(net, fe, **DET)
    steps = 140
    sig = [word_rows(steps, [(10, 14, 2), (18, 22, 3), (70, 74, 2), (78, 82, 3)]),
           word_rows(steps, [(20, 24, 3), (27, 31, 2), (90, 94, 2), (99, 103, 3)])]
    sm = torch.from_numpy(np.stack(sig)).to(Cm.device_of(lib))
    out = Sc.ScanOutput(None, sm, sm, None, None, None)
    ph = Sc.PhraseDetector(scanner, {"two three": ["w2", "w3"], "three two": ["w3", "w2"]}, window_ms=300, detection_threshold=0.5,
                           suppression_ms=100, labels=NAMES, **kw)
    return Sc, scanner, ph, out, np.stack(sig)


def fired(top, new):
    return [int(c) for c in top[new != 0]]


def test_detect_equals_rule_and_refires_after_background(emu_lib):
    Sc, scanner, ph, out, sig = phrase_case(emu_lib)
    assert ph.labels == ["two three", "three two", "_background_"] and ph.num_classes == 3
    assert ph.window_steps == 15 and ph.det.suppression_steps == 5 and ph.det.average_steps == ph.det.min_count == 1
    det = ph.detect(out)
    assert isinstance(det, Sc.ScanOutput) and det.logits is None and det.smoothed is det.probs
    same(ph.scores(out).cpu().numpy(), det.probs.cpu().numpy())
    for n in range(2):
        post = PR.scores(sig[n], [0, sig.shape[1]], ph.words, 15, 1, PRODUCT)
        same(det.probs[n].cpu().numpy(), post, "posteriors")
        top, score, new = PR.detect_rule(post, 5, 0.5)
        if n == 0:                                        # the phrase, the background, the phrase again: on the reference first
            seq = fired(top, new)
            assert any(seq[j:j + 3] == [0, 2, 0] for j in range(len(seq)))
        assert det.top[n].cpu().numpy().tobytes() == top.tobytes()
        assert det.score[n].cpu().numpy().tobytes() == score.tobytes()
        assert det.is_new[n].cpu().numpy().tobytes() == new.tobytes()
    seq = fired(det.top[0].cpu().numpy(), det.is_new[0].cpu().numpy())
    assert any(seq[j:j + 3] == [0, 2, 0] for j in range(len(seq)))
    assert 1 in fired(det.top[1].cpu().numpy(), det.is_new[1].cpu().numpy())
    # unordered: "two three" and "three two" score the same, ordered they do not
    un = Sc.PhraseDetector(scanner, [["w2", "w3"], ["w3", "w2"]], window_ms=300, ordered=False, labels=NAMES).scores(out).cpu().numpy()
    assert un[..., 0].tobytes() == un[..., 1].tobytes() and det.probs[..., 0].cpu().numpy().tobytes() != det.probs[..., 1].cpu().numpy().tobytes()
    # the ragged form of the same rows
    flat = out.smoothed.reshape(-1, 12)
    rout = Sc.RaggedScanOutput(None, flat, flat, None, None, None, np.array([0, 140, 280], np.int64))
    rdet = ph.detect(rout)
    assert isinstance(rdet, Sc.RaggedScanOutput) and np.array_equal(rdet.offsets, rout.offsets)
    for f in ("probs", "top", "score", "is_new"):
        assert torch.equal(getattr(rdet, f), getattr(det, f).reshape(280, *getattr(det, f).shape[2:])), f
    # and of a cascade's output: the same kind again, with the cascade's own fields
    cout = Sc.CascadeOutput(None, flat, flat, None, None, None, rout.offsets, torch.zeros(0, dtype=torch.int64), rout)
    cdet = ph.detect(cout)
    assert isinstance(cdet, Sc.CascadeOutput) and cdet.selected is cout.selected and cdet.first is rout
    assert torch.equal(cdet.top, rdet.top) and torch.equal(cdet.is_new, rdet.is_new) and torch.equal(cdet.probs, rdet.probs)


# ---- 5. the keyword stages, reused ------------------------------------------------------------------------------------------------------
def test_sweep_tune_and_mine_reuse_the_keyword_stages(emu_lib):
    Sc, scanner, ph, out, sig = phrase_case(emu_lib)
    det = ph.detect(out)
    thr = [0.1, 0.5, 0.7, 0.9]
    step_ms = scanner.step_ms
    # signal 0: an event over the first "two three" only (the second is the planted false accept); signal 1: both phrases labelled
    events = [[(18 * step_ms, 40 * step_ms, "two three")], [(27 * step_ms, 50 * step_ms, "three two"), (99 * step_ms, 120 * step_ms, 0)]]
    res = ph.sweep(out, thr, events=events, tolerance_ms=0.0)
    assert isinstance(res, Sc.PhraseSweepResult)
    ev_steps = ph.stage.event_steps(det, events, None, 0.0, ph.labels)[2]
    raw = Sc.detection_sweep(det.top, det.score, thr, ph.det.suppression_steps, 3, ev_steps, None, scanner.step_samples / 16000.0, lib=emu_lib)
    for f in ("detections", "hits", "duplicates"):
        assert torch.equal(getattr(res, f), getattr(raw, f)), f
    assert torch.equal(ph.sweep(det, thr, events=events, tolerance_ms=0.0).detections, res.detections)      # (a detected output is taken as is)
    cv, no_bg, with_bg = res.curve(), raw.curve([0, 1]), raw.curve()
    for key in cv:
        assert np.array_equal(cv[key], no_bg[key], equal_nan=True), key
    assert (with_bg["false_accepts"] > cv["false_accepts"]).all() and cv["hits"][1] == 3 and cv["false_accepts"][1] == 1
    assert res.operating_point(1e9) == raw.operating_point(1e9, [0, 1])
    # tune over two suppression values == two sweeps
    grid = ph.tune(out, thr, suppression_ms=(100, 1200), events=events, tolerance_ms=0.0)
    assert isinstance(grid, Sc.PhraseGridResult) and len(grid) == 2
    for j, ms in enumerate((100, 1200)):
        one = Sc.PhraseDetector(scanner, dict(zip(ph.names, ph.words)), window_ms=300, detection_threshold=0.5, suppression_ms=ms)
        want = one.sweep(out, thr, events=events, tolerance_ms=0.0)
        for f in ("detections", "hits", "duplicates"):
            assert torch.equal(getattr(grid.result(j), f), getattr(want, f)), (f, ms)
        assert isinstance(grid.result(j), Sc.PhraseSweepResult)
    assert not torch.equal(grid.detections[0], grid.detections[1])
    best = grid.best(1e9)
    assert best is not None and best["events"] == 3                      # (the phrases' events: the background has none and is not scored)
    # mine: the planted false accept, with the audio of its step
    audio = torch.from_numpy(segment_audio(2, 140 * scanner.step_samples, 3)).to(Cm.device_of(emu_lib))
    mined = ph.mine(out, audio, events=events, k=10, tolerance_ms=0.0)
    top0, _, new0 = PR.detect_rule(det.probs[0].cpu().numpy(), 5, 0.5)
    second = [s for s in np.flatnonzero(new0) if top0[s] == 0][1]
    assert len(mined) == 1 and mined.kind_names() == ["false_accept"]
    assert (int(mined.signal[0]), int(mined.step[0]), int(mined.label[0])) == (0, int(second), 0)
    end = (int(second) + 1) * scanner.step_samples
    assert torch.equal(mined.clips[0], audio[0, end - 16000:end])


# ---- 6. from a real scan ----------------------------------------------------------------------------------------------------------------
def check_real_scan(lib, k=1):
    Sc = scanning()
    fe, net, _, _, _ = setup(lib)
    scanner = Sc.KeywordScanner(net, fe, frames_per_step=k, **DET)
    step = scanner.step_samples
    audio = Cm.to_dev(lib, segment_audio(2, 30 * step, 41))
    sig = [audio[n % 2, :m * step].contiguous() for n, m in enumerate([22, 0, 3, 30])]
    out = scanner.scan_ragged(sig)
    sm = out.smoothed.cpu().numpy()
    order = np.argsort(-sm.mean(axis=0))                  # the random net's most likely classes are the words
    words = [[int(order[0]), int(order[1])], [int(order[1]), int(order[0])], [int(order[0]), int(order[0]), int(order[2])]]
    for combine, ordered in (("product", True), ("min", False)):
        ph = Sc.PhraseDetector(scanner, words, window_ms=8 * scanner.step_ms, ordered=ordered, combine=combine)
        assert ph.window_steps == 8 and ph.labels[0] == f"{order[0]} {order[1]}"
        got = ph.scores(out)
        assert got.shape == (55, 4)
        want = PR.scores(sm, out.offsets, words, 8, int(ph.ordered), T._lib.PHRASE_PRODUCT if ph.combine == "product" else T._lib.PHRASE_MIN)
        same(got.cpu().numpy(), want, (combine, ordered))
        if ordered:
            assert int((want[:, 0] != want[:, 1]).sum()) > 0             # "a b" is not "b a" on this scan
        same(ph.scores(out, on="probs").cpu().numpy(), PR.scores(out.probs.cpu().numpy(), out.offsets, words, 8, int(ph.ordered),
                                                                 PRODUCT if ph.combine == "product" else MIN))
    det = ph.detect(out)
    assert isinstance(det, Sc.RaggedScanOutput) and det.top.shape == (55,)
    dense = scanner.scan(audio)
    same(ph.scores(dense).cpu().numpy().reshape(60, 4),
         PR.scores(dense.smoothed.cpu().numpy().reshape(60, -1), [0, 30, 60], words, 8, int(ph.ordered), MIN))
    return scanner, out


def test_scores_of_a_real_scan(emu_lib):
    check_real_scan(emu_lib)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_c_refusals_write_nothing(emu_lib):
    lib = emu_lib
    v = planted_rows(np.random.RandomState(2), 50, 4)[None]
    ok = [[1, 2], [3]]

    def refused(msg, values=v, phrases=ok, w=5, ordered=1, combine=PRODUCT, offsets=None, off_words=None):
        rc, out = lib_scores(lib, values, phrases, w, ordered, combine, offsets=offsets, off_words=off_words, check=False)
        assert rc == -1 and msg in lib.tcr_last_error().decode(), (msg, rc, lib.tcr_last_error())
        assert (out == -7.0).all()

    assert lib_scores(lib, v, ok, 5, 1, PRODUCT)[0] == 0
    refused("n_phrases 0 outside 1..64", phrases=[])
    refused("n_phrases 65 outside 1..64", phrases=[[1]] * 65)
    refused("phrase 1 has 0 words (1..8)", phrases=[[1], []])
    refused("phrase 0 has 9 words (1..8)", phrases=[[1] * 9])
    refused("phrase 1 word 0: class 4 outside 0..3", phrases=[[1, 2], [4]])
    refused("phrase 0 word 1: class -1 outside 0..3", phrases=[[1, -1]])
    refused("phrase_offsets must start at 0", off_words=(np.array([1, 2, 3], np.int32), np.array([1, 2, 3], np.int32)))
    refused("phrase_offsets decrease at phrase 1", off_words=(np.array([0, 2, 1], np.int32), np.array([1, 2, 3], np.int32)))
    refused("window_steps must be >= 1 (got 0)", w=0)
    wm = lib.tcr_phrase_window_max(3)
    assert wm == w_max(3) == 5206 and lib.tcr_phrase_window_max(64) == 1 and lib.tcr_phrase_window_max(65) < 1 and lib.tcr_phrase_window_max(0) < 1
    refused(f"window_steps {wm + 1} above tcr_phrase_window_max(3 distinct word classes) = {wm}", w=wm + 1)
    assert lib_scores(lib, v, ok, wm, 1, PRODUCT)[0] == 0                 # (the limit itself is taken)
    many = planted_rows(np.random.RandomState(3), 20, 70)[None]
    refused("above tcr_phrase_window_max(65 distinct word classes)", values=many, phrases=[list(range(8 * q, 8 * q + 8)) for q in range(8)] + [[64]],
            w=1)
    refused("ordered must be 0 or 1 (got 2)", ordered=2)
    refused("unknown combine 2", combine=2)
    # null pointers and sizes past 2^31, on the raw entries (nothing is dereferenced before the checks)
    off, words = table(ok)
    cfg = T._lib.PhraseCfg(5, 1, PRODUCT)
    dev = Cm.device_of(lib)
    x, out = torch.from_numpy(v).to(dev), torch.full((1, 50, 3), -7.0, device=dev)
    so = torch.zeros(2, dtype=torch.int64, device=dev)
    args = [x.data_ptr(), 2, off.ctypes.data, words.ctypes.data, C.byref(cfg), out.data_ptr()]
    for hole in (0, 2, 3, 4, 5):
        a = list(args)
        a[hole] = None
        assert lib.tcr_phrase_scores(1, 50, 4, *a, None) == -1 and "tcr_phrase_scores: null argument" in lib.tcr_last_error().decode()
        assert lib.tcr_phrase_scores_ragged(1, so.data_ptr(), 50, 4, *a, None) == -1
    assert lib.tcr_phrase_scores_ragged(1, None, 50, 4, *args, None) == -1 and "tcr_phrase_scores_ragged: null argument" in lib.tcr_last_error().decode()
    for msg, shape in (("the number of steps must be positive (got 0)", (1, 0, 4)), ("the number of signals must be positive (got 0)", (0, 50, 4)),
                       ("num_classes must be positive (got 0)", (1, 50, 0)), ("the number of steps must be positive (got -3)", (1, -3, 4))):
        assert lib.tcr_phrase_scores(*shape, *args, None) == -1 and msg in lib.tcr_last_error().decode(), msg
    assert lib.tcr_phrase_scores_ragged(1, so.data_ptr(), 0, 4, *args, None) == -1 and "the number of steps must be positive (got 0)" in \
        lib.tcr_last_error().decode()
    assert lib.tcr_phrase_scores_ragged(0, so.data_ptr(), 50, 4, *args, None) == -1 and "the number of signals" in lib.tcr_last_error().decode()
    assert lib.tcr_phrase_scores(1, (1 << 31) // 4, 4, *args, None) == -1 and "is too large" in lib.tcr_last_error().decode()
    assert lib.tcr_phrase_scores(2, 1 << 30, 4, *args, None) == -1 and "is too large" in lib.tcr_last_error().decode()
    off4, words4 = table([[0], [1], [0, 1], [1, 0]])                      # P + 1 = 5 columns out of C = 2: the output is the wider array
    args4 = [x.data_ptr(), 4, off4.ctypes.data, words4.ctypes.data, C.byref(cfg), out.data_ptr()]
    rows = (1 << 31) // 5 + 1
    assert lib.tcr_phrase_scores_ragged(1, so.data_ptr(), rows, 2, *args4, None) == -1
    assert f"{rows} steps in all x 5 columns is too large" in lib.tcr_last_error().decode()
    assert (out == -7.0).all()


def test_python_refusals(emu_lib):
    Sc, scanner, ph, out, _ = phrase_case(emu_lib)
    mk = lambda phrases, **kw: Sc.PhraseDetector(scanner, phrases, labels=NAMES, **kw)
    with pytest.raises(T.TcrError, match="unknown word 'w99'"):
        mk([["w2", "w99"]])
    with pytest.raises(T.TcrError, match="unknown word 12"):
        mk([[2, 12]])
    with pytest.raises(T.TcrError, match="unknown word 'w2'"):
        Sc.PhraseDetector(scanner, [["w2"]])               # (no labels: names mean nothing)
    with pytest.raises(T.TcrError, match="phrase 'nothing' is empty"):
        mk({"nothing": []})
    with pytest.raises(T.TcrError, match="duplicate phrase name 'w2 w3'"):
        mk([["w2", "w3"], [2, 3], ["w2", "w3"]][::2])
    with pytest.raises(T.TcrError, match="duplicate phrase name '_background_'"):
        mk({"_background_": [2]})
    with pytest.raises(T.TcrError, match=r"65 phrases \(1..64\)"):
        mk({f"p{q}": [2] for q in range(65)})
    with pytest.raises(T.TcrError, match=r"0 phrases \(1..64\)"):
        mk([])
    with pytest.raises(T.TcrError, match=r"has 9 words \(1..8\)"):
        mk([[2] * 9])
    with pytest.raises(T.TcrError, match="combine must be one of"):
        mk([[2]], combine="sum")
    with pytest.raises(T.TcrError, match=f"above the {w_max(2)} that tcr_phrase_window_max allows for 2 distinct words"):
        mk([[2, 3]], window_ms=20 * (w_max(2) + 1))
    assert mk([[2, 3]], window_ms=20 * w_max(2)).window_steps == w_max(2) == 7937
    wrong = Sc.ScanOutput(None, out.probs[..., :5].contiguous(), out.smoothed[..., :5].contiguous(), None, None, None)
    for call in (ph.scores, ph.detect, lambda o: ph.sweep(o, [0.5])):
        with pytest.raises(T.TcrError, match="is not a scan of the scanner's 12 classes"):
            call(wrong)
    with pytest.raises(T.TcrError, match="on must be 'smoothed' or 'probs'"):
        ph.scores(out, on="logits")
    with pytest.raises(T.TcrError, match="unknown label 'w2'"):
        ph.sweep(out, [0.5], events=[[(0.0, 100.0, "w2")], []])            # events are labelled by phrase
    assert mk([["w2", "w3"], "w3 w2"]).names == ["w2 w3", "w3 w2"] and mk({"a": [2, "w3"]}).words == [[2, 3]]


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------------
def cli_case(lib, tmp_path, seed, lengths=(20000, 12800)):
    fe, net, _, _, _ = setup(lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    audio = segment_audio(len(lengths), max(lengths), seed)
    wavs = []
    for n, m in enumerate(lengths):
        wavs.append(str(tmp_path / f"p{n}.wav"))
        write_wav(wavs[-1], np.clip(audio[n, :m] * 32767, -32768, 32767).astype(np.int16))
    return path, wavs


def in_process(monkeypatch, lib):
    """The tools load their artifact onto `lib` (the emulator has no default device)."""
    from tcresnet_amd.deploy import FrozenModel
    load = FrozenModel.load.__func__
    monkeypatch.setattr(FrozenModel, "load", classmethod(lambda cls, p, lib_=None, device=None: load(cls, p, lib=lib, device=Cm.device_of(lib))))
    return FrozenModel


def top_words(model, wavs, k=2):
    """The classes a scan of the files puts on top most often: the words of the tests' phrases."""
    from tcresnet_amd.audio_input import Recordings
    sc = model.scanner(frames_per_step=k, average_window_ms=200, min_count=2, detection_threshold=0.3, suppression_ms=400)
    rec = Recordings(wavs, sc)
    out = sc.scan_ragged(rec.packed())
    order = np.argsort(-out.smoothed.cpu().numpy().mean(axis=0))
    return sc, rec, out, [int(order[0]), int(order[1])]


def test_scan_audio_phrases_cli(emu_lib, tmp_path, capsys, monkeypatch):
    from tcresnet_amd import scan_audio
    Sc = scanning()
    path, wavs = cli_case(emu_lib, tmp_path, 61)
    FrozenModel = in_process(monkeypatch, emu_lib)
    sc, rec, out, (a, b) = top_words(FrozenModel.load(path), wavs)
    labels = [f"c{i}" for i in range(12)]
    spec = f"c{a} c{b};c{b} c{a};c{a}"
    flags = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), "--frames_per_step", "2", "--average_window_ms", "200", "--min_count",
             "2", "--detection_threshold", "0.3", "--suppression_ms", "400", "--phrase_window_ms", "240"]
    capsys.readouterr()
    assert scan_audio.main(scan_audio.parse_arguments([*flags, "--ragged", "--summary", "--phrases", spec])) == 0
    cap = capsys.readouterr()
    ph = Sc.PhraseDetector(sc, [[a, b], [b, a], [a]], window_ms=240)
    assert ph.window_steps == 6 and ph.det.suppression_steps == 10 and abs(ph.det.threshold - 0.3) < 1e-6
    det = ph.detect(out)
    names = [f"c{a} c{b}", f"c{b} c{a}", f"c{a}", "_background_"]
    top, score, new = det.top.cpu().numpy(), det.score.cpu().numpy(), det.is_new.cpu().numpy()
    want = []
    for p in np.flatnonzero(new):
        n = int(np.searchsorted(out.offsets, p, side="right") - 1)
        i = int(p - out.offsets[n])
        want.append((i, n, f"{wavs[n]},{round(1000.0 * (i + 1) * 640 / 16000, 3):g},{names[top[p]]},{float(score[p]):.6f}"))
    assert cap.out.splitlines() == [line for _, _, line in sorted(want)] and len(want) >= 2
    assert '"detections": %d' % len(want) in cap.err
    # the padded one-call run, the phrases from a file, the other combiner and order
    (tmp_path / "phrases.txt").write_text(spec.replace(";", "\n") + "\n\n")
    assert scan_audio.main(scan_audio.parse_arguments([*flags, "--phrases", "@" + str(tmp_path / "phrases.txt"), "--phrase_combine", "min",
                                                       "--phrase_unordered"])) == 0
    dense_lines = capsys.readouterr().out.splitlines()
    dense = Sc.PhraseDetector(sc, [[a, b], [b, a], [a]], window_ms=240, ordered=False, combine="min")
    x = next(iter(rec.chunks(None)))[1]
    d = dense.detect(sc.scan(x))
    assert len(dense_lines) == int(d.is_new.sum()) >= 2 and all(line.split(",")[2] in names for line in dense_lines)
    for extra in (["--chunk_seconds", "1"], ["--ragged_chunk_seconds", "1"]):
        with pytest.raises(SystemExit, match="--phrases scores whole scans"):
            scan_audio.main(scan_audio.parse_arguments([*flags, "--phrases", spec, *extra]))
    with pytest.raises(T.TcrError, match="unknown word 'nope'"):
        scan_audio.main(scan_audio.parse_arguments([*flags, "--phrases", "c1 nope"]))


# ---- MI355X -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", [7, 256])
def test_gpu_scores_equal_definition(hip_lib, w):
    check_table(hip_lib, 12, w, [0, 1, w, 256, 257, 517])


@pytest.mark.gpu
def test_gpu_scores_of_a_real_scan(hip_lib):
    check_real_scan(hip_lib)


@pytest.mark.gpu
def test_gpu_sweep_audio_phrases_cli(hip_lib, tmp_path, capsys):
    from tcresnet_amd import sweep_audio
    from tcresnet_amd.deploy import FrozenModel
    Sc = scanning()
    path, wavs = cli_case(hip_lib, tmp_path, 62, lengths=(64000, 40000))
    sc, rec, out, (a, b) = top_words(FrozenModel.load(path), wavs)
    labels = [f"c{i}" for i in range(12)]
    names = [f"c{a} c{b}", f"c{b} c{a}"]
    rows = [(wavs[0], 500, 1500, names[0]), (wavs[0], 2500, 3200, names[1]), (wavs[1], 800, 1800, names[0])]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{s},{e},{c}\n" for f, s, e, c in rows))
    flags = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), "--frames_per_step", "2", "--average_window_ms", "200", "--min_count",
             "2", "--suppression_ms", "400", "--events", str(ev_csv), "--thresholds", "0:0.9:0.1", "--tolerance_ms", "300", "--phrases",
             ";".join(names), "--phrase_window_ms", "2000", "--phrase_combine", "min", "--ragged"]
    capsys.readouterr()
    assert sweep_audio.main(sweep_audio.parse_arguments(flags)) == 0
    got = list(csv.reader(io.StringIO(capsys.readouterr().out)))
    ph = Sc.PhraseDetector(sc, [x.split() for x in names], window_ms=2000, combine="min", labels=labels)
    events = [[(s, e, c) for f, s, e, c in rows if f == w] for w in wavs]
    res = ph.sweep(out, sweep_audio.parse_thresholds("0:0.9:0.1"), events=events, tolerance_ms=300)
    cv = res.curve()
    assert got[0] == list(sweep_audio.COLUMNS) and got[1:] == [[str(x) for x in sweep_audio.format_row(cv, t)] for t in range(10)]
    assert int(cv["events"][0]) == 3 and int(res.detections[:, :, :2].sum()) > 0
    with pytest.raises(SystemExit, match="--phrases scores whole scans"):
        sweep_audio.main(sweep_audio.parse_arguments([*flags[:-1], "--chunk_seconds", "1"]))
