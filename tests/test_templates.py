"""Enrolled keywords (tcr_dtw_scores, tcresnet_amd.scanning.TemplateDetector): the keyword posteriors and lengths are bitwise the NumPy
definition (tests/dtw_ref.py) at every lane and frames-per-lane boundary, dense and ragged; the detector, sweep, grid and mining stages
run on them with K + 1 classes; a template enrolled from a recording scores exactly 1 where it was cut.  Emulator (`-m "not gpu"`) and
MI355X (`-m gpu`).  Every comparison is bitwise, values and lengths alike."""
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
from tests.test_streaming import frozen_artifact, segment_audio, setup

MARK = -7.0
TIE_AT, TIE_N = 10, 4           # template 4 (64 frames): frames 10 .. 13 are one row


def frames_max(F):
    """include/tcresnet_hip.h: tcr_dtw_frames_max."""
    return min(256, 4096 // F) if 1 <= F <= 64 else 0


def walk_rows(rng, L, F):
    """A template: softmax rows of a random walk in the logits, float32 [L, F]."""
    x = np.cumsum(rng.randn(L, F) * 0.7, axis=0) + rng.randn(F) * 1.5
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def template_set(F, seed=0):
    """Templates of 1, 2, 3, 63, 64, 65, 128 and tcr_dtw_frames_max(F) frames -- the lane and frames-per-lane boundaries -- as six
    keywords: those of 63, 64 and 65 frames are one keyword's three templates.  The one of 64 frames repeats a frame four times."""
    rng = np.random.RandomState(900 + 31 * F + seed)
    tm = [walk_rows(rng, L, F) for L in (1, 2, 3, 63, 64, 65, 128, frames_max(F))]
    tm[4][TIE_AT:TIE_AT + TIE_N] = tm[4][TIE_AT]
    kw_off = np.array([0, 1, 2, 3, 6, 7, 8], np.int32)
    scale = np.array([np.float32(0.5 / len(t)) for t in tm], np.float32)
    return tm, kw_off, scale


def at_rate(t, rate):
    """The template's rows spoken at `rate`: 0.5 every frame twice, 1 as it is, 2 every other frame."""
    return np.repeat(t, 2, axis=0) if rate == 0.5 else t[::int(rate)]


def planted(rng, steps, F, pieces):
    """`planted_rows` of test_phrases.py as the background, with `pieces` (arrays of rows) written over it one after the other, a
    gap of 0 .. 3 background rows between them -- gap 0 twice running is a piece back to back -- as far as they fit."""
    v = planted_rows(rng, steps, F) if steps else np.zeros((0, F), np.float32)
    pos = 0
    for p, gap in pieces:
        if pos + len(p) > steps:
            break
        v[pos:pos + len(p)] = p
        pos += len(p) + gap
    return v


def signal_plans(tm):
    """What the 257-row signals hold: every template spoken at rates 0.5, 1 and 2 (the longest at 1 and 2 only: at rate 0.5 it is 512
    rows, more than a signal here has), one template twice back to back, and blocks of eight identical rows that equal the repeated
    frame of the 64-frame template, so that exact ties between diag, stay and skip decide the lengths."""
    t1, t2, t3, t63, t64, t65, t128, tmax = tm
    tie = np.repeat(t64[TIE_AT:TIE_AT + 1], 8, axis=0)
    r = at_rate
    return [[(r(tmax, 1), 0)],
            [(r(tmax, 2), 1), (r(t128, 2), 2), (r(t3, 0.5), 1), (r(t3, 1), 0), (r(t3, 2), 3), (r(t2, 0.5), 1), (r(t2, 1), 1), (r(t1, 1), 1), (r(t1, 0.5), 0)],
            [(r(t128, 0.5), 0)],
            [(r(t128, 1), 0), (r(t63, 1), 0), (r(t63, 1), 0)],
            [(tie, 0), (r(t64, 2), 2), (r(t64, 1), 1), (r(t65, 2), 0), (r(t65, 1), 2), (r(t63, 2), 0)],
            [(r(t64, 0.5), 0), (r(t63, 0.5), 0)],
            [(r(t65, 0.5), 3), (r(t64, 1)[:TIE_AT + 1], 0), (tie, 0), (r(t64, 1)[TIE_AT + TIE_N:], 1), (r(t2, 2), 1), (r(t3, 1), 0)]]


RAGGED = [0, 257, 1, 2, 0, 257, 63, 64, 65, 257, 0, 0, 257, 257, 257, 257, 0]        # 0, 1, 2, L - 1, L, L + 1 (L = 64) and 257


def table_inputs(F):
    """-> templates, keyword_offsets, scale, (packed ragged rows, offsets), dense cube [3, 70, F]."""
    tm, kw_off, scale = template_set(F)
    rng = np.random.RandomState(77 + F)
    plans = signal_plans(tm)
    short = [[(at_rate(tm[3], 1), 0)], [(at_rate(tm[4], 1), 0)], [(at_rate(tm[5], 1), 0)]]      # the signals of 63, 64, 65 rows
    sigs, full, few = [], 0, 0
    for m in RAGGED:
        if m == 257:
            sigs.append(planted(rng, m, F, plans[full]))
            full += 1
        elif m >= 63:
            sigs.append(planted(rng, m, F, short[few]))
            few += 1
        else:
            sigs.append(planted(rng, m, F, []))
    assert full == len(plans)
    off = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
    cube = np.stack([planted(rng, 70, F, [(at_rate(tm[3], 1), 0), (at_rate(tm[2], 1), 0)]),
                     planted(rng, 70, F, [(at_rate(tm[2], 0.5), 1), (at_rate(tm[4], 2), 0), (at_rate(tm[3], 2), 0)]),
                     planted(rng, 70, F, [(at_rate(tm[1], 1), 2), (at_rate(tm[4], 1), 0)])])
    return tm, kw_off, scale, (np.concatenate(sigs), off), cube


class Call:
    """tcr_dtw_scores(_ragged) on host arrays, every device buffer with a guard band of MARK in front of and behind it; `shift` floats
    in front of every buffer make the pointers 4-byte aligned and no more."""

    GUARD = 64

    def __init__(self, lib, shift=0):
        self.lib, self.dev, self.shift = lib, Cm.device_of(lib), shift

    def buf(self, shape, dtype, fill=None, src=None):
        n = int(np.prod(shape))
        whole = torch.full((self.GUARD + self.shift + n + self.GUARD,), MARK if fill is None else fill,
                           dtype=torch.float32 if dtype == np.float32 else torch.int32, device=self.dev)
        part = whole[self.GUARD + self.shift:self.GUARD + self.shift + n]
        if src is not None:
            part.copy_(torch.from_numpy(np.ascontiguousarray(src, dtype).reshape(-1)).to(self.dev))
        return whole, part

    def guards_ok(self, whole, n):
        g = self.GUARD + self.shift
        return bool((whole[:g] == int(MARK)).all()) and bool((whole[g + n:] == int(MARK)).all())

    def __call__(self, values, tm, kw_off, scale, max_steps=0, offsets=None, want_lengths=True, check=True, frame_off=None, n_templates=None,
                 n_keywords=None, F=None, n=None, steps=None, holes=()):
        lib = self.lib
        values = np.ascontiguousarray(values, np.float32)
        flat = np.concatenate(tm) if len(tm) else np.zeros((1, values.shape[-1]), np.float32)
        fo = np.concatenate([[0], np.cumsum([len(t) for t in tm])]).astype(np.int32) if frame_off is None else np.asarray(frame_off, np.int32)
        kw_off, scale = np.ascontiguousarray(kw_off, np.int32), np.ascontiguousarray(scale, np.float32)
        Q = len(fo) - 1 if n_templates is None else n_templates
        K = len(kw_off) - 1 if n_keywords is None else n_keywords
        cols = max(len(kw_off) - 1, 1)
        rows = int(np.prod(values.shape[:-1]))
        v_whole, v = self.buf(values.shape, np.float32, src=values)
        t_whole, t = self.buf(flat.shape, np.float32, src=flat)
        o_whole, o = self.buf((rows, cols + 1), np.float32)
        l_whole, ln = self.buf((rows, cols), np.int32, fill=int(MARK))
        cfg = T._lib.DtwCfg(max_steps)
        tables = [Q, t.data_ptr(), fo.ctypes.data, K, kw_off.ctypes.data, scale.ctypes.data, C.byref(cfg)]
        tail = [o.data_ptr(), ln.data_ptr() if want_lengths else None, None]
        head = [values.shape[-1] if F is None else F, v.data_ptr()]
        so = None
        if offsets is not None:
            so = torch.from_numpy(np.asarray(offsets, np.int64)).to(self.dev)
            head = [len(offsets) - 1 if n is None else n, so.data_ptr(), values.shape[0] if steps is None else steps, *head]
        else:
            head = [values.shape[0] if n is None else n, values.shape[1] if steps is None else steps, *head]
        args = [*head, *tables, *tail]
        for h in holes:                                     # (counted from the end: the pointer arguments of both forms line up there)
            args[h] = None
        rc = (lib.tcr_dtw_scores if offsets is None else lib.tcr_dtw_scores_ragged)(*args)
        if check:
            lib.check(rc, "tcr_dtw_scores")
        assert self.guards_ok(o_whole, rows * (cols + 1)) and self.guards_ok(l_whole, rows * cols), "a guard band was written"
        assert self.guards_ok(v_whole, values.size) and self.guards_ok(t_whole, flat.size)
        out = o.cpu().numpy().reshape(*values.shape[:-1], cols + 1)
        return rc, out, ln.cpu().numpy().reshape(*values.shape[:-1], cols)


def check_table(lib, F, shift=0):
    """The library against the reference, ragged and dense, with and without a step limit."""
    tm, kw_off, scale, (packed, off), cube = table_inputs(F)
    call = Call(lib, shift)
    N, steps = cube.shape[:2]
    doff = np.arange(N + 1, dtype=np.int64) * steps
    for max_steps in (0, 200):
        want, wlen = DR.scores(packed, off, tm, kw_off, scale, max_steps)
        _, got, glen = call(packed, tm, kw_off, scale, max_steps, offsets=off)
        same(got, want, ("ragged", F, max_steps))
        same(glen, wlen, ("ragged lengths", F, max_steps))
        dwant, dlen = DR.scores(cube.reshape(N * steps, F), doff, tm, kw_off, scale, max_steps)
        _, got, glen = call(cube, tm, kw_off, scale, max_steps)
        same(got.reshape(N * steps, -1), dwant, ("dense", F, max_steps))
        same(glen.reshape(N * steps, -1), dlen, ("dense lengths", F, max_steps))
    _, got, glen = call(packed, tm, kw_off, scale, 200, offsets=off, want_lengths=False)       # lengths NULL: the posteriors all the same
    same(got, want, ("no lengths", F))
    assert (glen == int(MARK)).all()
    return tm, kw_off, scale, packed, off, want, wlen


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_reference_dp_equals_brute_force():
    """Guards the reference: on L <= 3, steps <= 6, F = 2 the DP's costs are the minimum over every admissible path of the
    left-to-right float32 sum -- the same bits, because float32 addition is monotone."""
    rng = np.random.RandomState(3)
    finite = 0
    for L in (1, 2, 3):
        for steps in (1, 2, 3, 6):
            for _ in range(3):
                Tm, v = walk_rows(rng, L, 2), walk_rows(rng, steps, 2)
                if steps >= 3:
                    v[1] = v[2] = Tm[0]                      # exact ties and a zero distance
                cost, length, _ = DR.walk(Tm, v)
                for t in range(steps):
                    brute = DR.cost_brute(Tm, v, t)
                    assert cost[t].tobytes() == np.float32(brute).tobytes(), (L, steps, t, cost[t], brute)
                    finite += bool(np.isfinite(brute))
                    assert (length[t] >= 1) and (not np.isfinite(brute) or (L + 1) // 2 <= length[t] <= t + 1)
    assert finite >= 60


@pytest.mark.parametrize("F", [3, 12])
def test_scores_equal_definition(emu_lib, F):
    check_table(emu_lib, F)


def test_inputs_discriminate():
    """On the reference: the planted templates peak at exactly 1, rates 0.5 and 2 take paths of other lengths, the tie block takes a
    decision, the three-template keyword is won by each of its templates somewhere, and the step limit zeroes scores."""
    tm, kw_off, scale, (packed, off), _ = table_inputs(12)
    want, wlen = DR.scores(packed, off, tm, kw_off, scale, 0)
    lim, _ = DR.scores(packed, off, tm, kw_off, scale, 200)
    for k in range(6):
        assert (want[:, k] == 1.0).any(), k
    a = int(off[1])                                         # the first full signal: the longest template at rate 1
    assert want[a + 255, 5] == 1.0 and wlen[a + 255, 5] == len(tm[7]) == 256
    assert int((lim != want).any(axis=1).sum()) >= 1 and (lim[a + 255, 5] == 0.0)
    assert len(set(wlen[want[:, 4] > 0.8, 4].tolist())) >= 3          # 128 frames at rates 0.5, 1, 2: 256, 128 and 64 steps or so
    winners = set()
    for q in (3, 4, 5):
        cost, length, _ = DR.walk(tm[q], packed[off[13]:off[14]])          # the signal that holds all three
        c = DR.conf_of(cost, length, scale[q], 0)
        winners |= {q for t in range(len(c)) if c[t] == 1.0 and c[t] == want[off[13] + t, 3] and length[t] == wlen[off[13] + t, 3]}
    assert winners == {3, 4, 5}


# ---- 2. properties ----------------------------------------------------------------------------------------------------------------------
def check_properties(lib):
    rng = np.random.RandomState(12)
    F = 12
    call = Call(lib, shift=1)                               # every pointer 4-byte aligned and no more
    # a signal shorter than ceil(L / 2) cannot reach the last frame: 0 throughout, background 1; at ceil(L / 2) rows it can
    for L in (8, 9, 130):
        tm = [walk_rows(rng, L, F)]
        need = (L + 1) // 2
        v = planted_rows(rng, need, F)
        for m in (need - 1, need):
            want, wlen = DR.scores(v[:m], [0, m], tm, [0, 1], [np.float32(0.5 / L)])
            _, got, glen = call(v[None, :m], tm, [0, 1], [np.float32(0.5 / L)])
            same(got[0], want, ("short", L, m))
            same(glen[0], wlen, ("short lengths", L, m))
        assert (want[:need - 1, 0] == 0).all() and (want[:need - 1, 1] == 1).all()
        cost, length, _ = DR.walk(tm[0], v)
        assert not np.isfinite(cost[:need - 1]).any() and np.isfinite(cost[need - 1]) and length[need - 1] == need
    # a template cut from the values scores exactly 1 with length L at the range's last row
    v = planted_rows(rng, 90, F)
    tm = [v[20:20 + 37].copy(), v[5:5 + 1].copy(), v[60:60 + 30].copy()]
    kw, sc = [0, 1, 2, 3], [np.float32(0.5 / len(t)) for t in tm]
    _, got, glen = call(v[None], tm, kw, sc)
    want, wlen = DR.scores(v, [0, 90], tm, kw, sc)
    same(got[0], want, "cut")
    same(glen[0], wlen, "cut lengths")
    for k, (a, L) in enumerate(((20, 37), (5, 1), (60, 30))):
        assert got[0, a + L - 1, k] == 1.0 and glen[0, a + L - 1, k] == L
    # max_steps at its boundary: a match of exactly max_steps steps is kept, of one more zeroed
    t, k = 20 + 37 - 1, 0
    for limit, kept in ((37, True), (36, False)):
        _, g2, l2 = call(v[None], tm, kw, sc, max_steps=limit)
        w2, wl2 = DR.scores(v, [0, 90], tm, kw, sc, limit)
        same(g2[0], w2, ("limit", limit))
        same(l2[0], wl2, ("limit lengths", limit))
        assert (g2[0, t, k] == 1.0) == kept and (kept or g2[0, t, k] == 0.0) and l2[0, t, k] == 37
    # the rows behind the call's last row stay as they were: a call over the first 50 rows of a larger buffer
    dev = Cm.device_of(lib)
    out = torch.full((90, 4), MARK, device=dev)
    ln = torch.full((90, 3), int(MARK), dtype=torch.int32, device=dev)
    vd, td = torch.from_numpy(v).to(dev), torch.from_numpy(np.concatenate(tm)).to(dev)
    fo, ko, s_ = np.array([0, 37, 38, 68], np.int32), np.array(kw, np.int32), np.array(sc, np.float32)
    cfg = T._lib.DtwCfg(0)
    lib.check(lib.tcr_dtw_scores(1, 50, F, vd.data_ptr(), 3, td.data_ptr(), fo.ctypes.data, 3, ko.ctypes.data, s_.ctypes.data, C.byref(cfg),
                                 out.data_ptr(), ln.data_ptr(), None), "tcr_dtw_scores")
    same(out[:50].cpu().numpy(), want[:50], "first 50")
    same(ln[:50].cpu().numpy(), wlen[:50], "first 50 lengths")
    assert bool((out[50:] == MARK).all()) and bool((ln[50:] == int(MARK)).all())


def test_properties(emu_lib):
    check_properties(emu_lib)


def test_ragged_signal_never_reads_its_predecessor(emu_lib):
    F = 12
    rng = np.random.RandomState(9)
    tm = [walk_rows(rng, 20, F)]
    first, second = planted_rows(rng, 40, F), planted_rows(rng, 30, F)
    first[-12:] = tm[0][:12]                                # the template starts in the predecessor's last rows
    second[:8] = tm[0][12:]                                 # and ends in the signal's first: a match if the rows were one signal's
    packed = np.concatenate([first, second])
    sc = [np.float32(0.5 / 20)]
    call = Call(emu_lib)
    _, got, glen = call(packed, tm, [0, 1], sc, offsets=[0, 40, 70])
    _, alone, alen = call(second[None], tm, [0, 1], sc)
    same(got[40:], alone[0], "isolation")
    same(glen[40:], alen[0], "isolation lengths")
    joined, _ = DR.scores(packed, [0, 70], tm, [0, 1], sc)
    assert joined[47, 0] == 1.0 and alone[0, 7, 0] < 1.0


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_c_refusals_write_nothing(emu_lib):
    lib = emu_lib
    rng = np.random.RandomState(2)
    F = 4
    v = planted_rows(rng, 30, F)[None]
    tm = [walk_rows(rng, 5, F), walk_rows(rng, 3, F), walk_rows(rng, 7, F)]
    kw, sc = [0, 2, 3], [0.1, 0.2, 0.3]
    call = Call(lib)

    def refused(msg, values=v, tm=tm, kw=kw, sc=sc, ragged=False, **more):
        offsets = None
        if ragged:
            values, offsets = values.reshape(-1, values.shape[-1]), [0, 10, values.shape[1]]
        rc, out, ln = call(values, tm, kw, sc, offsets=offsets, check=False, **more)
        name = "tcr_dtw_scores_ragged: " if ragged else "tcr_dtw_scores: "
        err = lib.tcr_last_error().decode()
        assert rc == -1 and name in err and msg in err, (msg, rc, err)
        assert (out == MARK).all() and (ln == int(MARK)).all(), msg

    assert call(v, tm, kw, sc)[0] == 0
    for ragged in (False, True):
        for hole in (-3, -4, -5, -6, -8, -9, -11):         # (lengths may be null) out, cfg, scale, keyword_offsets, frame_offsets, templates, values
            refused("null argument", holes=(hole,), ragged=ragged)
        refused("n_features must be positive (got 0)", F=0, ragged=ragged)
        refused("n_features must be positive (got -1)", F=-1, ragged=ragged)
        refused("n_features 65 above TCR_DTW_MAX_FEATURES = 64", F=65, ragged=ragged)
        refused("n_templates 0 outside 1..64", n_templates=0, ragged=ragged)
        refused("n_templates 65 outside 1..64", n_templates=65, ragged=ragged)
        refused("n_keywords 0 outside 1..3", n_keywords=0, ragged=ragged)
        refused("n_keywords 4 outside 1..3", n_keywords=4, ragged=ragged)
        refused("frame_offsets must start at 0 (got 1)", frame_off=[1, 5, 8, 15], ragged=ragged)
        refused("frame_offsets decrease at template 1 (4 after 5)", frame_off=[0, 5, 4, 15], ragged=ragged)
        refused("template 1 has 0 frames (1..tcr_dtw_frames_max(4) = 256)", frame_off=[0, 5, 5, 15], ragged=ragged)
        refused("keyword_offsets must start at 0 (got 1)", kw=[1, 2, 3], ragged=ragged)
        refused("keyword_offsets decrease at keyword 1 (1 after 2)", kw=[0, 2, 1], n_keywords=2, ragged=ragged)
        refused("keyword 0 has no template", kw=[0, 0, 3], ragged=ragged)
        refused("keyword_offsets must end at n_templates = 3 (got 2)", kw=[0, 1, 2], ragged=ragged)
        for bad in (0.0, -0.5, np.inf, np.nan):
            refused("scale[1] = ", sc=[0.1, bad, 0.3], ragged=ragged)
        refused("max_steps must be >= 0 (got -1)", max_steps=-1, ragged=ragged)
        refused("the number of steps must be positive (got 0)", steps=0, ragged=ragged)
        refused("the number of steps must be positive (got -3)", steps=-3, ragged=ragged)
        refused("the number of signals must be positive (got 0)", n=0, ragged=ragged)
        refused("is too large", steps=(1 << 31) // 4, ragged=ragged)
    refused("tcr_dtw_scores_ragged: null argument", ragged=True, holes=(-14,))      # step_offsets
    # a template above the limit: 257 frames at F = 4, 65 at F = 64
    long = [walk_rows(rng, 257, F)]
    refused("template 0 has 257 frames (1..tcr_dtw_frames_max(4) = 256)", tm=long, kw=[0, 1], sc=[0.1])
    wide = planted_rows(rng, 10, 64)[None]
    refused("template 0 has 65 frames (1..tcr_dtw_frames_max(64) = 64)", values=wide, tm=[walk_rows(rng, 65, 64)], kw=[0, 1], sc=[0.1])
    assert call(wide, [walk_rows(rng, 64, 64)], [0, 1], [0.1])[0] == 0       # (the limit itself is taken)
    assert [lib.tcr_dtw_frames_max(f) for f in (0, 1, 3, 12, 16, 17, 64, 65)] == [frames_max(f) for f in (0, 1, 3, 12, 16, 17, 64, 65)] == \
        [0, 256, 256, 256, 256, 240, 64, 0]


def test_python_refusals(emu_lib):
    Sc = scanning()
    fe, net, _, _, _ = setup(emu_lib)
    scanner = Sc.KeywordScanner(net, fe, **DET)
    rng = np.random.RandomState(4)
    kt = Sc.KeywordTemplates()
    with pytest.raises(T.TcrError, match="at least one template"):
        Sc.TemplateDetector(scanner, kt)
    with pytest.raises(T.TcrError, match=r"float32 \[L, F\]"):
        kt.add("a", np.zeros((0, 12), np.float32))
    with pytest.raises(T.TcrError, match="cannot name a keyword"):
        kt.add("_background_", walk_rows(rng, 4, 12))
    kt.add("a", walk_rows(rng, 4, 12))
    with pytest.raises(T.TcrError, match="template of 5 features in a set of 12"):
        kt.add("b", walk_rows(rng, 4, 5))
    with pytest.raises(T.TcrError, match="on must be 'smoothed' or 'probs'"):
        Sc.TemplateDetector(scanner, kt, on="logits")
    with pytest.raises(T.TcrError, match="longer than the model's clip of 16000"):
        kt.enroll(scanner, "a", np.zeros(16000, np.float32))
    five = Sc.KeywordTemplates()
    five.add("a", walk_rows(rng, 4, 5))
    with pytest.raises(T.TcrError, match="the templates have 5 features, the scanner 12 classes"):
        Sc.TemplateDetector(scanner, five)
    big = Sc.KeywordTemplates()
    big.add("a", walk_rows(rng, 257, 12))
    with pytest.raises(T.TcrError, match=r"257 frames is above tcr_dtw_frames_max\(12\) = 256"):
        Sc.TemplateDetector(scanner, big)
    many = Sc.KeywordTemplates()
    for i in range(65):
        many.add(f"k{i % 3}", walk_rows(rng, 2, 12))
    with pytest.raises(T.TcrError, match=r"65 templates \(1..64\)"):
        Sc.TemplateDetector(scanner, many)
    td = Sc.TemplateDetector(scanner, kt)
    sm = torch.rand(2, 9, 12, device=Cm.device_of(emu_lib))
    wrong = Sc.ScanOutput(None, sm[..., :5].contiguous(), sm[..., :5].contiguous(), None, None, None)
    for fn in (td.scores, td.detect, lambda o: td.sweep(o, [0.5])):
        with pytest.raises(T.TcrError, match="is not a scan of the scanner's 12 classes"):
            fn(wrong)
    with pytest.raises(T.TcrError, match="on must be 'smoothed' or 'probs'"):
        td.scores(Sc.ScanOutput(None, sm, sm, None, None, None), on="logits")
    with pytest.raises(T.TcrError, match="n_streams must be positive"):
        td.streaming(0)


# ---- 4. the detector and the keyword stages over template posteriors ----------------------------------------------------------------------
def word_rows(steps, runs, ncls=12, high=0.9):
    v = np.full((steps, ncls), (1.0 - high) / (ncls - 1), np.float32)
    v[:, 0] = high
    for a, b, c in runs:
        v[a:b + 1] = (1.0 - high) / (ncls - 1)
        v[a:b + 1, c] = high
    return v


def stage_case(lib):
    """A scanner, two enrolled keywords -- "rise" (class 2 then 3: two templates, one slower) and "fall" (3 then 2) -- and a dense
    `ScanOutput` of two planted signals (no audio behind it): signal 0 says "rise", "fall" and a slow "rise", signal 1 "fall" and then
    "rise".  (The runs are rows that equal the templates' frames, so zero-cost paths tie all along them.)"""
    Sc = scanning()
    fe, net, _, _, _ = setup(lib)
    scanner = Sc.KeywordScanner(net, fe, **DET)
    kt = Sc.KeywordTemplates()
    kt.add("rise", word_rows(10, [(0, 4, 2), (5, 9, 3)]))
    kt.add("fall", word_rows(10, [(0, 4, 3), (5, 9, 2)]))
    kt.add("rise", word_rows(16, [(0, 7, 2), (8, 15, 3)]))
    steps = 140
    sig = np.stack([word_rows(steps, [(10, 14, 2), (15, 19, 3), (40, 44, 3), (45, 49, 2), (70, 77, 2), (78, 85, 3)]),
                    word_rows(steps, [(20, 24, 3), (25, 29, 2), (90, 94, 2), (95, 99, 3)])])
    sm = torch.from_numpy(sig).to(Cm.device_of(lib))
    out = Sc.ScanOutput(None, sm, sm, None, None, None)
    td = Sc.TemplateDetector(scanner, kt, detection_threshold=0.95, suppression_ms=100)
    return Sc, scanner, kt, td, out, sig


def ref_tables(kt):
    flat = [t for v in kt.keywords.values() for t in v]
    kw_off = np.concatenate([[0], np.cumsum([len(v) for v in kt.keywords.values()])]).astype(np.int32)
    return flat, kw_off, np.array([np.float32(0.5 / len(t)) for t in flat], np.float32)


def check_stages(lib):
    Sc, scanner, kt, td, out, sig = stage_case(lib)
    assert td.labels == ["rise", "fall", "_background_"] and td.num_classes == 3 and kt.names == ["rise", "fall"] and len(kt) == 3
    assert td.max_steps == 48 and td.det.suppression_steps == 5 and td.det.average_steps == td.det.min_count == 1
    assert td.tables.scale.tobytes() == np.array([0.5 / 10, 0.5 / 16, 0.5 / 10], np.float32).tobytes()
    flat, kw_off, scale = ref_tables(kt)
    assert [len(t) for t in flat] == [10, 16, 10] and kw_off.tolist() == [0, 2, 3]
    det, lengths = td.detect(out, return_lengths=True)
    assert isinstance(det, Sc.ScanOutput) and det.logits is None and det.smoothed is det.probs
    same(td.scores(out).cpu().numpy(), det.probs.cpu().numpy())
    rule = []
    for n in range(2):
        post, wlen = DR.scores(sig[n], [0, sig.shape[1]], flat, kw_off, scale, 48)
        same(det.probs[n].cpu().numpy(), post, "posteriors")
        same(lengths[n].cpu().numpy(), wlen, "lengths")
        top, score, new = PR.detect_rule(post, 5, 0.95)
        assert det.top[n].cpu().numpy().tobytes() == top.tobytes()
        assert det.score[n].cpu().numpy().tobytes() == score.tobytes()
        assert det.is_new[n].cpu().numpy().tobytes() == new.tobytes()
        rule.append((post, top, new))
    fired = [[(int(s), int(rule[n][1][s])) for s in np.flatnonzero(rule[n][2]) if rule[n][1][s] < 2] for n in range(2)]
    # each at the first step a path of no cost ends: rise, fall, rise; fall, rise (a keyword fires again once another label has)
    assert fired[0] == [(17, 0), (47, 1), (80, 0)] and fired[1] == [(27, 1), (97, 0)]
    assert det.probs[0, 19, 0] == 1.0 and lengths[0, 19, 0] == 10 and det.probs[0, 85, 0] == 1.0
    # the ragged form and a cascade's output of the same rows
    flat_sm = out.smoothed.reshape(-1, 12)
    rout = Sc.RaggedScanOutput(None, flat_sm, flat_sm, None, None, None, np.array([0, 140, 280], np.int64))
    rdet = td.detect(rout)
    assert isinstance(rdet, Sc.RaggedScanOutput)
    for f in ("probs", "top", "score", "is_new"):
        assert torch.equal(getattr(rdet, f), getattr(det, f).reshape(280, *getattr(det, f).shape[2:])), f
    cout = Sc.CascadeOutput(None, flat_sm, flat_sm, None, None, None, rout.offsets, torch.zeros(0, dtype=torch.int64), rout)
    cdet = td.detect(cout)
    assert isinstance(cdet, Sc.CascadeOutput) and cdet.first is rout and torch.equal(cdet.is_new, rdet.is_new)
    # sweep: per threshold the rule's detections; hits and false accepts against a labelled layout
    thr = [0.3, 0.95, 0.99]
    step_ms = scanner.step_ms
    events = [[(12 * step_ms, 25 * step_ms, "rise"), (42 * step_ms, 55 * step_ms, "fall")],
              [(22 * step_ms, 35 * step_ms, "fall"), (92 * step_ms, 105 * step_ms, 0)]]
    res = td.sweep(out, thr, events=events, tolerance_ms=0.0)
    assert isinstance(res, Sc.PhraseSweepResult) and tuple(res.detections.shape) == (2, 3, 3)
    counts = np.zeros((2, 3, 3), np.int64)
    for n in range(2):
        for j, th in enumerate(thr):
            top, _, new = PR.detect_rule(rule[n][0], 5, th)
            for s in np.flatnonzero(new):
                counts[n, j, top[s]] += 1
    assert np.array_equal(res.detections.cpu().numpy(), counts) and counts[:, 1, :2].sum() == 5
    cv = res.curve()
    assert cv["hits"][1] == 4 and cv["false_accepts"][1] == 1            # signal 0's second "rise" is the planted false accept
    grid = td.tune(out, thr, suppression_ms=(100, 1200), events=events, tolerance_ms=0.0)
    assert isinstance(grid, Sc.PhraseGridResult) and len(grid) == 2
    assert torch.equal(grid.result(0).detections, res.detections) and not torch.equal(grid.detections[0], grid.detections[1])
    wide = Sc.TemplateDetector(scanner, kt, detection_threshold=0.95, suppression_ms=1200).sweep(out, thr, events=events, tolerance_ms=0.0)
    assert torch.equal(grid.result(1).detections, wide.detections) and torch.equal(grid.result(1).hits, wide.hits)
    audio = torch.from_numpy(segment_audio(2, 140 * scanner.step_samples, 3)).to(Cm.device_of(lib))
    mined = td.mine(out, audio, events=events, k=10, tolerance_ms=0.0)
    assert len(mined) == 1 and mined.kind_names() == ["false_accept"]
    assert (int(mined.signal[0]), int(mined.step[0]), int(mined.label[0])) == (0, 80, 0)
    end = 81 * scanner.step_samples
    assert torch.equal(mined.clips[0], audio[0, end - 16000:end])


def test_detect_sweep_tune_and_mine(emu_lib):
    check_stages(emu_lib)


# ---- 5. end to end through a real scanner -------------------------------------------------------------------------------------------------
def check_enrolled(lib, tmp_path):
    Sc = scanning()
    fe, net, _, _, _ = setup(lib)
    from tcresnet_amd.deploy import FrozenModel
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    scanner = FrozenModel.load(path, lib=lib, device=Cm.device_of(lib)).scanner(frames_per_step=2, **DET)
    step = scanner.step_samples
    audio = segment_audio(2, 60 * step, 41)
    kt = Sc.KeywordTemplates()
    t0 = kt.enroll(scanner, "first", audio[0], start_ms=10 * scanner.step_ms, end_ms=30 * scanner.step_ms)      # steps 9 .. 29
    t1 = kt.enroll(scanner, "second", audio[1, :40 * step + 7], max_frames=16, on="probs")                       # 40 rows, every third: 14
    t2 = kt.enroll(scanner, "first", torch.from_numpy(audio[1]).to(scanner.device), start_ms=1205.0)
    scan = scanner.scan(torch.from_numpy(audio).to(scanner.device))
    sm, pr = scan.smoothed.cpu().numpy(), scan.probs.cpu().numpy()
    same(t0, sm[0, 9:30], "enrolled rows")
    same(t1, pr[1, :40:3], "every third row")
    first = int(np.ceil(1205.0 / scanner.step_ms)) - 1
    same(t2, sm[1, first:], "from start_ms on")
    assert kt.names == ["first", "second"] and [len(t) for t in kt.keywords["first"]] == [21, 60 - first]
    kt.save(str(tmp_path / "templates.npz"))
    back = Sc.KeywordTemplates.load(str(tmp_path / "templates.npz"))
    assert back.names == kt.names
    for name in kt.names:
        assert len(back.keywords[name]) == len(kt.keywords[name])
        for a, b in zip(back.keywords[name], kt.keywords[name]):
            same(a, b, "round trip")
    td = Sc.TemplateDetector(scanner, back, detection_threshold=0.9, suppression_ms=0)
    det, lengths = td.detect(scan, return_lengths=True)
    post, ln = det.probs.cpu().numpy(), lengths.cpu().numpy()
    assert post[0, 29, 0] == 1.0 and ln[0, 29, 0] == 21                      # where it was cut: exactly 1, the template's length
    assert post[1, 59, 0] == 1.0 and ln[1, 59, 0] == 60 - first
    flat, kw_off, scale = ref_tables(back)
    want, wlen = DR.scores(sm.reshape(120, 12), [0, 60, 120], flat, kw_off, scale, td.max_steps)
    same(post.reshape(120, 3), want, "real scan")
    same(ln.reshape(120, 2), wlen, "real scan lengths")
    for n in range(2):
        top, score, new = PR.detect_rule(post[n], 0, 0.9)
        assert det.top[n].cpu().numpy().tobytes() == top.tobytes() and det.is_new[n].cpu().numpy().tobytes() == new.tobytes()
        assert det.score[n].cpu().numpy().tobytes() == score.tobytes()
    assert int(det.top[0, 29]) == 0 and float(det.score[0, 29]) == 1.0
    on_probs = Sc.TemplateDetector(scanner, back, on="probs").scores(scan)
    same(on_probs.cpu().numpy().reshape(120, 3), DR.scores(pr.reshape(120, 12), [0, 60, 120], flat, kw_off, scale, td.max_steps)[0], "on probs")
    rag = scanner.scan_ragged([torch.from_numpy(audio[0, :22 * step]).to(scanner.device), torch.from_numpy(audio[1, :0]).to(scanner.device),
                               torch.from_numpy(audio[1]).to(scanner.device)])
    rdet = td.detect(rag)
    assert isinstance(rdet, Sc.RaggedScanOutput) and torch.equal(rdet.probs[22:], det.probs[1]) and torch.equal(rdet.probs[:22], det.probs[0, :22])


def test_enrolled_template_scores_one_where_it_was_cut(emu_lib, tmp_path):
    check_enrolled(emu_lib, tmp_path)


# ---- MI355X -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("F", [3, 12])
def test_gpu_scores_equal_definition(hip_lib, F):
    check_table(hip_lib, F)


@pytest.mark.gpu
def test_gpu_properties(hip_lib):
    check_properties(hip_lib)


@pytest.mark.gpu
def test_gpu_detect_sweep_tune_and_mine(hip_lib):
    check_stages(hip_lib)


@pytest.mark.gpu
def test_gpu_enrolled_template_scores_one_where_it_was_cut(hip_lib, tmp_path):
    check_enrolled(hip_lib, tmp_path)
