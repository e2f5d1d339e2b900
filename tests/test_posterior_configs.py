"""The posterior transforms across their configuration space (tests/posterior_configs.py): phrase scores (csrc/phrase.hip) at every
word count 1 .. 8 in both forms of the unrolled walk, at 63 and 64 phrases, 35 and 64 staged word classes, 35-, 46- and 70-class rows
and dynamic LDS from 11 KB to exactly 64 KB (the launches above 32 KB raise the kernel's limit first); template scores (csrc/dtw.hip)
at 1 .. 64 features -- tiles of 64, 60, 29, 25 and 16 rows, one to four frames a lane behind them, 64 templates in 64 keywords and
in one -- on an exact tie between two templates and at the length clamp; whole scans and carried pushes alike.  Every comparison is
bitwise against the NumPy definitions (tests/phrase_ref.py, tests/dtw_ref.py, `detect_rule`); the guards at the top show on the
reference alone that the rows reach the listed cases and that their inputs tell a wrong kernel from a right one.  Emulator
(`-m "not gpu"`) and MI355X (`-m gpu`), from the same rows."""
import numpy as np
import pytest
import torch

from oracle import numpy_ref as R
from tests import common as Cm
from tests import dtw_ref as DR
from tests import phrase_ref as PR
from tests import posterior_configs as PC
from tests import test_phrase_stream as TPS
from tests import test_template_stream as TTS
from tests.test_net_configs import Log, kernel_of
from tests.test_phrases import DET, lib_scores, same
from tests.test_scan import scanning
from tests.test_streaming import segment_audio
from tests.test_templates import Call, planted, walk_rows

INT32_MAX = 2 ** 31 - 1


# ---- 1. guards: the rows reach the cases, the inputs discriminate (host only) ----------------------------------------------------------
def test_rows_hold_the_listed_cases():
    """Computed from the rows: every word count in every mode (a row runs all four), 63 and 64 phrases, 35 and 64 staged classes, an
    LDS request above 32 KB and one of exactly 64 KB, every tile height, one to four frames a lane at more than 16 features, and the
    table limits; a row's stated geometry is the restatement's."""
    for r in PC.PHRASE_ROWS:
        assert (PC.distinct(r.phrases), PC.phrase_lds(r.phrases, r.w)) == (r.U, r.lds), r.name
        assert 1 <= r.w <= PC.window_max(r.U) and r.lds <= 65536 and all(0 <= c < r.C for q in r.phrases for c in q), r.name
        assert len(r.lengths) == len(PC.phrase_inputs(r.name).off) - 1
    rows = PC.PHRASE_ROW
    assert {len(q) for q in rows["word_counts"].phrases} == {1, 4, 5, 6, 7, 8}
    assert {len(q) for r in PC.PHRASE_ROWS for q in r.phrases} == set(range(1, 9)) and len(PC.MODES) == 4
    assert {len(q) for name in PC.STREAM_ROWS for q in rows[name].phrases} == set(range(1, 9))          # the run form too
    wc = rows["word_counts"].phrases
    assert any(len(q) != len(set(q)) for q in wc) and any(a[::-1] == b[:len(a)] for a in wc for b in wc if a is not b)
    assert {len(r.phrases) for r in PC.PHRASE_ROWS} >= {63, 64}
    assert all(sorted(len(rows["p64"].phrases[q]) for q in range(wave, 64, 4)) == sorted([1 + wave, 5 + wave] * 8) for wave in range(4))
    assert {r.U for r in PC.PHRASE_ROWS} >= {35, 64} and {r.C for r in PC.PHRASE_ROWS} >= {35, 46, 70}
    assert rows["u35_wmax"].w == PC.window_max(35) == 213 and rows["u64_w1"].w == PC.window_max(64) == 1
    assert rows["lds_64k_short"].w == 7937 > max(rows["lds_64k_short"].lengths)                        # the window never fills
    full = rows["lds_64k_full"]
    assert full.w == 3841 and max(full.lengths) >= full.w + PC.TILE + 1                                 # fills, then slides over a tile and more
    lds = [r.lds for r in PC.PHRASE_ROWS]
    assert any(32768 < x < 65536 for x in lds) and lds.count(65536) >= 3 and any(x <= 32768 for x in lds)
    assert {rows[name].lds > 32768 for name in PC.STREAM_ROWS} == {False, True}                         # the carried arm's launcher too
    # templates
    for g in PC.TEMPLATE_GEOM:
        assert (PC.frames_max(g.F), PC.tile_rows(g.F)) == (g.Lm, g.tr), g
    assert sorted(PC.GEOM[F].tr for F in PC.FEATURES) == [16, 16, 25, 29, 60, 64, 64, 64]
    assert {PC.GEOM[F].tr for F in PC.STREAM_FEATURES} == {60, 29, 16}
    assert {PC.fpl(L) for F in PC.FEATURES if F > 16 for L in PC.template_lengths(F)} == {1, 2, 3, 4}
    assert {PC.fpl(len(t)) for t in PC.stream_templates(17)[0]} == {1, 2, 4}
    assert max(PC.dtw_lds(PC.template_inputs(F).tm, F) for F in PC.FEATURES) == 32256 == PC.dtw_lds(PC.template_inputs(63).tm, 63)
    for F in PC.FEATURES:
        x, g = PC.template_inputs(F), PC.GEOM[F]
        assert [len(t) for t in x.tm] == PC.template_lengths(F) and max(len(t) for t in x.tm) == g.Lm and x.tm[0].shape[1] == F
        assert x.kw_off.tolist()[:3] == [0, 2, 3] and x.kw_off[-1] == len(x.tm) == len(x.kw_off)
        assert np.diff(x.off).tolist() == [0, g.tr - 1, g.tr, g.tr + 1, 2 * g.tr, 2 * g.tr + 1, 3 * g.tr + 5, 1, 0, g.Lm + 7]
    assert {F for F in PC.FEATURES if 1024 % F} == {17, 35, 40, 63}      # dead floats behind a fetch's rows, a tile boundary inside a wave
    assert {(len(k) - 1, int(k[-1])) for k in PC.LIMIT_TABLES.values()} == {(64, 64), (1, 64)}
    assert [len(t) for t in PC.limit_inputs(12)[0]] == [1 + q % 8 for q in range(64)]


def _columns(a, b):
    """Per column: do the two differ on some row."""
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=0)


@pytest.mark.parametrize("name", PC.PHRASE_IDS)
def test_phrase_inputs_discriminate(name):
    """On the reference, in every mode: every phrase scores above 0.25 somewhere; a phrase of 4 .. 7 words without its last word
    scores differently somewhere (an instance of another word count would show), and so does an ordered phrase reversed -- where
    the window holds more than one row: at w = 1 every word of a chain is read in the same row, so the order cannot matter (the
    minimum is the same number exactly, the product up to its rounding)."""
    r, x = PC.PHRASE_ROW[name], PC.phrase_inputs(name)
    P = len(r.phrases)
    cut = [(int(a), int(min(b, a + PC.GUARD_CUT))) for a, b in zip(x.off[:-1], x.off[1:]) if b > a]
    rows = np.concatenate([x.packed[a:b] for a, b in cut])
    coff = np.concatenate([[0], np.cumsum([b - a for a, b in cut])])
    short = [q for q in range(P) if 4 <= len(r.phrases[q]) <= 7]
    turned = [q for q in range(P) if r.phrases[q] != r.phrases[q][::-1]]
    for ordered, combine in PC.MODES:
        want = PC.phrase_reference(name, ordered, combine)[0]
        assert (want[:, :P] > 0.25).any(axis=0).all(), (name, ordered, combine, np.flatnonzero(~(want[:, :P] > 0.25).any(axis=0)))
        part = np.concatenate([want[a:b] for a, b in cut])
        if short:
            less = PR.scores(rows, coff, [r.phrases[q][:-1] for q in short], r.w, ordered, combine)
            assert _columns(less[:, :-1], part[:, short]).all(), (name, ordered, combine, "last word")
        if ordered and turned and r.w > 1:
            back = PR.scores(rows, coff, [r.phrases[q][::-1] for q in turned], r.w, ordered, combine)
            assert _columns(back[:, :-1], part[:, turned]).all(), (name, ordered, combine, "reversed")


def test_fast_reference_equals_the_definition():
    """`scores_dp_fast`, the reference of lds_64k_full, is bitwise the step-by-step definition on a 300-row cut of that row's input."""
    r, x = PC.PHRASE_ROW["lds_64k_full"], PC.phrase_inputs("lds_64k_full")
    a = PC.TILE - 30                                        # (the utterances start at row 236)
    rows = x.packed[a:a + 300]
    for ordered, combine in PC.MODES:
        same(PR.scores_dp_fast(rows, r.phrases, r.w, bool(ordered), combine), PR.scores(rows, [0, 300], r.phrases, r.w, ordered, combine, fast=False),
             (ordered, combine))
        same(PR.scores_dp_fast(rows, r.phrases, 40, bool(ordered), combine), PR.scores(rows, [0, 300], r.phrases, 40, ordered, combine, fast=False),
             (40, ordered, combine))


@pytest.mark.parametrize("F", PC.FEATURES)
def test_template_inputs_discriminate(F):
    """On the reference: every keyword reaches exactly 1; the last feature column matters; the rows around the first tile boundary
    carry scores; the step limit zeroes some."""
    x, g = PC.template_inputs(F), PC.GEOM[F]
    K = len(x.kw_off) - 1
    want, wlen, dwant, _ = PC.template_reference(F, 0)
    assert (want[:, :K] == 1.0).any(axis=0).all(), (F, np.flatnonzero(~(want[:, :K] == 1.0).any(axis=0)))
    other = x.packed.copy()
    other[:, F - 1] = np.clip(other[:, F - 1] + np.float32(0.125), 0, 1)
    moved = DR.scores(other, x.off, x.tm, x.kw_off, x.scale, 0)[0]
    assert _columns(moved[:, :K], want[:, :K]).all(), F
    if F > 1:                                               # a neighbour's column in its place
        rolled = DR.scores(np.roll(x.packed, 1, axis=1), x.off, x.tm, x.kw_off, x.scale, 0)[0]
        assert _columns(rolled[:, :K], want[:, :K]).all(), F
    edge = [int(a) + t for a, b in zip(x.off[:-1], x.off[1:]) for t in (g.tr - 1, g.tr, g.tr + 1) if a + t < b]
    assert len(edge) >= 12 and (want[edge, :K] > 0).any(axis=1).sum() >= 3, F
    lim = PC.template_reference(F, x.limit)[0]
    assert (lim != want).any() and (dwant[:, :K] == 1.0).any()
    assert g.Lm in wlen[:, PC.template_lengths(F).index(g.Lm) - 1]     # (the longest template's keyword: a path of all its frames)


# ---- 2. phrase scores, whole scans -----------------------------------------------------------------------------------------------------
def check_phrase_row(lib, name):
    """Ragged and dense, every mode, against the shared reference."""
    r, x = PC.PHRASE_ROW[name], PC.phrase_inputs(name)
    N, steps = r.dense
    for ordered, combine in PC.MODES:
        want, dwant = PC.phrase_reference(name, ordered, combine)
        same(lib_scores(lib, x.packed, r.phrases, r.w, ordered, combine, offsets=x.off)[1], want, ("ragged", name, ordered, combine))
        same(lib_scores(lib, x.cube, r.phrases, r.w, ordered, combine)[1].reshape(N * steps, -1), dwant, ("dense", name, ordered, combine))


@pytest.mark.parametrize("name", PC.PHRASE_IDS)
def test_phrase_scores_equal_definition(emu_lib, name):
    check_phrase_row(emu_lib, name)


# ---- 3. phrase streaming ---------------------------------------------------------------------------------------------------------------
def pushed(st, lib, chunks, **kw):
    """`Carried.push`, and from the emulator's launch log which of the two posterior kernels it ran: the lane kernel up to four rows
    a stream on average, the staged one above."""
    with Log(lib) as g:
        got = st.push(chunks, **kw)
    if lib.kind == "emu":
        ran = {kernel_of(e) for e in g.entries} & {"phrase_kernel", "phrase_lane_kernel"}
        rows = sum(len(c) for c in chunks)
        assert ran == {"phrase_lane_kernel" if rows <= PC.LANE_ROWS * len(chunks) else "phrase_kernel"}, (ran, rows, len(chunks))
    return got


def check_phrase_split(lib, name):
    """Three streams pushed in chunks of 1, 1, 2, 3, w - 1, w, w + 1, 1, 1, 257 and 300 rows: every push is the whole scan's rows."""
    r = PC.PHRASE_ROW[name]
    sizes, S = PC.split_sizes(r.w), 3
    starts = np.concatenate([[0], np.cumsum(sizes)])
    streams = PC.phrase_streams(name, S, int(starts[-1]))
    fired = 0
    for ordered, combine in PC.MODES:
        want = [TPS.whole(rows, r.phrases, r.w, ordered, combine) for rows in streams]
        fired += sum(int(x[3].sum()) for x in want)
        st = TPS.Carried(lib, S, r.C, r.phrases, r.w, ordered, combine)
        for at, m in zip(starts, sizes):
            got = pushed(st, lib, [rows[at:at + m] for rows in streams])
            for s in range(S):
                TPS.same4(got[s], want[s], at, (name, ordered, combine, s))
    assert fired >= 4 * len(PC.MODES)


@pytest.mark.parametrize("name", PC.STREAM_ROWS)
def test_phrase_split_equals_the_whole(emu_lib, name):
    check_phrase_split(emu_lib, name)


def check_phrase_single_rows(lib, name, S):
    """One-row pushes, the lane kernel with the ring wrapping twice.  word_counts at 65 streams: two workgroups, word counts 4 .. 8
    through the run form; p64 at 16 streams: 16 phrases of two word counts a wave, a phrase count that is a multiple of four."""
    r = PC.PHRASE_ROW[name]
    n = 2 * (r.w - 1) + 6
    streams = PC.phrase_streams(name, S, n, seed=1)
    P = len(r.phrases)
    for ordered, combine in PC.MODES:
        want = [TPS.whole(rows, r.phrases, r.w, ordered, combine) for rows in streams]
        heard = (np.concatenate([x[0] for x in want])[:, :P] > 0.25).any(axis=0)                # (phrases spoken in the streams in turn)
        assert heard.all() if S >= P else heard.sum() >= S
        st = TPS.Carried(lib, S, r.C, r.phrases, r.w, ordered, combine)
        for i in range(n):
            got = pushed(st, lib, [rows[i:i + 1] for rows in streams])
            for s in range(S):
                TPS.same4(got[s], want[s], i, (name, ordered, combine, s))


SINGLE_ROWS = [("word_counts", 65), ("p64", 16)]


@pytest.mark.parametrize("name,S", SINGLE_ROWS)
def test_phrase_single_row_pushes(emu_lib, name, S):
    check_phrase_single_rows(emu_lib, name, S)


def check_phrase_ragged(lib, name="p63_c46"):
    """Five streams advance by different amounts a call -- both kernels' ragged instances -- and stream 2 sits call 1 out."""
    r = PC.PHRASE_ROW[name]
    calls = [[1, 2, 0, 3, 1], [r.w, 300, 0, 2, r.w - 1], [0, 1, 4, 1, 2], [3, 3, 3, 3, 3], [r.w + 1, 0, 257, 1, 5]]
    S, total = 5, np.sum(calls, axis=0)
    streams = PC.phrase_streams(name, S, int(total.max()), seed=2)
    for ordered, combine in PC.MODES:
        want = [TPS.whole(streams[s][:total[s]], r.phrases, r.w, ordered, combine) for s in range(S)]
        st = TPS.Carried(lib, S, r.C, r.phrases, r.w, ordered, combine)
        at = [0] * S
        for j, m in enumerate(calls):
            before = st.state.clone()
            got = pushed(st, lib, [streams[s][at[s]:at[s] + m[s]] for s in range(S)], ragged=True)
            for s in range(S):
                if m[s] == 0:                               # the stream's integers and ring columns stay byte for byte
                    ints = lambda t: t[:5 * S].view(torch.int32).view(5, S)[:, s]
                    slots = lambda t: t[64:].view(torch.int32).view(r.w - 1, r.U, S)[:, :, s]
                    assert torch.equal(ints(st.state), ints(before)) and torch.equal(slots(st.state), slots(before)), (j, s)
                TPS.same4(got[s], want[s], at[s], (name, ordered, combine, j, s))
                at[s] += m[s]


def test_phrase_ragged_pushes(emu_lib):
    check_phrase_ragged(emu_lib)


# ---- 4. template scores, whole scans ---------------------------------------------------------------------------------------------------
def check_template_row(lib, F):
    """Ragged (every pointer one float off 16-byte alignment) and dense, without and with a step limit, lengths asked for and not."""
    x = PC.template_inputs(F)
    off_by_one, aligned = Call(lib, shift=1), Call(lib)
    N, steps = x.cube.shape[:2]
    for max_steps in (0, x.limit):
        want, wlen, dwant, dlen = PC.template_reference(F, max_steps)
        _, got, glen = off_by_one(x.packed, x.tm, x.kw_off, x.scale, max_steps, offsets=x.off)
        same(got, want, ("ragged", F, max_steps))
        same(glen, wlen, ("ragged lengths", F, max_steps))
        _, got, glen = aligned(x.cube, x.tm, x.kw_off, x.scale, max_steps)
        same(got.reshape(N * steps, -1), dwant, ("dense", F, max_steps))
        same(glen.reshape(N * steps, -1), dlen, ("dense lengths", F, max_steps))
    _, got, glen = aligned(x.packed, x.tm, x.kw_off, x.scale, x.limit, offsets=x.off, want_lengths=False)
    same(got, want, ("no lengths", F))
    assert (glen == int(TTS.MARK)).all()


@pytest.mark.parametrize("F", PC.FEATURES)
def test_template_scores_equal_definition(emu_lib, F):
    check_template_row(emu_lib, F)


def check_table_limits(lib, F, table):
    tm, scale, packed, off = PC.limit_inputs(F)
    kw_off = PC.LIMIT_TABLES[table]
    K = len(kw_off) - 1
    call = Call(lib, shift=1)
    for max_steps in (0, 6):
        want, wlen = DR.scores(packed, off, tm, kw_off, scale, max_steps)
        _, got, glen = call(packed, tm, kw_off, scale, max_steps, offsets=off)
        same(got, want, (table, F, max_steps))
        same(glen, wlen, (table, "lengths", F, max_steps))
    # on the reference: many keywords are heard; the one keyword of 64 templates is won by templates of several lengths
    assert got.shape[1] == K + 1 and (want[:, :K] == 1.0).any(axis=0).sum() >= min(K, 10)
    assert K > 1 or len(set(wlen[want[:, 0] == 1.0, 0].tolist())) >= 4


@pytest.mark.parametrize("table", list(PC.LIMIT_TABLES))
@pytest.mark.parametrize("F", PC.LIMIT_FEATURES)
def test_template_table_limits(emu_lib, F, table):
    check_table_limits(emu_lib, F, table)


def tie_case(F=35, L=6):
    """Two signals that hold the piece X: in the first it ends on a tile's last row, in the second on a tile's first."""
    rng = np.random.RandomState(61)
    tr = PC.tile_rows(F)
    X = walk_rows(rng, L, F)
    ends = [tr - 1, 2 * tr]
    sigs = [planted(rng, 2 * tr + 5, F, []) for _ in ends]
    for v, e in zip(sigs, ends):
        v[e - L + 1:e + 1] = X
    return X, np.concatenate(sigs), np.array([0, 2 * tr + 5, 4 * tr + 10], np.int64), [ends[0], 2 * tr + 5 + ends[1]]


def check_exact_tie(lib):
    """A keyword's templates X and X[1:] both cost exactly 0 where X ends: both score 1, over L and L - 1 steps.  The first of the
    two in the table wins -- a later template replaces only what is strictly less."""
    F, L = 35, 6
    X, packed, off, at = tie_case(F, L)
    sc = [np.float32(0.5 / L)] * 2
    call = Call(lib)
    for tm, carried in (([X, X[1:]], L), ([X[1:], X], L - 1)):
        want, wlen = DR.scores(packed, off, tm, [0, 2], sc)
        for q in range(2):                                  # on the reference: both templates tie at those rows, at different lengths
            alone, alen = DR.scores(packed, off, [tm[q]], [0, 1], sc[:1])
            assert (alone[at, 0] == 1.0).all() and (alen[at, 0] == len(tm[q])).all()
        assert (want[at, 0] == 1.0).all() and (wlen[at, 0] == carried).all()
        _, got, glen = call(packed, tm, [0, 2], sc, offsets=off)
        same(got, want, ("tie", carried))
        same(glen, wlen, ("tie lengths", carried))
        assert (glen[at, 0] == carried).all()


def test_exact_tie_keeps_the_first_template(emu_lib):
    check_exact_tie(emu_lib)


# ---- 5. template streaming -------------------------------------------------------------------------------------------------------------
def check_template_streams(lib, F, max_steps=0):
    """Three streams in chunks of 1, 1, tr - 1, tr, tr + 1, 2, 2 tr + 3 and 1 rows, then a ragged call that stream 1 sits out (its state
    stays byte for byte), a reset of stream 0, and a last ragged call: all five outputs are the whole scan's since the reset."""
    tm, kw_off, scale = PC.stream_templates(F)
    tr, S = PC.tile_rows(F), 3
    calls = [[m] * S for m in PC.stream_chunks(F)] + [[tr + 2, 0, 3], [4] * S, [1, tr + 1, 2]]
    idle_call, reset_call = len(calls) - 3, len(calls) - 2
    total = np.sum(calls, axis=0)
    rng = np.random.RandomState(300 + F)
    pieces = [(PC.zero_cost(tm[q], rate), gap) for q, rate, gap in ((1, 1, 1), (2, 2, 0), (3, 2, 2), (1, 0.5, 0), (2, 1, 1), (0, 1, 0), (1, 1, 0))]
    streams = [planted(rng, int(total[s]), F, pieces[s:] + pieces[:s]) for s in range(S)]
    st = TTS.Carried(lib, S, F, tm, kw_off, scale, max_steps)
    at, since, fired = [0] * S, [0] * S, 0
    for j, m in enumerate(calls):
        reset = None
        if j == reset_call:
            reset, since[0] = np.array([1, 0, 0], np.uint8), at[0]
        before = st.stream_state(1) if j == idle_call else None
        got = st.push([streams[s][at[s]:at[s] + m[s]] for s in range(S)], reset=reset)
        if j == idle_call:
            assert np.array_equal(st.stream_state(1), before)
        for s in range(S):
            if m[s]:
                want = TTS.whole(streams[s][since[s]:at[s] + m[s]], tm, kw_off, scale, max_steps)
                TTS.same5(got[s], want, at[s] - since[s], ("streams", F, j, s))
                fired += int(got[s][4].sum())
            at[s] += m[s]
    assert fired >= 3 and since[0] > 0


@pytest.mark.parametrize("F", PC.STREAM_FEATURES)
def test_template_streams_equal_the_whole(emu_lib, F):
    check_template_streams(emu_lib, F, max_steps=0 if F != 35 else 90)


def check_length_clamp(lib, max_steps):
    """A carried column whose lengths stand at INT32_MAX - 2, - 1 and INT32_MAX, written into a fresh state by the header's layout: the
    path stays in the last frame (the rows equal it), so every step adds one to a length that is full -- the output stays at
    INT32_MAX, as `min(n, INT32_MAX - 1) + 1` says."""
    F, L = 12, 3
    rng = np.random.RandomState(8)
    tm = [walk_rows(rng, L, F)]
    scale = np.array([np.float32(0.5 / L)], np.float32)
    st = TTS.Carried(lib, 1, F, tm, [0, 1], scale, max_steps)
    D = np.array([0.003, 0.002, 0.001], np.float32)
    n = np.array([INT32_MAX - 2, INT32_MAX - 1, INT32_MAX], np.int32)
    ints = 256 // 4
    assert st.state.numel() == ints + 2 * L
    st.state[ints:ints + L] = torch.from_numpy(D).to(st.dev)
    st.state.view(torch.int32)[ints + L:] = torch.from_numpy(n).to(st.dev)
    assert st.stream_state(0)[5:].tobytes() == D.tobytes() + n.tobytes()        # (read back the way the header lays it out)
    v = np.repeat(tm[0][L - 1:], 3, axis=0)
    cost, length, (D1, n1) = DR.walk(tm[0], v, state=(D.copy(), n.copy()))
    assert length.tolist() == [INT32_MAX] * 3 and (cost == D[2]).all()           # an unclamped sum would have left int32
    conf = DR.conf_of(cost, length, scale[0], max_steps)
    post = np.stack([conf, np.float32(1.0) - conf], axis=1).astype(np.float32)
    assert (conf == 0.0).all() if max_steps else (conf > 0.99).all()
    want = (post, length[:, None], *PR.detect_rule(post, TTS.SUPP, TTS.THR))
    TTS.same5(st.push([v])[0], want, 0, ("clamp", max_steps))
    assert st.stream_state(0)[5:].tobytes() == D1.tobytes() + n1.tobytes()      # and the column it leaves behind


@pytest.mark.parametrize("max_steps", [0, 1000])
def test_length_clamp(emu_lib, max_steps):
    check_length_clamp(emu_lib, max_steps)


# ---- 6. the Python layer on a network of other than 12 labels ----------------------------------------------------------------------------
def check_python_layer(lib):
    """A scanner of a 46-label TCResNet8 (width 0.3, one coefficient): `enroll` caps a template at tcr_dtw_frames_max(46) = 89 frames,
    not at 256; `PhraseDetector` and `TemplateDetector` posteriors are bitwise the C entries' on the scan's rows."""
    Sc = scanning()
    fe = Cm.make_frontend(lib, 640, 320, num_mfccs=1)
    arch = Cm.make_arch("TCResNet8", 0.3, in_channels=1, num_classes=46)
    p, s = R.init_params(arch, 3)
    R.randomize_bn(arch, p, s, 4)
    net = Cm.make_net(lib, "TCResNet8", 0.3, fe.n_frames, p, s, in_channels=1, num_classes=46)
    scanner = Sc.KeywordScanner(net, fe, frames_per_step=2, **DET)
    assert scanner.net.num_classes == 46 and lib.tcr_dtw_frames_max(46) == PC.frames_max(46) == 89
    n = 100
    audio = segment_audio(1, n * scanner.step_samples, 47)
    kt = Sc.KeywordTemplates()
    t = kt.enroll(scanner, "long", audio[0])
    scan = scanner.scan(Cm.to_dev(lib, audio))
    sm = scan.smoothed.cpu().numpy()[0]
    assert sm.shape == (n, 46)
    same(t, sm[::2], "every second row: 50 frames")
    kt.add("cut", sm[30:41])
    td = Sc.TemplateDetector(scanner, kt, max_stretch=0)
    flat, kw_off = [t, sm[30:41]], [0, 1, 2]
    scale = [np.float32(0.5 / len(x)) for x in flat]
    post, lengths = td.scores(scan, return_lengths=True)
    _, want, wlen = Call(lib)(sm[None], flat, kw_off, scale)
    same(post.cpu().numpy(), want, "template posteriors")
    same(lengths.cpu().numpy(), wlen, "template lengths")
    same(want[0], DR.scores(sm, [0, n], flat, kw_off, scale)[0], "the definition")
    assert want[0, 40, 1] == 1.0 and wlen[0, 40, 1] == 11
    order = [int(c) for c in np.argsort(-sm.mean(axis=0))[:5]]
    words = [order[:4], order[::-1], order[1:3]]
    ph = Sc.PhraseDetector(scanner, words, window_ms=12 * scanner.step_ms)
    assert ph.window_steps == 12
    got = ph.scores(scan).cpu().numpy()
    same(got, lib_scores(lib, sm[None], words, 12, 1, PC.PRODUCT)[1], "phrase posteriors")
    same(got[0], PR.scores(sm, [0, n], words, 12, 1, PC.PRODUCT), "the definition")


def test_python_layer_on_a_46_label_net(emu_lib):
    check_python_layer(emu_lib)


# ---- MI355X ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", PC.PHRASE_IDS)
def test_gpu_phrase_scores_equal_definition(hip_lib, name):
    check_phrase_row(hip_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PC.STREAM_ROWS)
def test_gpu_phrase_split_equals_the_whole(hip_lib, name):
    check_phrase_split(hip_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,S", SINGLE_ROWS)
def test_gpu_phrase_single_row_pushes(hip_lib, name, S):
    check_phrase_single_rows(hip_lib, name, S)


@pytest.mark.gpu
def test_gpu_phrase_ragged_pushes(hip_lib):
    check_phrase_ragged(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("F", PC.FEATURES)
def test_gpu_template_scores_equal_definition(hip_lib, F):
    check_template_row(hip_lib, F)


@pytest.mark.gpu
@pytest.mark.parametrize("table", list(PC.LIMIT_TABLES))
@pytest.mark.parametrize("F", PC.LIMIT_FEATURES)
def test_gpu_template_table_limits(hip_lib, F, table):
    check_table_limits(hip_lib, F, table)


@pytest.mark.gpu
def test_gpu_exact_tie_keeps_the_first_template(hip_lib):
    check_exact_tie(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("F", PC.STREAM_FEATURES)
def test_gpu_template_streams_equal_the_whole(hip_lib, F):
    check_template_streams(hip_lib, F, max_steps=0 if F != 35 else 90)


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [0, 1000])
def test_gpu_length_clamp(hip_lib, max_steps):
    check_length_clamp(hip_lib, max_steps)


@pytest.mark.gpu
def test_gpu_python_layer_on_a_46_label_net(hip_lib):
    check_python_layer(hip_lib)
