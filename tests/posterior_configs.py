"""Phrase and template configurations for tests/test_posterior_configs.py: the (classes, phrase table, window) and (features, template
table) points from which csrc/phrase.hip and csrc/dtw.hip derive their kernel instances, LDS sizes and tile shapes, one row per
case, and the inputs the tests run them on.

phrase.hip, restated from the host code:  U = the distinct word classes of the table;  stride = TILE + w - 1 staged rows a column;
dynamic LDS = 4 stride U bytes, at most 65536 (w <= tcr_phrase_window_max(U) = 16384 // U - 255; above 32768 the launcher raises the
kernel's limit first);  one unrolled instance per word count 1 .. 8, order and combiner, once staged (phrase_kernel) and once over
runs of rows (phrase_lane_kernel, which a push of at most 4 rows a stream on average takes);  the lane kernel deals phrase q to wave
q % 4.

dtw.hip:  Lm = tcr_dtw_frames_max(F) = min(256, 4096 // F) frames a template at most;  a tile of signal rows is tr = min(1024 // F, 64)
rows, lane r folds row r;  a template of L frames runs the instance of ceil(L / 64) frames a lane (1 .. 4);  dynamic LDS = 4 x 64 F x
the call's largest frames-per-lane bytes.

A row states the geometry it is there for (U, LDS bytes; Lm, tr) and `test_rows_hold_the_listed_cases` asserts it against the
restatement above, so that an edited row cannot drift away from the case it claims."""
import functools
from collections import namedtuple

import numpy as np

from tests import dtw_ref as DR
from tests import phrase_ref as PR
from tests.test_phrases import planted_rows
from tests.test_templates import planted, walk_rows

TILE, LDS_FLOATS, LANE_ROWS = 256, 16384, 4
PRODUCT, MIN = PR.PRODUCT, PR.MIN
MODES = [(1, PRODUCT), (1, MIN), (0, PRODUCT), (0, MIN)]            # (ordered, combine)


def window_max(U):
    """include/tcresnet_hip.h: tcr_phrase_window_max."""
    return LDS_FLOATS // U - (TILE - 1) if U >= 1 else 0


def distinct(phrases):
    return len({c for q in phrases for c in q})


def phrase_lds(phrases, w):
    """The dynamic LDS bytes phrase_kernel is launched with."""
    return 4 * (TILE + w - 1) * distinct(phrases)


# ---- the phrase rows -------------------------------------------------------------------------------------------------------------------
# lengths: the ragged signals' rows; dense: the (N, steps) cube; U, lds: the geometry the row is there for
PhraseRow = namedtuple("PhraseRow", "name C phrases w lengths dense U lds")

WORD_COUNTS = [[1, 2, 3, 4], [4, 3, 2, 1, 5], [5, 6, 6, 7, 8, 9], [2, 4, 6, 8, 10, 11, 3], [9, 8, 7, 6, 5, 4, 3, 2], [3]]   # [0] is the reverse of [1]'s prefix
P64 = [[(5 * q + q // 8 + 7 * m) % 12 for m in range(1 + q % 8)] for q in range(64)]
P63_C46 = [[(5 * q + 11 * m) % 46 for m in range(1 + q % 8)] for q in range(63)]
U35 = [[(8 * q + m) % 35 for m in range(8)] for q in range(5)]
U64 = [list(range(8 * q, 8 * q + 8)) for q in range(8)]
FULL = [[1, 2, 3, 4], [4, 3], [2]]

PHRASE_ROWS = [
    PhraseRow("word_counts",   12, WORD_COUNTS,      9,               [0, 1, 8, 9, 10, 256, 257, 300],      (2, 261), 11, 11616),
    PhraseRow("p64",           12, P64,              7,               [0, 1, 6, 7, 8, 257, 300, 300, 256],  (2, 261), 12, 12576),
    PhraseRow("p63_c46",       46, P63_C46,          40,              [0, 1, 39, 40, 41, 257, 300, 300],    (2, 261), 46, 54280),
    PhraseRow("u35_wmax",      35, U35,              window_max(35),  [0, 1, 212, 213, 214, 600],           (2, 230), 35, 65520),
    PhraseRow("u64_w1",        70, U64,              1,               [0, 1, 2, 257, 300],                  (2, 261), 64, 65536),
    PhraseRow("lds_64k_short", 3,  [[1, 2], [2, 1]], window_max(2),   [300, 10],                            (2, 40),  2,  65536),
    PhraseRow("lds_64k_full",  12, FULL,             window_max(4),   [4200, 10],                           (2, 10),  4,  65536),
]
PHRASE_ROW = {r.name: r for r in PHRASE_ROWS}
PHRASE_IDS = [r.name for r in PHRASE_ROWS]
STREAM_ROWS = ["word_counts", "p63_c46", "u35_wmax"]
GUARD_CUT = 700                 # the discrimination guards read a signal's first rows only (lds_64k_full: its plants lie there)


def utterance(v, at, words, w):
    """Writes one utterance of a phrase into rows `at` .. of v: min(n, w) rows, the words spread over them in order (more words than the
    window has rows: neighbours share a row), word m at 0.99 - 0.01 m -- the last word is the weakest, so dropping it changes the
    product and the minimum alike -- and everything else in those rows at 0.01.  (Rows that hold two words are no distribution; every
    value stays in [0, 1].)  -> the rows written."""
    n = len(words)
    rows = min(n, w)
    v[at:at + rows] = np.float32(0.01)
    for m, c in enumerate(words):
        v[at + m * rows // n, c] = np.float32(0.99 - 0.01 * m)
    return rows


def spoken(rng, lengths, C, phrases, w, gap=2, strict=True):
    """`planted_rows` signals of the given lengths with every phrase spoken once: each utterance goes into the longest signal that
    still has room for it (a signal of more than a tile and 40 rows starts 20 rows in front of its first tile boundary, so utterances
    cross it), `gap` background rows between two.  strict: every phrase must find room."""
    sigs = [planted_rows(rng, m, C) if m else np.zeros((0, C), np.float32) for m in lengths]
    order = sorted(range(len(lengths)), key=lambda s: -lengths[s])
    at = {s: TILE - 20 if lengths[s] >= TILE + 40 else 2 for s in order}
    for words in phrases:
        rows = min(len(words), w)
        s = next((s for s in order if at[s] + rows <= lengths[s]), None)
        assert s is not None or not strict, ("no room for", words)
        if s is None:
            continue
        at[s] += utterance(sigs[s], at[s], words, w) + gap
    return sigs


PhraseInputs = namedtuple("PhraseInputs", "packed off cube doff")


@functools.lru_cache(maxsize=None)
def phrase_inputs(name):
    """The row's inputs: packed ragged rows with their offsets, and the dense cube with its."""
    r = PHRASE_ROW[name]
    rng = np.random.RandomState(4000 + PHRASE_IDS.index(name))
    sigs = spoken(rng, r.lengths, r.C, r.phrases, r.w)
    off = np.concatenate([[0], np.cumsum(r.lengths)]).astype(np.int64)
    N, steps = r.dense
    cube = np.stack(spoken(rng, [steps] * N, r.C, r.phrases, r.w, strict=False))
    return PhraseInputs(np.concatenate(sigs), off, cube, np.arange(N + 1, dtype=np.int64) * steps)


@functools.lru_cache(maxsize=None)
def phrase_reference(name, ordered, combine):
    """(ragged, dense) of tests/phrase_ref.py (`scores_dp_fast` per signal), computed once per process and left unchanged."""
    r, x = PHRASE_ROW[name], phrase_inputs(name)
    N, steps = r.dense
    want = PR.scores(x.packed, x.off, r.phrases, r.w, ordered, combine)
    dwant = PR.scores(x.cube.reshape(N * steps, r.C), x.doff, r.phrases, r.w, ordered, combine)
    want.setflags(write=False)
    dwant.setflags(write=False)
    return want, dwant


@functools.lru_cache(maxsize=None)
def phrase_streams(name, n_streams, n_rows, seed=0):
    """Streams of n_rows rows for the row's table, every phrase spoken in the streams in turn (as far as a stream has room)."""
    r = PHRASE_ROW[name]
    rng = np.random.RandomState(4100 + 10 * PHRASE_IDS.index(name) + seed)
    streams = [planted_rows(rng, n_rows, r.C) for _ in range(n_streams)]
    at = [1 + s % 3 for s in range(n_streams)]
    for turn in range(max(1, -(-n_streams // len(r.phrases)))):
        for q, words in enumerate(r.phrases):
            s = (q + turn * len(r.phrases)) % n_streams
            if at[s] + min(len(words), r.w) <= n_rows:
                at[s] += utterance(streams[s], at[s], words, r.w) + 1
    return streams


def split_sizes(w):
    """Rows a push of the phrase split cases: history shorter than w - 1, exactly w - 1, the ring wrapping, more than a tile."""
    return [m for m in (1, 1, 2, 3, w - 1, w, w + 1, 1, 1, 257, 300) if m > 0]


# ---- the template rows -----------------------------------------------------------------------------------------------------------------
FEATURES = [1, 2, 16, 17, 35, 40, 63, 64]
STREAM_FEATURES = [17, 35, 64]
LIMIT_FEATURES = [12, 35]
TemplateGeom = namedtuple("TemplateGeom", "F Lm tr")
TEMPLATE_GEOM = [TemplateGeom(1, 256, 64), TemplateGeom(2, 256, 64), TemplateGeom(16, 256, 64), TemplateGeom(17, 240, 60),
                 TemplateGeom(35, 117, 29), TemplateGeom(40, 102, 25), TemplateGeom(63, 65, 16), TemplateGeom(64, 64, 16),
                 TemplateGeom(12, 256, 64)]
GEOM = {g.F: g for g in TEMPLATE_GEOM}


def frames_max(F):
    """include/tcresnet_hip.h: tcr_dtw_frames_max."""
    return min(256, 4096 // F) if 1 <= F <= 64 else 0


def tile_rows(F):
    return min(1024 // F, 64)


def fpl(L):
    """Frames a lane owns for a template of L frames: the instance dtw_kernel runs."""
    return -(-L // 64)


def dtw_lds(tm, F):
    return 4 * 64 * F * max(fpl(len(t)) for t in tm)


def template_lengths(F):
    Lm = frames_max(F)
    out = []
    for L in (1, 2, 3, min(63, Lm), min(64, Lm), min(65, Lm), min(129, Lm), Lm - 1, Lm):
        if L not in out:
            out.append(L)
    return out


def signal_lengths(F):
    tr, Lm = tile_rows(F), frames_max(F)
    return [0, tr - 1, tr, tr + 1, 2 * tr, 2 * tr + 1, 3 * tr + 5, 1, 0, Lm + 7]


def zero_cost(t, rate):
    """Rows on which the template t has a path of cost exactly 0 that ends at the last of them: rate 1 the template itself (the
    diagonal), rate 2 every other frame up to the last (skips; an even template starts in frame 1), rate 0.5 every frame twice."""
    if rate == 2:
        return t[(len(t) - 1) % 2::2]
    return np.repeat(t, 2, axis=0) if rate == 0.5 else t


def place(lengths, tm):
    """Which pieces the signals hold, back to back: per signal a list of (template, rate).  Every template is there once at a rate of
    cost 0 -- the longest as it is (it fits the last signal only), the others in the tightest signal that takes them, as they are or,
    failing that, at rate 2 -- and whatever room is left takes further pieces at rates 2, 1 and 0.5."""
    def attempt(all_at_2):
        room, plan = list(lengths), [[] for _ in lengths]

        def put(q, rates, tightest=True):
            for rate in rates:
                rows = len(zero_cost(tm[q], rate))
                fits = [s for s in range(len(room)) if room[s] >= rows]
                if fits:
                    s = (min if tightest else max)(fits, key=lambda s: room[s])
                    room[s] -= rows
                    plan[s].append((q, rate))
                    return True
            return False
        by_size = sorted(range(len(tm)), key=lambda q: -len(tm[q]))
        for i, q in enumerate(by_size):
            if not put(q, (1,) if i == 0 else (2,) if all_at_2 else (1, 2)):
                return None
        for rate in (2, 1, 0.5):
            for q in by_size[1:]:
                put(q, (rate,), tightest=False)
        return plan
    plan = attempt(False) or attempt(True)
    assert plan is not None, "the templates do not fit the signals"
    return plan


TemplateInputs = namedtuple("TemplateInputs", "tm kw_off scale packed off cube plan limit")


@functools.lru_cache(maxsize=None)
def template_inputs(F):
    """Templates (`walk_rows`) of `template_lengths(F)` frames -- the first two one keyword, the rest a keyword each -- the ragged
    signals of `signal_lengths(F)` rows with the pieces of `place` back to back, a dense cube [3, 2 tr + 3, F] and the positive step
    limit.  (One feature: softmax rows of one class are all 1, so the rows are column 0 of two-class ones.)"""
    W = max(F, 2)
    rng = np.random.RandomState(7000 + F)
    wide = [walk_rows(rng, L, W) for L in template_lengths(F)]
    lengths = signal_lengths(F)
    plan = place(lengths, wide)
    sigs = [planted(rng, m, W, [(zero_cost(wide[q], rate), 0) for q, rate in pieces]) for m, pieces in zip(lengths, plan)]
    steps = 2 * tile_rows(F) + 3
    cube = np.stack([planted(rng, steps, W, [(zero_cost(wide[q], rate), gap) for q, rate, gap in pieces])
                     for pieces in ([(2, 1, 0), (3, 2, 1), (1, 1, 0)], [(4, 2, 0), (2, 0.5, 2), (0, 1, 0)], [(len(wide) - 1, 2, 0), (1, 1, 0)])])
    tm = [np.ascontiguousarray(t[:, :F]) for t in wide]
    kw_off = np.array([0, *range(2, len(tm) + 1)], np.int32)
    scale = np.array([np.float32(0.5 / len(t)) for t in tm], np.float32)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return TemplateInputs(tm, kw_off, scale, np.ascontiguousarray(np.concatenate(sigs)[:, :F]), off, np.ascontiguousarray(cube[..., :F]), plan,
                          max(2, frames_max(F) // 2))


@functools.lru_cache(maxsize=None)
def template_reference(F, max_steps):
    """(ragged out, ragged lengths, dense out, dense lengths) of tests/dtw_ref.py, once per process."""
    x = template_inputs(F)
    N, steps = x.cube.shape[:2]
    doff = np.arange(N + 1, dtype=np.int64) * steps
    return (*DR.scores(x.packed, x.off, x.tm, x.kw_off, x.scale, max_steps),
            *DR.scores(x.cube.reshape(N * steps, F), doff, x.tm, x.kw_off, x.scale, max_steps))


LIMIT_LENGTHS = [0, 70, 1, 130]


@functools.lru_cache(maxsize=None)
def limit_inputs(F):
    """64 templates of 1 .. 8 frames (template q: 1 + q % 8) and signals that hold every third of them back to back."""
    rng = np.random.RandomState(7100 + F)
    tm = [walk_rows(rng, 1 + q % 8, F) for q in range(64)]
    pieces = [(tm[q], q % 2) for q in range(7, 64, 3)]
    sigs = [planted(rng, m, F, pieces[i:]) for i, m in enumerate(LIMIT_LENGTHS)]
    scale = np.array([np.float32(0.5 / len(t)) for t in tm], np.float32)
    return tm, scale, np.concatenate(sigs), np.concatenate([[0], np.cumsum(LIMIT_LENGTHS)]).astype(np.int64)


LIMIT_TABLES = {"q64_k64": np.arange(65, dtype=np.int32), "q64_k1": np.array([0, 64], np.int32)}


def stream_templates(F):
    """Templates of 1, 3, min(65, Lm) and Lm frames; the middle keyword has two."""
    rng = np.random.RandomState(7200 + F)
    Lm = frames_max(F)
    tm = [walk_rows(rng, L, F) for L in (1, 3, min(65, Lm), Lm)]
    return tm, np.array([0, 1, 3, 4], np.int32), np.array([np.float32(0.5 / len(t)) for t in tm], np.float32)


def stream_chunks(F):
    tr = tile_rows(F)
    return [1, 1, tr - 1, tr, tr + 1, 2, 2 * tr + 3, 1]
