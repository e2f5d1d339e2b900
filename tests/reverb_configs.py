"""The configuration table of tests/test_reverb.py: one row is one tcr_reverb call over a small table of clips.  A row states the
classes it is there for (`cls`, derived from its own numbers when it is built, so a statement cannot drift from the row), and
`test_table_reaches_every_class` asserts that the table reaches ALL_CLASSES.  Not a cross product: every class at least once.

T = TCR_REVERB_TILE (outputs per workgroup), D = TCR_REVERB_STAGE (input samples per LDS stage), MAX = TCR_REVERB_TAPS_MAX."""
import numpy as np

import tcresnet_amd as T_

T, D, MAX = T_._lib.REVERB_TILE, T_._lib.REVERB_STAGE, T_._lib.REVERB_TAPS_MAX

CLIP_LENGTHS = {1: "1", 2: "2", 15: "15", 16: "16", 17: "17", T - 1: "T-1", T: "T", T + 1: "T+1", 2 * T + 5: "2T+5"}
TAPS = {1: "1", 2: "2", 3: "3", 4: "4", 5: "5", 16: "16", 17: "17", D - 1: "D-1", D: "D", D + 1: "D+1", 2 * D + 3: "2D+3", MAX: "MAX"}
TAILS = ("0", "full", "mid", "beyond")

ALL_CLASSES = ({f"n:{v}" for v in CLIP_LENGTHS.values()} | {f"L:{v}" for v in TAPS.values()} | {f"tail:{v}" for v in TAILS}
               | {f"{w}:{p}" for w in ("in_off", "ir_off", "out_off") for p in ("odd", "even")}
               | {"fmt:i16", "fmt:f32", "outs:f", "outs:p", "outs:both", "mixed", "rails", "skip:MAX-against-3"})


def outputs(n, L, tail):
    """m of a clip of n samples under L taps: tail "0" keeps n, "full" n + L - 1, "mid" one value in between (n + (L - 1) // 2; L >= 3),
    "beyond" 37 outputs past n + L - 1 (zeros), an int: that many outputs."""
    if isinstance(tail, int):
        return tail
    return {"0": n, "full": n + L - 1, "mid": n + (L - 1) // 2, "beyond": n + L - 1 + 37}[tail]


class Row:
    """clips: [(n, L, tail)]; fmt "i16" | "f32"; outs "f" | "p" | "both"; in_pad / ir_pad: elements in front of the first clip /
    response in their buffers (between two of them: 1 + that); loud: full-scale input under an all-ones response (the rails)."""

    def __init__(self, name, clips, fmt="i16", outs="both", in_pad=0, ir_pad=0, loud=False, seed=0):
        self.name, self.clips, self.fmt, self.outs, self.in_pad, self.ir_pad, self.loud, self.seed = name, clips, fmt, outs, in_pad, ir_pad, loud, seed
        self.n = np.array([c[0] for c in clips], np.int64)
        self.L = np.array([c[1] for c in clips], np.int64)
        self.m = np.array([outputs(*c) for c in clips], np.int64)
        self.in_off = in_pad + np.concatenate([[0], np.cumsum(self.n + 1 + in_pad)[:-1]]).astype(np.int64)
        self.ir_off = ir_pad + np.concatenate([[0], np.cumsum(self.L + 1 + ir_pad)[:-1]]).astype(np.int64)
        self.out_off = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.cls = self._classes()

    def _classes(self):
        c = {f"fmt:{self.fmt}", f"outs:{self.outs}"}
        for (n, L, tail), m, io, ro, oo in zip(self.clips, self.m, self.in_off, self.ir_off, self.out_off[:-1]):
            if n in CLIP_LENGTHS:
                c.add(f"n:{CLIP_LENGTHS[n]}")
            if L in TAPS:
                c.add(f"L:{TAPS[L]}")
            if m > 0 and n > 0:
                if tail in TAILS and (tail != "mid" or n < m < n + L - 1) and (tail != "0" or L > 1):
                    c.add(f"tail:{tail}")
                c |= {f"in_off:{'odd' if io % 2 else 'even'}", f"ir_off:{'odd' if ro % 2 else 'even'}", f"out_off:{'odd' if oo % 2 else 'even'}"}
            if L == MAX and n == 3 and m == n + L - 1:
                c.add("skip:MAX-against-3")
        live = self.m > 0
        if (self.m > 2 * T).any() and (live & (self.m < 64)).sum() >= 20 and (self.n == 0).any() and ((self.n > 0) & (self.m == 0)).any():
            c.add("mixed")
        if self.loud:
            c.add("rails")
        return c

    def total(self):
        return int(self.out_off[-1])


ROWS = [
    Row("one-sample", [(1, 1, "full"), (1, 1, "full")]),
    Row("two-two", [(2, 2, "full"), (2, 2, "0")], outs="f", in_pad=1),
    Row("fifteen-three", [(15, 3, "0"), (15, 3, "mid")], outs="p", ir_pad=1),
    Row("sixteen-four", [(16, 4, "mid"), (16, 4, "full")], fmt="f32", in_pad=3, ir_pad=2),
    Row("seventeen-five", [(17, 5, "beyond"), (17, 5, "full")], fmt="f32", outs="p"),
    Row("tile-minus-one", [(T - 1, 16, "full"), (5, 17, "full")], in_pad=1, ir_pad=1),
    Row("tile", [(T, 17, "0"), (T, 17, "full")], fmt="f32", outs="f"),
    Row("tile-plus-one", [(T + 1, D - 1, "full")], in_pad=2),
    Row("two-tiles-five", [(3, 2, "full"), (2 * T + 5, D, "mid")], ir_pad=3),
    Row("stage-plus-one", [(17, D + 1, "full"), (16, D + 1, "beyond")], fmt="f32"),
    Row("two-stages-three", [(1, 1, 1), (T + 1, 2 * D + 3, "full")], fmt="f32", outs="both", in_pad=1),
    Row("longest-response", [(3, MAX, "full")], in_pad=1, ir_pad=1),
    Row("mixed", [(2 * T + 5, 300, "full")] + [(k, 1 + (7 * k) % 40, "full") for k in range(1, 31)] + [(0, 5, 0), (5, 3, 0), (0, 1, 0)]
        + [(9, 2, "full")], in_pad=1),
    Row("rails", [(600, 64, "full"), (600, 64, "0")], loud=True),
]

# around the tile edges, for the MI355X: 300 clips of T - 2 .. T + 2 outputs (and of 1 .. 3 tiles), short responses
EDGE_ROW = Row("tile-edges", [(T - 20 + (k % 5) + (k % 3) * T, 17 + k % 7, T - 2 + (k % 5) + (k % 3) * T) for k in range(300)], in_pad=1, ir_pad=1)
LONG_ROW = Row("second-against-longest", [(16000, MAX, "full")])
