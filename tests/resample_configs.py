"""Resampler configurations for tests/test_resample_configs.py: the (up L, down M, taps P) triples from which tcr_resample
(csrc/resample.hip) derives a workgroup's tile, one row per branch of that arithmetic.

The tile, restated from the host code:  pitch = P | 1;  G = min(L, 32, 6144 // pitch) table rows per workgroup (G = 0: refused, a row
does not fit);  rows_span = ceil(G M / L) + 1;  P + rows_span > 14336: refused, one q of a row group does not fit the staged span;
b_fit = (14336 - P - rows_span) // M + 1;  B = min(b_fit, max(1, 1024 // G)) values of q per workgroup, rounded down to a multiple of
four when above 4;  ceil(L / G) row groups, the last of L - (groups - 1) G rows;  span_cap = (B - 1) M + rows_span + P rounded up to
four;  LDS bytes = 4 (G pitch + span_cap + 64).  A row states its (G, B, groups, last, lds) and the class it is there for; the test
asserts both against `geometry` and `CLASSES`, and a real pair's (L, M, P) against design_table, so that an edited row cannot drift
away from the branch it claims."""
from collections import namedtuple

MAX_ROWS, TABLE_FLOATS, SPAN_FLOATS, TILE_OUTPUTS = 32, 6144, 14336, 1024
MAX_LDS = 4 * (TABLE_FLOATS + SPAN_FLOATS + 2 * MAX_ROWS)                # 82176 B = 80.25 KB: what the file's header states

Geometry = namedtuple("Geometry", "G B groups last lds b_fit b_aim")
# pair: (in_rate, out_rate, zero_crossings) where the triple is a real conversion, else None; n_out: the outputs the tests convert
Config = namedtuple("Config", "name cls L M P pair G B groups last lds n_out")

TAPS_REFUSED, SPAN_REFUSED = "taps", "span"


def geometry(L, M, P):
    """Geometry of an accepted triple; TAPS_REFUSED / SPAN_REFUSED for what tcr_resample refuses by size."""
    pitch = P | 1
    G = min(L, MAX_ROWS, TABLE_FLOATS // pitch)
    if G < 1:
        return TAPS_REFUSED
    rows_span = -(-G * M // L) + 1
    if P + rows_span > SPAN_FLOATS:
        return SPAN_REFUSED
    b_fit = (SPAN_FLOATS - P - rows_span) // M + 1
    b_aim = max(1, TILE_OUTPUTS // G)
    B = min(b_fit, b_aim)
    if B > 4:
        B &= ~3
    groups = -(-L // G)
    span_cap = ((B - 1) * M + rows_span + P + 3) // 4 * 4
    return Geometry(G, B, groups, L - (groups - 1) * G, 4 * (G * pitch + span_cap + 2 * MAX_ROWS), b_fit, b_aim)


SHORT, TABLE, BOUNDARY, SMALL_B, MANY, DEGENERATE = "short_last_group", "table_limited_G", "table_boundary", "small_or_rounded_B", "many_whole_groups", "degenerate_filter"


def _uncut(L, P):
    return min(L, MAX_ROWS) <= TABLE_FLOATS // (P | 1)


# class -> what (row, its Geometry) must satisfy to be in it
CLASSES = {
    SHORT: lambda r, g: g.groups > 1 and g.last < g.G,                                       # G = L - r0 < a.G in the kernel
    TABLE: lambda r, g: r.L > 1 and not _uncut(r.L, r.P) and g.G == TABLE_FLOATS // (r.P | 1),    # the table budget decides G
    BOUNDARY: lambda r, g: _uncut(r.L, r.P) and not _uncut(r.L, r.P + 2),                    # the last P whose G the budget leaves alone
    SMALL_B: lambda r, g: g.B <= 4 or g.B != min(g.b_fit, g.b_aim),                          # Bq = 1 (the b >= B mask), or B cut by &= ~3
    MANY: lambda r, g: g.groups >= 20 and g.last == g.G,
    DEGENERATE: lambda r, g: r.P <= 2 or r.P == TABLE_FLOATS - 2,                            # lead 0, and the largest P
}

ROWS = [
    # ---- the last row group is short
    Config("16000_44100",       SHORT,      441, 160,   64, (16000, 44100, 32),  32,   32, 14, 25, 28736, 14200),   # n_out > B L = 14112: a second q-tile of 14 groups
    Config("48000_44100",       SHORT,      147, 160,   70, (48000, 44100, 32),  32,   32,  5, 19, 29616, 4800),    # B L = 4704
    Config("raw_33_7_4",        SHORT,       33,   7,    4, None,                32,   32,  2,  1,  1824, 1100),    # a last group of one row; B L = 1056
    Config("44100_8000_z16",    SHORT,       80, 441,  178, (44100, 8000, 16),   32,   32,  3, 16, 79280, 300),     # zero_crossings 16: G back at 32
    # ---- G cut by the 6144-float table budget
    Config("44100_8000",        TABLE,       80, 441,  354, (44100, 8000, 32),   17,   32,  5, 12, 80876, 2600),    # the largest LDS request of a real pair, over 64 KB; B L = 2560
    Config("raw_32_33_192",     TABLE,       32,  33,  192, None,                31,   32,  2,  1, 29180, 300),
    Config("raw_32_33_190",     BOUNDARY,    32,  33,  190, None,                32,   32,  1, 32, 29696, 300),
    Config("raw_64_5_192",      TABLE,       64,   5,  192, None,                31,   32,  3,  2, 25596, 2100),    # B L = 2048
    Config("raw_3_2_2048",      TABLE,        3,   2, 2048, None,                 2,  512,  2,  1, 28952, 1600),    # B L = 1536
    # ---- B in {1, 2, 3, 4}, and B rounded down to whole four-chain units
    Config("raw_1_14333_2",     SMALL_B,      1, 14333,  2, None,                 1,    1,  1,  1, 57612, 3),       # the largest accepted M at L = 1, P = 2
    Config("raw_1_6000_2",      SMALL_B,      1, 6000,   2, None,                 1,    2,  1,  1, 48284, 5),
    Config("raw_1_4700_2",      SMALL_B,      1, 4700,   2, None,                 1,    3,  1,  1, 56684, 7),
    Config("raw_1_3500_4",      SMALL_B,      1, 3500,   4, None,                 1,    4,  1,  1, 56308, 9),
    Config("384000_8000",       SMALL_B,      1,   48, 3072, (384000, 8000, 32),  1,  232,  1,  1, 69396, 480),     # b_fit = 234
    Config("192000_8000",       SMALL_B,      1,   24, 1536, (192000, 8000, 32),  1,  532,  1,  1, 63636, 1100),    # b_fit = 533
    Config("16000_48000",       SMALL_B,      3,    1,   64, (16000, 48000, 32),  3,  340,  1,  3,  2668, 2100),    # 1024 // 3 = 341; B L = 1020
    # ---- many whole groups
    Config("11025_16000",       MANY,       640, 441,   64, (11025, 16000, 32),  32,   32, 20, 32, 63616, 700),
    # ---- degenerate filters
    Config("raw_7_3_1",         DEGENERATE,   7,   3,    1, None,                 7,  144,  1,  7,  2028, 1100),    # lead 0; B L = 1008
    Config("raw_5_1_1",         DEGENERATE,   5,   1,    1, None,                 5,  204,  1,  5,  1108, 1100),    # 1024 // 5 = 204; B L = 1020
    Config("raw_33_32_2",       DEGENERATE,  33,  32,    2, None,                32,   32,  2,  1,  4752, 1100),
    Config("raw_1_1_6142",      DEGENERATE,   1,   1, 6142, None,                 1, 1024,  1,  1, 53500, 300),     # the largest P
]
ROW = {r.name: r for r in ROWS}
ROW_IDS = [r.name for r in ROWS]

# (cause, L, M, P): refused by size.  The span rows all have 14336 - P - rows_span in (-M, 0): a division that truncates toward zero
# turns that into b_fit = 1.
REFUSED = [
    ("taps",   1,       1, 6144),
    ("span",   1,   14334,    2),        # one past the largest accepted M
    ("span",   1,  100000,    2),
    ("span",   2,   40000,    2),
    ("span",  64,   30000,    2),
    ("groups", 65535 * 32 + 1, 1, 2),    # 65536 row groups of 32: one more than a launch covers
]
