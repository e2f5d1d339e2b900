"""The table of tests/test_g2d_dw.py: small graphs around the depthwise node of the 2-D graph engine, each row written for classes of the
kernels (csrc/net2d_dw.hip) or of the host code (csrc/net2d.cpp) and stating them.  A row is
    (id, plane height, plane width, batch, graph, classes[, options])
`graph` builds on tests/test_g2d_configs.py's Spec with one more op; `classes` are "kind:value" words that
test_g2d_dw.py::test_rows_hold_the_listed_cases checks against the row's own spec and against the list the table must reach.
Options: nc = classes of the head, T = the forward row tile the row states."""
from tests.test_g2d_configs import Spec

# the geometry of net2d_dw.hip restated (dw2d_plan): the 64-thread instance takes planes that are one tile of at most 256 outputs whose
# gathered rows fit 1024 floats; otherwise 256 threads and tiles of ROW_TILE rows, fewer while the gathered rows exceed 4096 floats
ROW_TILE, LDS_FLOATS, SMALL_OUTPUTS, SMALL_LDS_FLOATS, MAX_TAPS = 32, 4096, 256, 1024, 1024


def src_rows(dgrad, rows, k_eff, stride, sh):
    return min(rows + k_eff - 1 if dgrad else (rows - 1) * stride + k_eff, sh)


def plan(dgrad, h, w, oh, ow, kh, dh, sh):
    """(threads, rows per tile) of the forward (dgrad False: positions on the output plane) or data gradient (on the input plane)."""
    ph, pw, s_h, s_w = (h, w, oh, ow) if dgrad else (oh, ow, h, w)
    k_eff = (kh - 1) * dh + 1
    if ph * pw <= SMALL_OUTPUTS and src_rows(dgrad, ph, k_eff, sh, s_h) * s_w <= SMALL_LDS_FLOATS:
        return 64, ph
    t = ROW_TILE
    while t > 1 and src_rows(dgrad, t, k_eff, sh, s_h) * s_w > LDS_FLOATS:
        t -= 1
    return 256, t


class DwSpec(Spec):
    def dw(self, inp, k, stride=(1, 1), rate=(1, 1), pad="SAME", relu=False, bias=False):
        i = len(self.nodes)
        return self._add(op="dwconv", k=k, stride=stride, rate=rate, pad=pad, relu=relu, w=f"n{i}/depthwise_weights",
                         b=f"n{i}/biases" if bias else None, **{"in": inp})


def graph(fn):
    s = DwSpec()
    logits = fn(s)
    return {"nodes": s.nodes, "logits": logits}


def sep(c, k=(3, 3), nc=12, bn=False, **kw):
    """A dense 3 x 3 stem to `c` channels (ReLU, bias), the depthwise conv under test -- so its data gradient runs and shows in the stem's
    filter gradient -- [a BN with only `center`], the head."""
    def build(s):
        x = s.dw(s.conv(-1, (3, 3), c, relu=True, bias=True), k, **kw)
        if bn:
            x = s.bn(x, center=True, scale=False, relu=True)
        return s.head(x, nc)
    return build


def _bias_relu(s):
    x = s.conv(-1, (3, 3), 6, relu=True, bias=True)
    for bias, relu in ((False, False), (True, False), (False, True), (True, True)):
        x = s.dw(x, (3, 3), bias=bias, relu=relu)
    return s.head(x)


def _fanout(s):
    a = s.conv(-1, (3, 3), 6, relu=True, bias=True)
    return s.head(s.add(s.dw(a, (3, 3), bias=True), s.conv(a, (3, 3), 6), relu=True))       # a's gradient: two accumulations


def _from_input(s):
    return s.head(s.conv(s.dw(-1, (3, 3), bias=True, relu=True), (3, 3), 6, relu=True))    # no data gradient (in = -1), C = 1


def _wide_input(s):
    return s.head(s.conv(s.dw(-1, (3, 3), bias=True), (1, 1), 4, relu=True), 2)


def _separable(s):
    """Two depthwise-separable blocks behind a strided stem, as a DS-CNN has them."""
    x = s.bn(s.conv(-1, (4, 3), 8, stride=(2, 1), bias=True), center=True, scale=False, relu=True)
    for _ in range(2):
        x = s.bn(s.dw(x, (3, 3)), center=True, scale=False, relu=True)
        x = s.bn(s.conv(x, (1, 1), 8), center=True, scale=False, relu=True)
    return s.head(x)


def _shards(s):
    return s.head(s.dw(s.dw(s.conv(-1, (3, 3), 6, relu=True, bias=True), (3, 3), relu=True, bias=True), (3, 2), stride=(2, 1)))


ROWS = [
    # ---- planes
    ("p1x1", 1, 1, 9, sep(5), "plane:1x1 k:3x3 c:5 b:9"),
    ("p1x7", 1, 7, 3, sep(5, (1, 5)), "plane:1x7 k:1x5"),
    ("p5x1_k9x1", 5, 1, 3, sep(5, (9, 1)), "plane:5x1 k:9x1 window>plane"),          # 1-D temporal; the 9-tap window is larger than the plane
    ("p13x5", 13, 5, 2, sep(5, bias=True), "plane:13x5 b:2 bias:1 relu:0"),
    # ---- forward row tiles of the 256-thread instance: T - 1, T, T + 1, 2T + 1 rows (9 wide: more than 256 outputs)
    ("rows31", 31, 9, 1, sep(3), "rows:T-1 c:3 b:1", {"T": 32}),
    ("rows32", 32, 9, 1, sep(3), "rows:T", {"T": 32}),
    ("rows33", 33, 9, 1, sep(3), "rows:T+1", {"T": 32}),
    ("rows65_s21", 65, 9, 1, sep(3, stride=(2, 1), relu=True, bias=True), "rows:dgrad-2T+1 stride:2x1", {"T": 32}),   # 33 output rows; the data gradient tiles 65
    ("rows65", 65, 9, 1, sep(3), "rows:2T+1", {"T": 32}),
    ("p98x40", 98, 40, 1, sep(4), "plane:98x40 c:4", {"T": 32}),
    ("tile_shrinks", 40, 130, 1, _wide_input, "rows:T<32 in:-1 c:1", {"T": 29, "nc": 2}),   # 34 rows x 130 floats > 4096: the tile shrinks to 29
    # ---- kernels
    ("k1x1", 6, 5, 3, sep(5, (1, 1)), "k:1x1"),
    ("k4x10", 13, 12, 2, sep(5, (4, 10)), "k:4x10"),                                  # even: SAME pads (1, 2) x (4, 5)
    ("k5x5_on_3x3", 3, 3, 3, sep(5, (5, 5)), "k:5x5 window>plane"),
    ("k_valid_plane", 5, 4, 3, sep(5, (5, 4), pad="VALID", relu=True), "k:valid=plane relu:1 bias:0"),
    # ---- strides on planes that are no multiple of them
    ("s22", 7, 5, 3, sep(5, stride=(2, 2)), "stride:2x2"),
    ("s21", 7, 6, 3, sep(5, stride=(2, 1)), "stride:2x1"),
    ("s12", 6, 7, 3, sep(5, stride=(1, 2)), "stride:1x2"),
    ("s33", 8, 7, 3, sep(5, stride=(3, 3)), "stride:3x3"),
    ("s22_valid", 8, 7, 3, sep(5, stride=(2, 2), pad="VALID"), "stride:2x2 valid"),   # (8 - 3) % 2 != 0: the last input row gets no gradient
    # ---- rates
    ("r22", 9, 7, 3, sep(5, rate=(2, 2)), "rate:2x2"),
    ("r14", 5, 10, 3, sep(5, (2, 3), rate=(1, 4)), "rate:1x4"),
    # ---- channels
    ("c3", 4, 3, 2, sep(3), "c:3"),
    ("c4", 4, 3, 2, sep(4), "c:4"),
    ("c63", 4, 3, 2, sep(63), "c:63"),
    ("c64", 4, 3, 2, sep(64), "c:64"),
    ("c65", 4, 3, 2, sep(65), "c:65"),
    ("c276", 3, 3, 2, sep(276), "c:276"),
    # ---- batches around the filter-gradient chunks (ceil(batch / 8), at most 64), a center-only BN behind the node
    ("b1", 4, 3, 1, sep(5, bn=True), "b:1 bn:center"),
    ("b8", 4, 3, 8, sep(5, bn=True), "b:8 bn:center"),
    ("b9", 4, 3, 9, sep(5, bn=True), "b:9 bn:center"),
    ("b17", 4, 3, 17, sep(5, bn=True), "b:17 bn:center"),
    ("b513", 2, 2, 513, sep(4, nc=2), "b:513", {"nc": 2}),                             # the 64-chunk clamp: 9 utterances per block, 57 chunks
    # ---- bias / ReLU, structure
    ("bias_relu", 6, 5, 3, _bias_relu, "bias:0 bias:1 relu:0 relu:1"),
    ("fanout", 6, 5, 3, _fanout, "fanout"),
    ("from_input", 6, 5, 3, _from_input, "in:-1 c:1"),
    ("separable", 9, 6, 4, _separable, "bn:center separable"),
    ("shards", 6, 5, 6, _shards, "shards"),
]
ROW_IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}
SHARD_ROW, STAGED_ROW, ORDER_ROWS = "shards", "b9", ["rows65_s21", "b17", "fanout"]
# what the table must reach
REQUIRED = ("plane:1x1 plane:1x7 plane:5x1 plane:13x5 plane:98x40 rows:T-1 rows:T rows:T+1 rows:2T+1 rows:T<32 "
            "k:1x1 k:3x3 k:9x1 k:1x5 k:4x10 k:5x5 window>plane k:valid=plane stride:2x2 stride:2x1 stride:1x2 stride:3x3 rate:2x2 rate:1x4 "
            "c:1 c:3 c:4 c:5 c:63 c:64 c:65 c:276 b:1 b:2 b:8 b:9 b:17 b:513 bias:0 bias:1 relu:0 relu:1 bn:center fanout in:-1").split()

# construction-time geometries of the exact checks (tests/test_g2d_dw.py::check_exact): (h, w, c, k, stride, rate, pad)
EXACT = [
    (1, 1, 3, (3, 3), (1, 1), (1, 1), "SAME"),
    (5, 1, 3, (9, 1), (1, 1), (1, 1), "SAME"),
    (1, 7, 2, (1, 5), (1, 1), (1, 1), "SAME"),
    (13, 12, 2, (4, 10), (1, 1), (1, 1), "SAME"),
    (3, 3, 3, (5, 5), (1, 1), (1, 1), "SAME"),
    (5, 4, 3, (5, 4), (1, 1), (1, 1), "VALID"),
    (7, 5, 3, (3, 3), (2, 2), (1, 1), "SAME"),
    (7, 6, 3, (3, 3), (2, 1), (1, 1), "SAME"),
    (6, 7, 3, (3, 3), (1, 2), (1, 1), "SAME"),
    (8, 7, 3, (3, 3), (3, 3), (1, 1), "SAME"),
    (8, 7, 3, (3, 3), (2, 2), (1, 1), "VALID"),
    (9, 7, 3, (3, 3), (1, 1), (2, 2), "SAME"),
    (5, 10, 3, (2, 3), (1, 1), (1, 4), "SAME"),
    (31, 9, 2, (3, 3), (1, 1), (1, 1), "SAME"),
    (33, 9, 2, (3, 3), (1, 1), (1, 1), "SAME"),
    (65, 9, 2, (3, 3), (1, 1), (1, 1), "SAME"),
    (65, 9, 2, (5, 3), (2, 1), (1, 1), "SAME"),
    (98, 40, 1, (3, 3), (1, 1), (1, 1), "SAME"),
    (40, 130, 1, (3, 3), (1, 1), (1, 1), "SAME"),
]
