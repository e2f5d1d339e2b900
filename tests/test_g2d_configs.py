"""The generic 2-D layer-graph engine (csrc/net2d.cpp, net2d_kernels.hip, the C ABI tcr_g2d_*, engine.Graph2D) across its layer
configuration space: a table of small graphs, each written for one branch of the kernels or of the host code that no factory model
takes -- output-channel tiles and remainders, reduced channels that are no multiple of 4, position counts around the 32-position
groups, non-square kernels / strides / dilations, SAME and VALID windows of every pooling form, filter-gradient batch chunks, BN
with one of center / scale, fan-out, aliasing dropouts, the SVDF pieces, the head.  One spec describes a graph to both sides: the
builder below turns it into an engine.Graph2D, oracle.net2d_ref.graph_forward interprets it in float64.  Per row: eval logits /
probabilities / argmax, train-mode logits / loss / EVERY gradient / moving statistics, run-to-run reproducibility; which kernels
ran, from the emulator's launch log; then shards, one Adam step and the decayed set, writes outside what the C ABI declares,
pointers one float off, the construction-time refusals, the detection stack on a graph that is no factory model.  Emulator
(`-m "not gpu"`) and MI355X (`-m gpu`): the same rows, shapes and batches (the dispatch is host code)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import dscnn_ref as D
from oracle import net2d_ref as O
from oracle import numpy_ref as R
from tests import common as Cm
from tests.test_models2d import _randomise, _split
from tests.test_net_configs import GUARD, MIN_BN_POSITIONS, OPT_TOL, PATTERN, PROB_TOL, STAT_TOL, Guarded, Log, kernel_of, launch_log  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_TOL = 1e-4
GRAD_RTOL = 3e-4            # tests/test_models2d.py::_check's default for this engine, relative to max(|ref|, 1e-3)
HALO = T._lib.HALO
TSEED, TOFF = 17, 5         # dropout seed and sample offset of the rows' training step
TCR_TUNE_BWD_MASK = 12      # include/tcresnet_hip.h


# ---- one spec for both sides ----------------------------------------------------------------------------------------------------------
class Spec:
    """Node list in the form oracle.net2d_ref.graph_forward reads; variables are named after the node's index."""

    def __init__(self):
        self.nodes = []

    def _add(self, **n):
        self.nodes.append(n)
        return len(self.nodes) - 1

    def conv(self, inp, k, cout, stride=(1, 1), rate=(1, 1), pad="SAME", relu=False, bias=False):
        i = len(self.nodes)
        return self._add(op="conv", k=k, cout=cout, stride=stride, rate=rate, pad=pad, relu=relu, w=f"n{i}/weights",
                         b=f"n{i}/biases" if bias else None, **{"in": inp})

    def bn(self, inp, center=True, scale=True, relu=False, prefix=None):
        return self._add(op="bn", prefix=prefix or f"n{len(self.nodes)}/BatchNorm", center=center, scale=scale, relu=relu, **{"in": inp})

    def pool(self, inp, kind, k=None, stride=(1, 1), pad="VALID"):
        return self._add(op="pool", kind=kind, k=k, stride=stride, pad=pad, **{"in": inp})

    def add(self, a, b, relu=False):
        return self._add(op="add", a=a, b=b, relu=relu)

    def dropout(self, inp, keep):
        return self._add(op="dropout", keep=keep, **{"in": inp})

    def tfilt(self, inp):
        return self._add(op="tfilt", w=f"n{len(self.nodes)}/weights_time", **{"in": inp})

    def gsum(self, inp, group, relu=False, bias=False):
        return self._add(op="gsum", group=group, relu=relu, b=f"n{len(self.nodes)}/bias" if bias else None, **{"in": inp})

    def head(self, inp, nc=12, pool=True):
        """[global average ->] 1 x 1 conv with bias: the logits node."""
        return self.conv(self.pool(inp, "avg") if pool else inp, (1, 1), nc, bias=True)


def build_graph(lib, spec, h, w, finalize=True):
    """The spec as an engine.Graph2D: the same node list, so engine and oracle cannot differ in topology."""
    g = T.Graph2D("", h, w, 1, lib=lib, device=Cm.device_of(lib))
    for i, n in enumerate(spec["nodes"]):
        op = n["op"]
        if op == "conv":
            got = g.conv(n["in"], n["k"], n["cout"], n["w"], stride=n["stride"], rate=n["rate"], padding=n["pad"], relu=n["relu"], biases_name=n["b"])
        elif op == "bn":
            got = g.batch_norm(n["in"], n["prefix"], center=n["center"], scale=n["scale"], relu=n["relu"])
        elif op == "pool":
            got = g.pool(n["in"], n["kind"], n["k"], n["stride"], n["pad"])
        elif op == "add":
            got = g.add(n["a"], n["b"], relu=n["relu"])
        elif op == "dropout":
            got = g.dropout(n["in"], n["keep"])
        elif op == "tfilt":
            got = g.time_filter(n["in"], n["w"])
        else:
            got = g.group_sum(n["in"], n["group"], relu=n["relu"], biases_name=n["b"])
        assert got == i, (op, got, i)
    if finalize:
        g.finalize(spec["logits"])
    return g


def graph(fn):
    """fn(Spec) -> logits node  ->  the spec dict."""
    s = Spec()
    logits = fn(s)
    return {"nodes": s.nodes, "logits": logits}


# ---- row templates ------------------------------------------------------------------------------------------------------------------
def chan(c, cin_next=8):
    """3 x 3 conv to `c` channels, then one that reduces over them (its data gradient has M = c): the output-channel tiles."""
    return lambda s: s.head(s.conv(s.conv(-1, (3, 3), c, relu=True), (3, 3), cin_next, bias=True))


def geo(nc=12, stem=5, **kw):
    """A 5-channel stem, then the conv under test (so its data gradient runs and is seen in the stem's filter gradient)."""
    kw.setdefault("k", (3, 3))
    kw.setdefault("cout", 6)
    return lambda s: s.head(s.conv(s.conv(-1, (3, 3), stem, relu=True, bias=True), **kw), nc)


def pooled(kind, relu=False, **kw):
    """A stem WITHOUT ReLU (the argmax of every window matters), the pooling under test, the head."""
    return lambda s: s.head(s.pool(s.conv(-1, (3, 3), 5, relu=relu, bias=True), kind, **kw))


def conv_bn(c=8, **bn):
    return lambda s: s.head(s.bn(s.conv(s.bn(s.conv(-1, (3, 3), c), relu=True), (3, 3), c), **bn))


def bn_on(c, **bn):
    return lambda s: s.head(s.bn(s.conv(-1, (3, 3), c), **bn))


def _bias_relu(s):
    x = -1
    for bias, relu in ((False, False), (True, False), (False, True), (True, True)):
        x = s.conv(x, (3, 3), 6, bias=bias, relu=relu)
    return s.head(x)


def _cin_chain(s):
    x = -1
    for c in (3, 5, 17, 6):
        x = s.conv(x, (3, 3), c, relu=True, bias=True)      # (a bias: no patches of exact zeros behind the one-channel input)
    return s.head(x)


def _bn_1x1(s):
    return s.conv(s.bn(s.pool(s.conv(-1, (3, 3), 6, relu=True), "avg"), relu=True), (1, 1), 12, bias=True)


def _bn_names(s):
    a = s.bn(s.conv(-1, (3, 3), 8), relu=True, prefix="first/BatchNorm")
    return s.head(s.bn(s.conv(a, (3, 3), 8), prefix="second/bn"))


def _max_after_bn(s):
    return s.head(s.pool(s.bn(s.conv(-1, (3, 3), 6)), "max", (3, 3), (2, 2), "SAME"))


def _max_after_relu_dropout(s):
    return s.head(s.pool(s.dropout(s.conv(-1, (3, 3), 6, relu=True), 0.6), "max", (2, 2), (2, 2), "SAME"))


def _fan3(s):
    a = s.conv(-1, (3, 3), 6, relu=True)
    b, c = s.conv(a, (3, 3), 6), s.conv(a, (1, 1), 6, relu=True)
    return s.head(s.add(s.add(b, c), a, relu=True))


def _add_aa(s):
    a = s.conv(-1, (3, 3), 6, bias=True)
    return s.head(s.conv(s.add(a, a, relu=True), (3, 3), 6))


def _two_from_input(s):
    return s.head(s.add(s.conv(-1, (3, 3), 6, relu=True), s.conv(-1, (1, 5), 6)))


def _dead_branch(s):
    a = s.conv(-1, (3, 3), 6, relu=True)
    s.pool(s.bn(s.conv(a, (3, 3), 5, bias=True), relu=True), "max", (2, 2), (2, 2), "SAME")        # nobody reads this
    return s.head(s.conv(a, (3, 3), 6))


def _dropout_logits(s):
    return s.dropout(s.head(s.conv(-1, (3, 3), 6, relu=True)), 0.7)


def _dropout_dropout(s):
    return s.head(s.dropout(s.dropout(s.conv(-1, (3, 3), 6, relu=True), 0.8), 0.5))


def _dropout_dropout_logits(s):
    return s.dropout(s.dropout(s.head(s.conv(-1, (3, 3), 6, relu=True)), 0.9), 0.8)


def _tfilt_input(s):
    return s.conv(s.conv(s.tfilt(-1), (1, 1), 6, relu=True, bias=True), (1, 1), 12, bias=True)


def svdf(group, relu, bias, c=6):
    return lambda s: s.conv(s.gsum(s.tfilt(s.conv(-1, (3, 3), c)), group, relu=relu, bias=bias), (1, 1), 12, bias=True)


def _shards(s):
    a = s.dropout(s.conv(-1, (3, 3), 6, relu=True, bias=True), 0.5)
    return s.head(s.dropout(s.conv(a, (3, 3), 7, relu=True), 0.8))


def _detect(s):
    a = s.conv(-1, (3, 3), 8, stride=(2, 3), relu=True, bias=True)
    return s.head(s.conv(s.pool(a, "max", (3, 3), (2, 2), "SAME"), (3, 3), 8, relu=True))


# (id, plane height, plane width, batch, graph[, options]).  Options: ls = label smoothing; zero = prefixes of the variables whose
# gradient must be exactly zero.  Each row's comment names the branch it is there for.
ROWS = [
    # ---- conv output-channel tiles: launch_conv2d_t's MT = min(3, tiles) and the remainder workgroup; the same counts as the next conv's
    # reduced channels, i.e. the M of its data gradient
    ("cout12", 6, 5, 3, chan(12)),          # one partial tile (MT = 1)
    ("cout16", 6, 5, 3, chan(16)),          # one full tile
    ("cout17", 6, 5, 3, chan(17)),          # two tiles, the second one channel wide (MT = 2)
    ("cout33", 6, 5, 3, chan(33)),          # three tiles (MT = 3), the third one channel wide
    ("cout48", 6, 5, 3, chan(48)),          # three full tiles
    ("cout49", 6, 5, 3, chan(49)),          # four tiles: a second workgroup row with two of its three tiles past the end
    ("cout97", 6, 5, 3, chan(97)),          # seven tiles: three workgroup rows, the last with one tile one channel wide
    # ---- reduced channels that are no multiple of 4: the c4 loop's `kc < KC` predicate (forward cin, data gradient cout)
    ("cin_1_3_5_17", 6, 5, 3, _cin_chain),
    # ---- positions: 32 per wave, 128 per workgroup
    ("pos24", 3, 4, 2, chan(6)),            # batch x plane below one wave's 32
    ("pos128", 4, 4, 8, chan(6)),           # exactly one workgroup
    ("pos129", 1, 3, 43, chan(6)),          # a second workgroup holding one position; 43 utterances: six filter-gradient chunks of 8, 8 ... 3
    ("pos_2x3_b7", 2, 3, 7, chan(6)),       # a 32-position group spans six utterances
    # ---- geometry
    ("k1x5", 6, 7, 3, geo(k=(1, 5))),       # non-square kernels
    ("k5x1", 7, 6, 3, geo(k=(5, 1))),
    ("k4x2", 7, 6, 3, geo(k=(4, 2))),       # even kernel: SAME pads (1, 2) x (0, 1)
    ("s21_even", 8, 6, 3, geo(stride=(2, 1))),      # SAME on an even plane: the one pad element goes high
    ("s21_odd", 7, 5, 3, geo(stride=(2, 1))),       # on an odd plane: one low, one high
    ("s13_even", 6, 6, 3, geo(stride=(1, 3))),
    ("s13_odd", 5, 7, 3, geo(stride=(1, 3))),
    ("s22_even", 8, 6, 3, geo(stride=(2, 2))),
    ("s22_odd", 7, 9, 3, geo(stride=(2, 2))),
    ("valid_s2_8x7", 8, 7, 3, geo(stride=(2, 2), pad="VALID")),     # (8 - 3) % 2 != 0: the last input row gets no gradient
    ("valid_s2_7x8", 7, 8, 3, geo(stride=(2, 2), pad="VALID")),     # ... the last input column
    ("k1_s2", 7, 6, 3, geo(k=(1, 1), stride=(2, 2))),               # stride larger than the kernel, SAME: total pad < 0 clamps to 0
    ("dil21", 9, 7, 3, geo(k=(3, 2), rate=(2, 1))),                 # non-square dilation on a non-square kernel
    ("dil13", 5, 10, 3, geo(k=(2, 3), rate=(1, 3))),
    ("dil44", 10, 9, 3, geo(rate=(4, 4))),
    ("dil_past_plane", 3, 3, 4, geo(rate=(4, 4))),                  # effective 9 x 9 on 3 x 3: every tap but the centre in the padding
    ("full_plane_valid", 5, 4, 3, lambda s: s.conv(s.conv(s.conv(-1, (3, 3), 5, relu=True), (5, 4), 9, pad="VALID", relu=True), (1, 1), 12, bias=True)),   # the fully connected form
    ("bias_relu", 6, 5, 3, _bias_relu),                             # bias and ReLU on and off, all four
    # ---- pooling: SAME windows clipped to the plane (avg divides by the in-plane count), VALID windows inside it
    ("avg_33s2_same", 7, 6, 3, pooled("avg", k=(3, 3), stride=(2, 2), pad="SAME")),     # overlapping strided windows
    ("max_33s2_same", 7, 6, 3, pooled("max", k=(3, 3), stride=(2, 2), pad="SAME")),
    ("avg_22s1_same", 6, 5, 3, pooled("avg", k=(2, 2), stride=(1, 1), pad="SAME")),     # the pad on the high side only
    ("max_22s1_same", 6, 5, 3, pooled("max", k=(2, 2), stride=(1, 1), pad="SAME")),
    ("avg_22s3_valid", 8, 9, 3, pooled("avg", k=(2, 2), stride=(3, 3), pad="VALID")),   # stride larger than the window: inputs no window holds
    ("max_22s3_valid", 8, 9, 3, pooled("max", k=(2, 2), stride=(3, 3), pad="VALID")),
    ("avg_big_same", 3, 4, 3, pooled("avg", k=(5, 7), stride=(1, 1), pad="SAME")),      # a window larger than the plane
    ("max_big_same", 3, 4, 3, pooled("max", k=(5, 7), stride=(1, 1), pad="SAME")),
    ("avg_13s13_valid", 5, 10, 3, pooled("avg", k=(1, 3), stride=(1, 3), pad="VALID")),
    ("max_13s13_valid", 5, 10, 3, pooled("max", k=(1, 3), stride=(1, 3), pad="VALID")),
    ("max_global", 6, 5, 3, pooled("max")),                                             # global pool (avg: every row's head)
    ("max_after_bn", 7, 6, 3, _max_after_bn),                       # no ReLU zeros in front: every window's argmax matters
    ("max_after_relu_dropout", 6, 6, 3, _max_after_relu_dropout),   # windows of zeros and ties at zero
    # ---- batches: launch_conv2d_wgrad's ceil(batch / 8) chunks -- 1, 2, 3 (6 + 6 + 5) and 5 of them -- on a conv + BN graph
    ("b1", 4, 3, 1, conv_bn()),
    ("b9", 4, 3, 9, conv_bn()),
    ("b17", 4, 3, 17, conv_bn()),
    ("b33", 4, 3, 33, conv_bn()),
    ("b513", 2, 2, 513, lambda s: s.head(s.conv(s.conv(-1, (3, 3), 4, relu=True), (3, 3), 4), 2)),   # the 64-chunk clamp: 9 utterances per block, 57 chunks
    # ---- BN: one of center / scale (dbeta to scratch, the zero block for beta), the 16-byte forms' c * (plane + 8) % 4
    ("bn_center_only", 4, 3, 3, conv_bn(center=True, scale=False)),
    ("bn_center_only_relu", 4, 3, 3, conv_bn(center=True, scale=False, relu=True)),
    ("bn_scale_only", 4, 3, 3, conv_bn(center=False, scale=True)),
    ("bn_scale_only_relu", 4, 3, 3, conv_bn(center=False, scale=True, relu=True)),
    ("bn_1x1", 4, 3, 9, _bn_1x1),                                   # BN on a 1 x 1 plane behind a global pool
    ("bn_c5_3x3", 3, 3, 3, bn_on(5, relu=True)),                    # 5 x 17 floats per utterance: the scalar forms
    ("bn_c8_4x4", 4, 4, 3, bn_on(8, relu=True)),                    # 8 x 24: the 16-byte apply
    ("bn_names", 4, 4, 3, _bn_names),                               # a "BatchNorm" prefix and a plain one: the decayed set (OPTIM_ROW)
    # ---- structure
    ("fan3", 6, 5, 3, _fan3),                                       # a ReLU conv read by three nodes
    ("add_aa", 6, 5, 3, _add_aa),                                   # add(a, a): both fan-outs into one gradient buffer
    ("two_from_input", 6, 5, 3, _two_from_input),                   # two convs read the network input (no data gradient)
    ("dead_branch", 6, 5, 3, _dead_branch, {"zero": ("n1/", "n2/")}),   # a branch nobody consumes: gradients exactly zero
    ("dropout_logits", 6, 5, 3, _dropout_logits),                   # eval: the head reads through the aliasing dropout
    ("dropout_dropout", 6, 5, 3, _dropout_dropout),
    ("dropout_dropout_logits", 6, 5, 3, _dropout_dropout_logits),   # two aliases in a row in front of the head
    # ---- the SVDF pieces
    ("tfilt_input", 6, 5, 4, _tfilt_input),                         # the time filter on the network input: no data gradient (gin0 null)
    ("gsum1", 6, 5, 3, svdf(1, False, False)),
    ("gsum2_bias_relu", 6, 5, 3, svdf(2, True, True)),
    ("gsum3_bias", 6, 5, 3, svdf(3, False, True)),
    ("gsum2_relu", 6, 5, 3, svdf(2, True, False, c=10)),
    # ---- the head
    ("nc2", 6, 5, 3, geo(nc=2)),
    ("nc35", 6, 5, 3, geo(nc=35)),
    ("smooth", 6, 5, 3, geo(nc=12), {"ls": 0.1}),                   # label smoothing 0.1
    # ---- the named tests' graphs (also plain rows)
    ("shards", 6, 5, 6, _shards),                                   # BN-free with dropout, batch 6 (SHARD_ROW)
]
ROW_IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}
SHARD_ROW, OPTIM_ROW = "shards", "bn_names"
GUARD_ROWS = ["cout49", "max_after_relu_dropout", "bn_names", "gsum2_bias_relu", "pos129"]
UNALIGNED_ROWS = ["bn_c8_4x4", "bn_names", "max_33s2_same"]
KNOB_ROW, STAGED_ROW = "bn_c8_4x4", "b9"

_SPECS = {}


def spec_of(row):
    if row[0] not in _SPECS:
        _SPECS[row[0]] = graph(row[4])
    return _SPECS[row[0]]


def opts_of(row):
    return row[5] if len(row) > 5 else {}


# ---- the launch log -----------------------------------------------------------------------------------------------------------------
def source_launch_names():
    """check_launch("...") names and __global__ kernels of net2d_kernels.hip, from the source text."""
    with open(os.path.join(ROOT, "tc-resnet_amd", "csrc", "net2d_kernels.hip")) as fh:
        text = fh.read()
    return set(re.findall(r'check_launch\("([A-Za-z0-9_]+)"\)', text)), set(re.findall(r"__global__[^;{]*?void (\w+)\(", text))


# a check_launch name that stands for kernels of other names
LAUNCH_OF = {"tfilt_bwd_kernel": ("tfilt_dx_kernel", "tfilt_dw_kernel")}
# the kernels of bn.hip that net2d.cpp's calls can end in (launch_bn_fold / _chan_reduce / _chan_sums / _bn_finalize / _bn_apply /
# _bn_bwd_finalize / _bn_bwd_apply)
BN_FORMS = {"bn_fold_kernel", "chan_reduce_kernel", "chan_reduce4_kernel", "chan_sums_kernel", "bn_finalize_kernel", "bn_apply_kernel",
            "bn_apply4_kernel", "bn_bwd_finalize_kernel", "bn_bwd_apply_kernel", "bn_bwd_apply4_kernel", "bn_bwd_apply4x_kernel"}
EXEMPT = {
    "bn_bwd_apply4_kernel": "launch_bn_bwd_apply takes its 16-byte forms for accumulate = 0 only; net2d.cpp always accumulates into the input's gradient",
    "bn_bwd_apply4x_kernel": "as bn_bwd_apply4_kernel",
}
LAUNCHED = set()


# the instances of net2d_kernels.hip's two kernel templates: conv2d_mfma_kernel<MT, DGRAD>, eltwise2d_kernel<MODE>
FORMS = {f"conv2d_mfma_kernel<{mt}, {d}>" for mt in (1, 2, 3) for d in ("false", "true")} | {f"eltwise2d_kernel<{m}>" for m in range(5)}


def forms_of(logs):
    """The template instances among the logged launches ("... = void tcr::conv2d_mfma_kernel<3, false>(tcr::Conv2dArgs)")."""
    return {m for g in logs for e in g.entries for m in re.findall(r"tcr::((?:conv2d_mfma|eltwise2d)_kernel<[^>()]*>)\(", e)}


def implied_names(spec, h, w, aligned=True):
    """The kernels of net2d_kernels.hip and BN_FORMS that eval, training forward and backward of a spec launch by default; every
    node's shape; the template instances among the kernels (FORMS)."""
    names = {"features_to_plane_kernel", "head2d_kernel", "eltwise2d_kernel"}      # (the loss gradient is fanned into the logits node)
    forms = {"eltwise2d_kernel<2>"}
    mt = lambda m: min(3, -(-m // 16))
    shapes = []
    shape = lambda i: (1, h, w) if i < 0 else shapes[i]
    for n in spec["nodes"]:
        op = n["op"]
        cin, ih, iw = shape(n.get("in", n.get("a")))
        if op == "conv":
            names |= {"conv2d_mfma_kernel", "conv2d_wgrad_kernel"} | ({"chan_sum2d_kernel"} if n["b"] else set())
            forms |= {f"conv2d_mfma_kernel<{mt(n['cout'])}, false>"} | ({f"conv2d_mfma_kernel<{mt(cin)}, true>"} if n["in"] >= 0 else set())
            x = torch.zeros((1, 1, ih, iw), dtype=torch.float64)
            y = O.conv2d(x, torch.zeros(tuple(n["k"]) + (1, 1), dtype=torch.float64), tuple(n["stride"]), tuple(n["rate"]), n["pad"])
            shapes.append((n["cout"], y.shape[2], y.shape[3]))
        elif op == "bn":
            vec = aligned and (cin * (ih * iw + 2 * HALO)) % 4 == 0
            names |= {"bn_fold_kernel", "chan_reduce_kernel", "bn_finalize_kernel", "bn_apply4_kernel" if vec else "bn_apply_kernel",
                      "bn_bwd_finalize_kernel", "bn_bwd_apply_kernel"}
            shapes.append((cin, ih, iw))
        elif op == "pool":
            names |= {"pool2d_fwd_kernel", "pool2d_bwd_kernel"}
            x = torch.zeros((1, 1, ih, iw), dtype=torch.float64)
            y = O.avg_pool(x, tuple(n["k"]), tuple(n["stride"]), n["pad"]) if n["k"] else x[:, :, :1, :1]
            shapes.append((cin, y.shape[2], y.shape[3]))
        elif op in ("add", "dropout"):
            forms |= {"eltwise2d_kernel<0>"} if op == "add" else {"eltwise2d_kernel<3>", "eltwise2d_kernel<4>"}
            shapes.append((cin, ih, iw))
        elif op == "tfilt":
            names |= {"tfilt_fwd_kernel", "tfilt_dw_kernel"} | ({"tfilt_dx_kernel"} if n["in"] >= 0 else set())
            shapes.append((cin, 1, 1))
        else:
            names |= {"gsum_fwd_kernel", "gsum_dx_kernel"} | ({"chan_sum2d_kernel"} if n["b"] else set())
            shapes.append((cin // n["group"], 1, 1))
        if n.get("relu") and op != "bn":            # (a BN's ReLU is part of its own kernels)
            forms.add("eltwise2d_kernel<1>")
    return names, shapes, forms


def assert_launches(lib, row, logs, aligned=True, swap=None, abi=False):
    """Of net2d_kernels.hip's kernels and the BN forms, the row launched exactly those its spec stands for (emulator).  abi: the passes
    went through the C ABI on a ready input plane (no re-layout of front-end features among them)."""
    if lib.kind != "emu":
        return
    got = {kernel_of(e) for g in logs for e in g.entries}
    LAUNCHED.update(got)
    want, _, forms = implied_names(spec_of(row), row[1], row[2], aligned)
    eval_only = {f for f in forms if f.startswith("eltwise2d_kernel") or f.endswith("true>")} if len(logs) == 1 else set()
    assert forms_of(logs) == forms - eval_only, (row[0], "instances", sorted(forms_of(logs)), "expected", sorted(forms - eval_only))
    for a, b in (swap or {}).items():
        want = (want - {a}) | {b}
    want -= {"features_to_plane_kernel"} if abi else set()
    scope = source_launch_names()[1] | BN_FORMS
    assert got & scope == want, (row[0], "launched", sorted((got & scope) - want), "not launched", sorted(want - (got & scope)))


# ---- one row --------------------------------------------------------------------------------------------------------------------------
def record(kind, lib, name, errs):
    print("G2D_CONFIGS_ERR", json.dumps({"kind": kind, "lib": lib.kind, "row": name, "errs": {k: float(f"{v:.4g}") for k, v in errs.items()}}))


def features(batch, h, w, seed=300):
    return np.random.RandomState(seed).uniform(-2.0, 2.0, (batch, h, w)).astype(np.float32)


def planar(lib, x):
    return T.features_to_planar(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(Cm.device_of(lib)), lib=lib)


def masks_of(eng, spec, batch, seed=TSEED, off=TOFF):
    return [O.dropout_mask(seed, n, off, batch, int(np.prod(eng.shape(n))), spec["nodes"][n]["keep"]) for n in eng.dropout_nodes] or None


def row_setup(lib, row, seed=0):
    name, h, w, batch = row[:4]
    spec = spec_of(row)
    eng = build_graph(lib, spec, h, w)
    sd = _randomise(eng, seed + 1)
    p, s = _split(eng, sd)
    x = features(batch, h, w, 300 + seed)
    labels = R.synth_labels(batch, num_classes=eng.num_classes).astype(np.float64)
    for i, n in enumerate(spec["nodes"]):
        if n["op"] == "bn":
            assert batch * eng.shape(i)[1] * eng.shape(i)[2] >= MIN_BN_POSITIONS, (name, i)
    return dict(spec=spec, eng=eng, sd=sd, p=p, s=s, x=x, xt=torch.tensor(x.astype(np.float64)), labels=labels, masks=masks_of(eng, spec, batch))


def oracle_eval(st):
    tp = {k: torch.tensor(v) for k, v in st["p"].items()}
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in O.graph_forward(st["spec"], tp, st["s"], st["xt"], False, None).items()}


def oracle_train(st, kept, ls=0.0, errs=None, name=""):
    """The oracle's training step on the kernels' side of the ReLU inputs within tau of zero (`kept`: the post-ReLU activations > 0)."""
    with O.follow_kinks(kept) as log:
        out, model, _tot, grads = O.loss_and_grads(lambda pp: O.graph_forward(st["spec"], pp, st["s"], st["xt"], True, st["masks"]), st["p"],
                                                   st["labels"], label_smoothing=ls)
    near, total, followed = log["near"], log["total"], log["followed"]
    assert near <= 2 + 1e-4 * total and followed <= near, (name, "ReLU inputs within tau of zero", near, "of", total, "followed", followed)
    if errs is not None:
        errs["relu_near"] = near
    return out, model, grads


def grad_errors(got_of, tensors, gref, what, zero=()):
    worst, checked = 0.0, 0
    for k, ref in gref.items():
        got = got_of(k).reshape(ref.shape).astype(np.float64)
        checked += 1
        if any(k.startswith(z) for z in zero):
            assert not ref.any() and np.all(got == 0.0), (what, k, "a variable nobody's output depends on has gradient exactly 0")
            continue
        e = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-3))
        worst = max(worst, e)
        assert e < GRAD_RTOL, f"{what}: {k}: grad rel err {e}"
    trainable = [k for k, ti in tensors.items() if ti.arena == 0]
    assert checked == len(trainable) and set(gref) == set(trainable), (what, checked, len(trainable))
    return worst


def stat_errors(stat_of, new_stats, what):
    worst = 0.0
    for k, ref in new_stats.items():
        e = float(np.abs(stat_of(k) - ref).max() / max(1.0, np.abs(ref).max()))
        worst = max(worst, e)
        assert e < STAT_TOL, f"{what}: {k}: moving statistic err {e}"
    return worst


def pad_mask(eng):
    pads = torch.ones(eng.n_param, dtype=torch.bool)
    for ti in eng.tensors.values():
        if ti.arena == 0:
            pads[ti.offset:ti.offset + ti.size] = False
    return pads


def check_row(lib, row):
    """One row against the oracle.  Returns its worst errors."""
    name, h, w, batch = row[:4]
    ls = opts_of(row).get("ls", 0.0)
    st = row_setup(lib, row)
    eng, spec = st["eng"], st["spec"]
    feat = planar(lib, st["x"])
    errs = {}
    ev = oracle_eval(st)
    with Log(lib) as ge:
        logits, probs = [v.clone() for v in eng.forward_infer(feat)]
    lg = logits.cpu().numpy()
    errs["eval_logits"] = float(np.abs(lg - ev["logits"]).max())
    errs["eval_probs"] = float(np.abs(probs.cpu().numpy() - ev["probs"]).max())
    print(name, "eval", errs)
    assert errs["eval_logits"] < Cm.LOGIT_TOL and errs["eval_probs"] < PROB_TOL, (name, errs)
    assert np.array_equal(lg.argmax(1), ev["logits"].argmax(1)), name
    l2, p2 = eng.forward_infer(feat)
    assert torch.equal(logits, l2) and torch.equal(probs, p2), (name, "second forward_infer differs")
    for n in eng.dropout_nodes:             # eval-mode dropout: the identity, its output IS its input's buffer
        src = spec["nodes"][n]["in"]
        assert eng.node_output(n, batch, False).data_ptr() == eng.node_output(src, batch, False).data_ptr(), (name, n)
    # training step
    lab = Cm.to_dev(lib, st["labels"])
    stats0 = eng.stats.clone()
    with Log(lib) as gf:
        tl, tp, loss = [v.clone() for v in eng.forward_train(feat, lab, seed=TSEED, sample_offset=TOFF, label_smoothing=ls)]
    kept = [(eng.node_output(n, batch, True) > 0).cpu() for n in eng.relu_nodes]
    with Log(lib) as gb:
        g1 = eng.backward().clone()
    assert_launches(lib, row, (ge, gf, gb))
    out, model, grads = oracle_train(st, kept, ls, errs, name)
    errs["train_logits"] = float(np.abs(tl.cpu().numpy() - out["logits"]).max())
    errs["train_probs"] = float(np.abs(tp.cpu().numpy() - out["probs"]).max())
    errs["loss"] = abs(float(loss) / batch - model)
    print(name, "train forward", {k: errs[k] for k in ("train_logits", "train_probs", "loss")})
    assert errs["train_logits"] < Cm.LOGIT_TOL and errs["train_probs"] < PROB_TOL and errs["loss"] < LOSS_TOL, (name, errs)
    errs["stats"] = stat_errors(lambda k: eng._view(k).cpu().numpy(), out["new_stats"], name)
    errs["grads"] = grad_errors(lambda k: eng.grad_view(k).cpu().numpy(), eng.tensors, grads, name, opts_of(row).get("zero", ()))
    assert not bool(g1.cpu()[pad_mask(eng)].any()), (name, "gradient arena not zero between its tensors")
    print(name, "train", {k: errs[k] for k in ("grads", "stats", "relu_near")})
    # run-to-run: bitwise
    eng.stats.copy_(stats0)
    tl2, _, loss2 = eng.forward_train(feat, lab, seed=TSEED, sample_offset=TOFF, label_smoothing=ls)
    assert torch.equal(tl, tl2) and float(loss) == float(loss2), (name, "second forward_train differs")
    assert torch.equal(g1, eng.backward()), (name, "second backward differs")
    if name == OPTIM_ROW:
        check_adam(lib, st, g1, errs)
    record("rows", lib, name, errs)
    return errs


def check_adam(lib, st, g1, errs):
    """One tf.train.AdamOptimizer step (t = 1) with weight decay on the kernels' own gradient against the oracle's step, the decayed
    set taken from the NAMES (oracle.numpy_ref.is_l2_param: factory/audio_nets.py:175-180) -- the plain-named BN's gamma and beta are
    decayed, the "BatchNorm"-named ones are not -- and tcr_g2d_decay_floats ends where the last decayed tensor does."""
    eng = st["eng"]
    lr, wd = 1e-3, 0.01
    names = eng.trainable_names()
    assert R.is_l2_param("second/bn/gamma") and not R.is_l2_param("first/BatchNorm/gamma") and {"second/bn/gamma", "first/BatchNorm/beta"} <= set(names)
    w = {k: eng._view(k).cpu().numpy().astype(np.float64) for k in names}
    g = {k: eng.grad_view(k).cpu().numpy().astype(np.float64) + (wd * w[k] if R.is_l2_param(k) else 0.0) for k in names}
    zeros = {k: np.zeros_like(v) for k, v in w.items()}
    want, m, v = D.adam_step(w, zeros, zeros, g, lr, 1)
    decayed = [eng.tensors[k] for k in names if R.is_l2_param(k)]
    others = [eng.tensors[k] for k in names if not R.is_l2_param(k)]
    end = max(ti.offset + ti.size for ti in decayed)
    assert lib.tcr_g2d_decay_floats(eng._h) == eng.n_decay and end <= eng.n_decay < end + 128 and eng.n_decay <= min(ti.offset for ti in others)
    eng.slots.clear()
    eng.adam_step(lr, 1, weight_decay=wd)
    view = lambda arena, k: arena.cpu().numpy()[eng.tensors[k].offset:eng.tensors[k].offset + eng.tensors[k].size].reshape(w[k].shape)
    errs["adam"] = max(float(np.abs(view(eng.params, k) - want[k]).max()) for k in names)
    slot = max(max(float(np.abs(view(eng.slots["Adam"], k) - m[k]).max()), float(np.abs(view(eng.slots["Adam_1"], k) - v[k]).max())) for k in names)
    assert errs["adam"] < OPT_TOL and slot < OPT_TOL, ("adam", errs["adam"], slot)
    # the decay is what separates the two sets: without it the decayed tensors' first moments are off by (1 - beta1) wd |w| ~ 1e-3
    assert float(np.abs(view(eng.slots["Adam"], "second/bn/gamma") - 0.1 * eng.grad_view("second/bn/gamma").cpu().numpy()).max()) > 100 * OPT_TOL
    eng.slots.clear()


@pytest.mark.parametrize("name", ROW_IDS)
def test_config_row(emu_lib, name):
    check_row(emu_lib, ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_IDS)
def test_gpu_config_row(hip_lib, name):
    check_row(hip_lib, ROW[name])


# ---- the table itself -----------------------------------------------------------------------------------------------------------------
def test_rows_hold_the_listed_cases():
    """The table itself (a row that leaves takes its case with it), from the specs: no library needed."""
    assert len(set(ROW_IDS)) == len(ROWS)
    S = {r[0]: (spec_of(r), implied_names(spec_of(r), r[1], r[2])[1]) for r in ROWS}
    convs = [(r, n, S[r[0]][1][i], (1, r[1], r[2]) if n["in"] < 0 else S[r[0]][1][n["in"]]) for r in ROWS for i, n in enumerate(S[r[0]][0]["nodes"])
             if n["op"] == "conv"]
    pools = [(r, n, S[r[0]][1][i], S[r[0]][1][n["in"]]) for r in ROWS for i, n in enumerate(S[r[0]][0]["nodes"]) if n["op"] == "pool" and n["k"]]
    bns = [(r, n, S[r[0]][1][i]) for r in ROWS for i, n in enumerate(S[r[0]][0]["nodes"]) if n["op"] == "bn"]
    assert {12, 16, 17, 33, 48, 49, 97} <= {n["cout"] for _, n, _, _ in convs} and {12, 16, 17, 33, 48, 49, 97, 1, 3, 5, 17} <= {i[0] for _, _, _, i in convs}
    assert all(o[0] <= 97 and i[1] <= 16 and i[2] <= 12 for _, _, o, i in convs)
    npos = {r[3] * o[1] * o[2] for r, n, o, _ in convs}
    assert min(npos) < 32 and {128, 129} <= npos and (7, 2, 3) in {(r[3], r[1], r[2]) for r in ROWS}
    assert {(1, 5), (5, 1), (4, 2)} <= {tuple(n["k"]) for _, n, _, _ in convs}
    for st in ((2, 1), (1, 3), (2, 2)):         # SAME on an even and on an odd length of the strided dimension
        par = {tuple(i[1 + d] % 2 for d in (0, 1) if st[d] > 1) for _, n, _, i in convs if tuple(n["stride"]) == st and n["pad"] == "SAME" and n["k"] == (3, 3)}
        assert len({p[0] for p in par}) == 2, (st, par)
    assert any(n["pad"] == "VALID" and n["stride"] == (2, 2) and (i[1] - 3) % 2 and not (i[2] - 3) % 2 for _, n, _, i in convs)
    assert any(n["pad"] == "VALID" and n["stride"] == (2, 2) and (i[2] - 3) % 2 for _, n, _, i in convs)
    assert any(n["k"] == (1, 1) and n["stride"] == (2, 2) and n["pad"] == "SAME" for _, n, _, _ in convs)
    assert {(2, 1), (1, 3), (4, 4)} <= {tuple(n["rate"]) for _, n, _, _ in convs}
    assert any(n["rate"] == (4, 4) and i[1:] == (3, 3) for _, n, _, i in convs) and any(n["pad"] == "VALID" and tuple(n["k"]) == i[1:] and i[1] > 1 for _, n, _, i in convs)
    assert {(b, rl) for _, n, _, _ in convs for b, rl in [(bool(n["b"]), n["relu"])]} == {(False, False), (True, False), (False, True), (True, True)}
    for kind in ("avg", "max"):
        have = {(tuple(n["k"]), tuple(n["stride"]), n["pad"]) for _, n, _, _ in pools if n["kind"] == kind}
        assert {((3, 3), (2, 2), "SAME"), ((2, 2), (1, 1), "SAME"), ((2, 2), (3, 3), "VALID"), ((1, 3), (1, 3), "VALID")} <= have, kind
        assert any(n["kind"] == kind and n["pad"] == "SAME" and n["k"][0] > i[1] and n["k"][1] > i[2] for _, n, _, i in pools)
    assert {1, 9, 17, 33} <= {r[3] for r, _, _ in bns} and ROW["b513"][1:4] == (2, 2, 513)
    assert {(True, False), (False, True)} <= {(n["center"], n["scale"]) for _, n, _ in bns}
    assert {(n["center"], n["scale"], n["relu"]) for _, n, _ in bns} >= {(c, s, rl) for c, s in ((True, False), (False, True)) for rl in (False, True)}
    assert any(o[1:] == (1, 1) for _, _, o in bns) and {0, 1} <= {min(1, (o[0] * (o[1] * o[2] + 2 * HALO)) % 4) for _, _, o in bns}
    assert all(r[3] * o[1] * o[2] >= MIN_BN_POSITIONS for r, _, o in bns)
    heads = {S[r[0]][1][S[r[0]][0]["logits"]][0] for r in ROWS}
    assert {2, 12, 35} <= heads and any(opts_of(r).get("ls") == 0.1 for r in ROWS)
    assert {1, 2, 3} <= {n["group"] for r in ROWS for n in S[r[0]][0]["nodes"] if n["op"] == "gsum"}
    assert any(n["op"] == "tfilt" and n["in"] < 0 for r in ROWS for n in S[r[0]][0]["nodes"]) and any(n["op"] == "tfilt" and n["in"] >= 0 for r in ROWS for n in S[r[0]][0]["nodes"])
    assert all(n in ROW for n in GUARD_ROWS + UNALIGNED_ROWS + [SHARD_ROW, OPTIM_ROW, KNOB_ROW, STAGED_ROW])
    assert not any(n["op"] == "bn" for n in S[SHARD_ROW][0]["nodes"]) and any(n["op"] == "dropout" for n in S[SHARD_ROW][0]["nodes"]) and ROW[SHARD_ROW][3] == 6


def test_every_g2d_launch_is_covered():
    """Every check_launch name / kernel of net2d_kernels.hip and every BN form net2d.cpp can end in is what some row (or the knob and
    staged tests below) runs.  A row's implied kernels are asserted against the emulator's launch log when the row runs
    (assert_launches: exactly those), so the table speaks for the log; what rows launched in this process before this test is checked
    against the table once more."""
    launches, kernels = source_launch_names()
    assert len(launches) >= 12 and len(kernels) >= 13, (launches, kernels)
    covered, forms = set(), set()
    for r in ROWS:
        covered |= implied_names(spec_of(r), r[1], r[2])[0]
        forms |= implied_names(spec_of(r), r[1], r[2])[2]
    assert forms == FORMS, ("template instances no row reaches", sorted(FORMS - forms))
    for n in UNALIGNED_ROWS:
        covered |= implied_names(spec_of(ROW[n]), ROW[n][1], ROW[n][2], aligned=False)[0]
    covered |= {"chan_reduce4_kernel"}          # test_chan_reduce4_through_its_knob asserts it from the log
    covered |= {"chan_sums_kernel"}             # test_staged_equals_unstaged asserts it from the log
    scope = kernels | BN_FORMS
    assert not set(EXEMPT) - scope, ("exempt names that the sources no longer have", set(EXEMPT) - scope)
    missing = scope - covered - set(EXEMPT)
    assert not missing, ("no row of tests/test_g2d_configs.py reaches", sorted(missing))
    for name in launches:
        assert all(k in covered for k in LAUNCH_OF.get(name, (name,))), name
    assert (LAUNCHED & scope) <= covered, sorted((LAUNCHED & scope) - covered)


def check_chan_reduce4(lib):
    """chan_reduce4_kernel needs 4096 waves' worth of workgroups by default, which no test-sized plane has: TCR_TUNE_BWD_MASK = 4 lifts that
    condition (reset in the `finally`).  8 channels on a 4 x 4 plane meet its others; against the oracle like a row."""
    row = ROW[KNOB_ROW]
    name, h, w, batch = row[:4]
    st = row_setup(lib, row)
    eng = st["eng"]
    feat, lab = planar(lib, st["x"]), Cm.to_dev(lib, st["labels"])
    try:
        lib.tcr_tune(TCR_TUNE_BWD_MASK, 4)
        with Log(lib) as ge:
            eng.forward_infer(feat)
        with Log(lib) as gf:
            tl, tp, loss = [v.clone() for v in eng.forward_train(feat, lab, seed=TSEED, sample_offset=TOFF)]
        kept = [(eng.node_output(n, batch, True) > 0).cpu() for n in eng.relu_nodes]
        with Log(lib) as gb:
            g1 = eng.backward().clone()
    finally:
        lib.tcr_tune(TCR_TUNE_BWD_MASK, 0)
    assert_launches(lib, row, (ge, gf, gb), swap={"chan_reduce_kernel": "chan_reduce4_kernel"})
    errs = {}
    out, model, grads = oracle_train(st, kept, 0.0, errs, name)
    errs["train_logits"] = float(np.abs(tl.cpu().numpy() - out["logits"]).max())
    errs["loss"] = abs(float(loss) / batch - model)
    assert errs["train_logits"] < Cm.LOGIT_TOL and errs["loss"] < LOSS_TOL, errs
    errs["stats"] = stat_errors(lambda k: eng._view(k).cpu().numpy(), out["new_stats"], name)
    errs["grads"] = grad_errors(lambda k: eng.grad_view(k).cpu().numpy(), eng.tensors, grads, name)
    record("knob", lib, name + "_chan_reduce4", errs)


def test_chan_reduce4_through_its_knob(emu_lib):
    check_chan_reduce4(emu_lib)


@pytest.mark.gpu
def test_gpu_chan_reduce4_through_its_knob(hip_lib):
    check_chan_reduce4(hip_lib)


def check_staged(lib):
    """The cross-replica BN hand-off (tcr_g2d_*_stage, identity hook) on a row at two filter-gradient chunks: bitwise the unstaged step;
    chan_sums_kernel is what hands the sums over."""
    row = ROW[STAGED_ROW]
    st = row_setup(lib, row)
    eng = st["eng"]
    feat, lab = planar(lib, st["x"]), Cm.to_dev(lib, st["labels"])
    outs, seen = [], []
    for hook in (None, lambda sums: seen.append(sums.numel())):
        eng.load_state_dict(st["sd"])
        with Log(lib) as g:
            logits, probs, loss = eng.forward_train(feat, lab, seed=TSEED, sync_hook=hook)
            grads = eng.backward().clone()
        outs.append((logits.clone(), probs.clone(), loss.clone(), grads, eng.stats.clone()))
    if lib.kind == "emu":
        assert g.has("chan_sums_kernel")
        LAUNCHED.update(kernel_of(e) for e in g.entries)
    assert len(seen) == 2 * (lib.tcr_g2d_num_stages(eng._h) - 1) > 0
    for a, c, what in zip(outs[0], outs[1], ("logits", "probs", "loss", "grads", "moving stats")):
        assert torch.equal(a, c), f"staged {what} differ from the unstaged run"


def test_staged_equals_unstaged(emu_lib):
    check_staged(emu_lib)


@pytest.mark.gpu
def test_gpu_staged_equals_unstaged(hip_lib):
    check_staged(hip_lib)


# ---- shards ---------------------------------------------------------------------------------------------------------------------------
def check_shards(lib):
    """"A sharded batch draws the same mask" (eltwise2d_kernel) and head2d_kernel's 1 / global_batch: a BN-free graph with dropout at
    batch 6, whole and as two shards of 3 with global_batch = 6 and sample offsets 0 and 3 -- each shard's logits bitwise the whole
    run's rows, the shards' gradients summing to the whole run's (each to GRAD_RTOL of the oracle's whole-batch gradient)."""
    row = ROW[SHARD_ROW]
    name, h, w, batch = row[:4]
    st = row_setup(lib, row)
    st["masks"] = masks_of(st["eng"], st["spec"], batch, off=0)
    eng = st["eng"]
    feat, lab = planar(lib, st["x"]), Cm.to_dev(lib, st["labels"])
    tl, _, loss = [v.clone() for v in eng.forward_train(feat, lab, seed=TSEED, sample_offset=0)]
    kept = [(eng.node_output(n, batch, True) > 0).cpu() for n in eng.relu_nodes]
    whole = eng.backward().clone()
    total, losses = torch.zeros_like(whole), 0.0
    for off in (0, 3):
        sl, _, slo = eng.forward_train(feat[off:off + 3].contiguous(), lab[off:off + 3].contiguous(), seed=TSEED, sample_offset=off, global_batch=batch)
        assert torch.equal(sl, tl[off:off + 3]), (name, "shard at", off, "logits differ from the whole run's rows")
        total += eng.backward()
        losses += float(slo)
    assert abs(losses - float(loss)) < LOSS_TOL * batch
    errs = {}
    _out, _model, grads = oracle_train(st, kept, 0.0, errs, name)
    view = lambda arena, k: arena.cpu().numpy()[eng.tensors[k].offset:eng.tensors[k].offset + eng.tensors[k].size]
    errs["grads"] = grad_errors(lambda k: view(whole, k), eng.tensors, grads, name)
    errs["shard_grads"] = grad_errors(lambda k: view(total, k), eng.tensors, grads, name + " (sum of the shards)")
    errs["shards_vs_whole"] = max(float(np.abs(view(total, k) - view(whole, k)).max() / max(np.abs(view(whole, k)).max(), 1e-3)) for k in grads)
    assert errs["shards_vs_whole"] < GRAD_RTOL, (name, errs)
    record("shards", lib, name, errs)


def test_shards_draw_the_whole_batchs_masks(emu_lib):
    check_shards(emu_lib)


@pytest.mark.gpu
def test_gpu_shards_draw_the_whole_batchs_masks(hip_lib):
    check_shards(hip_lib)


# ---- writes stay inside what the API declares; pointers one float off ----------------------------------------------------------------
def abi_steps(lib, row, st, shift):
    """tcr_g2d_forward_infer / _forward_train / _backward through the C ABI: every buffer a call writes exactly as large as declared (the
    workspaces: tcr_g2d_workspace_bytes, passed as their size) between guard regions, `shift` floats behind a 16-byte boundary; with a
    shift the read-only operands (parameters, input plane, labels) move as well."""
    name, batch = row[0], row[3]
    eng = st["eng"]
    nc, h = eng.num_classes, eng._h
    x0 = eng.input_from_features(planar(lib, st["x"]))
    sizes = (("logits", batch * nc), ("probs", batch * nc), ("loss", 1), ("grads", eng.n_param), ("stats", eng.n_stat),
             ("ws0", lib.tcr_g2d_workspace_bytes(h, batch, 0) // 4), ("ws1", lib.tcr_g2d_workspace_bytes(h, batch, 1) // 4))
    bufs = {k: Guarded(lib, n, shift) for k, n in sizes}
    assert bufs["ws0"].n > 0 and bufs["ws1"].n > bufs["ws0"].n
    bufs["stats"].body.copy_(eng.stats)
    ro = {"params": Guarded(lib, eng.n_param, shift), "x": Guarded(lib, x0.numel(), shift), "labels": Guarded(lib, batch * nc, shift)}
    for k, src in (("params", eng.params), ("x", x0.reshape(-1)), ("labels", Cm.to_dev(lib, st["labels"]).reshape(-1))):
        ro[k].body.copy_(src)
    every = dict(bufs, **ro)
    assert all(b.ptr() % 16 == 4 * shift for b in every.values())
    stream = eng._stream()

    def intact(call):
        bad = [k for k, b in every.items() if not b.intact()]
        assert not bad, (name, call, "wrote outside", bad)

    def short(rc, call):
        assert rc < 0 and b"workspace" in lib.tcr_last_error(), (name, call, rc, lib.tcr_last_error())

    ws = bufs["ws0"]
    infer = lambda nbytes: lib.tcr_g2d_forward_infer(h, ro["params"].ptr(), bufs["stats"].ptr(), ro["x"].ptr(), batch, ws.ptr(), nbytes,
                                                     bufs["logits"].ptr(), bufs["probs"].ptr(), stream)
    short(infer(ws.n * 4 - 4), "tcr_g2d_forward_infer")         # a DECLARED size one float short is refused before anything is launched
    with Log(lib) as ge:
        lib.check(infer(ws.n * 4), "tcr_g2d_forward_infer")
    intact("tcr_g2d_forward_infer")
    ev = (bufs["logits"].body.clone(), bufs["probs"].body.clone())
    ws = bufs["ws1"]
    train = lambda nbytes: lib.tcr_g2d_forward_train(h, ro["params"].ptr(), bufs["stats"].ptr(), ro["x"].ptr(), ro["labels"].ptr(), batch, batch, TSEED,
                                                     TOFF, 0.0, ws.ptr(), nbytes, bufs["logits"].ptr(), bufs["probs"].ptr(), bufs["loss"].ptr(), stream)
    back = lambda nbytes: lib.tcr_g2d_backward(h, ro["params"].ptr(), ro["x"].ptr(), batch, TSEED, TOFF, ws.ptr(), nbytes, bufs["grads"].ptr(), stream)
    short(train(ws.n * 4 - 4), "tcr_g2d_forward_train")
    with Log(lib) as gf:
        lib.check(train(ws.n * 4), "tcr_g2d_forward_train")
    intact("tcr_g2d_forward_train")
    short(back(ws.n * 4 - 4), "tcr_g2d_backward")
    with Log(lib) as gb:
        lib.check(back(ws.n * 4), "tcr_g2d_backward")
    intact("tcr_g2d_backward")
    return bufs, ev, (ge, gf, gb)


def node_act(lib, eng, ws, node, batch):
    """A node's training activation in a caller's workspace (tcr_g2d_node_output)."""
    off, plane, halo = C.c_int64(), C.c_int64(), C.c_int()
    lib.check(lib.tcr_g2d_node_output(eng._h, node, batch, 1, C.byref(off), C.byref(plane), C.byref(halo)), "tcr_g2d_node_output")
    c, h, w = eng.shape(node)
    return ws.body[off.value:off.value + batch * c * plane.value].view(batch, c, plane.value)[:, :, halo.value:halo.value + h * w].reshape(batch, c, h, w)


def check_guards(lib, row):
    """The three passes through the C ABI between guard regions: the guards keep their pattern, the results are bitwise the engine's
    own, and the gradient arena -- handed over full of the pattern -- comes back zero outside the tensors."""
    name, batch = row[0], row[3]
    st = row_setup(lib, row)
    eng = st["eng"]
    nc = eng.num_classes
    feat, lab = planar(lib, st["x"]), Cm.to_dev(lib, st["labels"])
    want_eval = [v.clone() for v in eng.forward_infer(feat)]
    stats0 = eng.stats.clone()
    want_train = [v.clone() for v in eng.forward_train(feat, lab, seed=TSEED, sample_offset=TOFF)]
    want_grads = eng.backward().clone()
    want_stats = eng.stats.clone()
    eng.stats.copy_(stats0)
    bufs, ev, _ = abi_steps(lib, row, st, 0)
    assert torch.equal(ev[0].view(batch, nc), want_eval[0]) and torch.equal(ev[1].view(batch, nc), want_eval[1]), (name, "tcr_g2d_forward_infer")
    assert torch.equal(bufs["logits"].body.view(batch, nc), want_train[0]) and torch.equal(bufs["probs"].body.view(batch, nc), want_train[1])
    assert float(bufs["loss"].body[0]) == float(want_train[2]) and torch.equal(bufs["stats"].body, want_stats), (name, "tcr_g2d_forward_train")
    got = bufs["grads"].body
    assert torch.equal(got, want_grads), (name, "tcr_g2d_backward", float((got - want_grads).abs().max()))
    pads = pad_mask(eng)
    assert int(pads.sum()) >= 64 and not bool(got.cpu()[pads].any()), (name, "gradient arena not zero outside its tensors")


@pytest.mark.parametrize("name", GUARD_ROWS)
def test_writes_stay_inside_declared_buffers(emu_lib, name):
    check_guards(emu_lib, ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GUARD_ROWS)
def test_gpu_writes_stay_inside_declared_buffers(hip_lib, name):
    check_guards(hip_lib, ROW[name])


def check_unaligned(lib, name):
    """Every pointer of the three passes one float behind a 16-byte boundary (a C-ABI caller owes the library 4-byte alignment only):
    against the oracle with the rows' tolerances (not bitwise: the BN forms change their summation order), guards intact, and on the
    emulator the BN forms that ran are the scalar ones."""
    row = ROW[name]
    batch = row[3]
    st = row_setup(lib, row)
    eng, nc = st["eng"], st["eng"].num_classes
    bufs, ev, logs = abi_steps(lib, row, st, 1)
    assert_launches(lib, row, logs, aligned=False, abi=True)
    if lib.kind == "emu":
        ran = {kernel_of(e) for g in logs for e in g.entries}
        assert not ran & {"bn_apply4_kernel", "chan_reduce4_kernel", "bn_bwd_apply4_kernel", "bn_bwd_apply4x_kernel"}, sorted(ran)
    ref = oracle_eval(st)
    errs = {"eval_logits": float(np.abs(ev[0].view(batch, nc).cpu().numpy() - ref["logits"]).max()),
            "eval_probs": float(np.abs(ev[1].view(batch, nc).cpu().numpy() - ref["probs"]).max())}
    assert errs["eval_logits"] < Cm.LOGIT_TOL and errs["eval_probs"] < PROB_TOL, (name, "unaligned eval", errs)
    assert np.array_equal(ev[0].view(batch, nc).cpu().numpy().argmax(1), ref["logits"].argmax(1))
    kept = [(node_act(lib, eng, bufs["ws1"], n, batch) > 0).cpu() for n in eng.relu_nodes]
    out, model, grads = oracle_train(st, kept, 0.0, errs, name)
    errs["train_logits"] = float(np.abs(bufs["logits"].body.view(batch, nc).cpu().numpy() - out["logits"]).max())
    errs["train_probs"] = float(np.abs(bufs["probs"].body.view(batch, nc).cpu().numpy() - out["probs"]).max())
    errs["loss"] = abs(float(bufs["loss"].body[0]) / batch - model)
    assert errs["train_logits"] < Cm.LOGIT_TOL and errs["train_probs"] < PROB_TOL and errs["loss"] < LOSS_TOL, (name, "unaligned train", errs)
    view = lambda arena, k: arena.cpu().numpy()[eng.tensors[k].offset:eng.tensors[k].offset + eng.tensors[k].size]
    errs["stats"] = stat_errors(lambda k: view(bufs["stats"].body, k), out["new_stats"], name + " (unaligned)")
    errs["grads"] = grad_errors(lambda k: view(bufs["grads"].body, k), eng.tensors, grads, name + " (unaligned)")
    record("unaligned", lib, name, errs)


@pytest.mark.parametrize("name", UNALIGNED_ROWS)
def test_pointers_one_float_off(emu_lib, name):
    check_unaligned(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNALIGNED_ROWS)
def test_gpu_pointers_one_float_off(hip_lib, name):
    check_unaligned(hip_lib, name)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    """The construction-time TCR_REQUIREs of net2d.cpp: a negative status with a message, nothing added to the graph, and the graph goes
    on to finalize and run (or is destroyed as it stands)."""
    dev = Cm.device_of(lib)

    def refused(call, *what):
        with pytest.raises(T.TcrError) as e:
            call()
        assert all(w in str(e.value) for w in what), str(e.value)
        assert all(w.encode() in lib.tcr_last_error() for w in what)

    g = T.Graph2D("", 6, 5, 1, lib=lib, device=dev)
    refused(lambda: g.conv(-1, (3, 3), 4, "w", stride=(2, 1), rate=(1, 2)), "tcr_g2d_conv", "dilation needs stride 1")
    refused(lambda: g.conv(-1, (3, 3), 4, "w", stride=(2, 2), rate=(2, 2)), "dilation needs stride 1")
    refused(lambda: g.conv(-1, (7, 3), 4, "w", padding="VALID"), "7x3 kernel does not fit the 6x5 input")
    refused(lambda: g.conv(-1, (2, 2), 4, "w", rate=(1, 5), padding="VALID"), "does not fit")          # (the dilated extent: 1 + 5 > 5)
    refused(lambda: g.conv(-1, (3, 3), 0, "w"), "tcr_g2d_conv: bad argument")
    refused(lambda: g.conv(-1, (3, 3), 4, "w", stride=(0, 1)), "tcr_g2d_conv: bad argument")
    refused(lambda: g.conv(0, (3, 3), 4, "w"), "tcr_g2d_conv", "bad graph / input id")               # (no node 0 yet)
    refused(lambda: g.pool(-1, "max", (2, 6), (1, 1), "VALID"), "tcr_g2d_pool", "2x6 window does not fit the 6x5 input")
    refused(lambda: g.pool(-1, "avg", (2, 2), (0, 1), "VALID"), "tcr_g2d_pool: bad stride")
    refused(lambda: g.batch_norm(-1, "in/BatchNorm"), "tcr_g2d_batch_norm: bad argument")               # BN on the network input
    refused(lambda: g.dropout(-1, 0.5), "tcr_g2d_dropout: bad argument")                                # dropout on the network input
    refused(lambda: g.group_sum(-1, 1), "tcr_g2d_group_sum", "1 x 1 input")                             # (6 x 5)
    with pytest.raises(T.TcrError, match="tcr_g2d_finalize"):
        g.finalize(0)                                                                                   # nothing to finalize yet
    assert not g.finalized
    a = g.conv(-1, (3, 3), 6, "a/weights", relu=True)
    b = g.conv(a, (3, 3), 6, "b/weights", stride=(2, 2))
    c = g.conv(a, (3, 3), 5, "c/weights")
    assert (a, b, c) == (0, 1, 2)                                                                       # the refusals added nothing
    refused(lambda: g.add(a, b), "tcr_g2d_add: shapes differ (6,6,5) vs (6,3,3)")
    refused(lambda: g.add(a, c), "shapes differ (6,6,5) vs (5,6,5)")
    refused(lambda: g.add(a, -1), "tcr_g2d_add: the network input cannot be an operand")
    refused(lambda: g.add(-1, a), "the network input cannot be an operand")
    refused(lambda: g.add(a, 7), "tcr_g2d_add", "bad graph / input id")
    refused(lambda: g.group_sum(a, 2), "tcr_g2d_group_sum: needs a 1 x 1 input")                        # not 1 x 1
    for keep in (0.0, -0.5, 1.5):
        refused(lambda: g.dropout(a, keep), "tcr_g2d_dropout: bad argument")
    refused(lambda: g.time_filter(a, ""), "tcr_g2d_time_filter: the variable needs a name")
    p = g.pool(a, "avg")
    assert g.shape(p) == (6, 1, 1)
    refused(lambda: g.group_sum(p, 4), "6 channels divide by the group 4")
    refused(lambda: g.group_sum(p, 0), "tcr_g2d_group_sum")
    refused(lambda: g.finalize(a), "tcr_g2d_finalize: the logits node must be 1 x 1 spatially (got 6 x 5)")
    refused(lambda: g.finalize(9), "tcr_g2d_finalize: bad argument")
    assert not g.finalized and lib.tcr_g2d_workspace_bytes(g._h, 2, 0) == 0
    d = g.dropout(g.group_sum(p, 3, biases_name="bias"), 1.0)                                           # keep_prob exactly 1 is allowed
    g.finalize(g.conv(d, (1, 1), 12, "fc/weights", biases_name="fc/biases"))
    # ... after finalize: every builder call and a second finalize
    for call in (lambda: g.conv(a, (3, 3), 4, "late"), lambda: g.batch_norm(a, "late/BatchNorm"), lambda: g.pool(a, "max"), lambda: g.add(a, a),
                 lambda: g.dropout(a, 0.5), lambda: g.time_filter(a, "late"), lambda: g.group_sum(p, 1)):
        refused(call, "bad graph / input id")
    refused(lambda: g.finalize(p), "tcr_g2d_finalize: bad argument")
    assert lib.tcr_g2d_num_tensors(g._h) == len(g.tensors) == 6
    # the graph still runs, and gives what the oracle gives for what was accepted
    s = Spec()
    sa = s.conv(-1, (3, 3), 6, relu=True)
    s.conv(sa, (3, 3), 6, stride=(2, 2))
    s.conv(sa, (3, 3), 5)
    sl = s.conv(s.dropout(s.gsum(s.pool(sa, "avg"), 3, bias=True), 1.0), (1, 1), 12, bias=True)
    names = dict(zip(["n0/weights", "n1/weights", "n2/weights", "n4/bias", "n6/weights", "n6/biases"],
                     ["a/weights", "b/weights", "c/weights", "bias", "fc/weights", "fc/biases"]))
    sd = _randomise(g, 3)
    p64, stats = _split(g, sd)
    x = features(3, 6, 5)
    ref = O.graph_forward({"nodes": s.nodes, "logits": sl}, {k: torch.tensor(p64[v]) for k, v in names.items()}, stats, torch.tensor(x.astype(np.float64)))
    logits, _ = g.forward_infer(planar(lib, x))
    assert float(np.abs(logits.cpu().numpy() - ref["logits"].numpy()).max()) < Cm.LOGIT_TOL
    # a graph that met only refusals is destroyed as it stands
    g2 = T.Graph2D("", 2, 2, 1, lib=lib, device=dev)
    refused(lambda: g2.conv(-1, (3, 3), 4, "w", padding="VALID"), "3x3 kernel does not fit the 2x2 input")
    del g2
    for bad in ((0, 5, 1), (6, 0, 1), (6, 5, 0)):
        with pytest.raises(T.TcrError, match="tcr_g2d_create: bad argument"):
            T.Graph2D("", *bad, lib=lib, device=dev)


def test_refusals(emu_lib):
    check_refusals(emu_lib)


# ---- the detection stack on a graph that is no factory model ------------------------------------------------------------------------------
def check_detection_stack(lib, n_streams):
    """A graph none of the factories builds -- a conv of stride (2, 3), a SAME max pool of overlapping windows -- behind a 40 ms / 20 ms
    front-end (49 frames x 10 coefficients): every push's logits / probabilities are bitwise forward_infer of the stream windows, and a
    short scan is bitwise the pushes (tests/test_net_configs.py::check_detection_stack's scheme)."""
    from tests import test_detect_families as TD
    from tests.test_scan import assert_bitwise, pushed
    from tests.test_streaming import segment_audio
    fe = Cm.make_frontend(lib, 640, 320, num_mfccs=10)
    assert (fe.n_frames, fe.n_coef) == (49, 10)
    net = build_graph(lib, graph(_detect), fe.n_frames, fe.n_coef)
    TD.randomise(net, 2)
    TD.run_pushes(lib, fe, net, n_streams, 1, 3, {2: [1]}, average_window_ms=60, min_count=1, suppression_ms=40, detection_threshold=0.0)
    dkw = dict(average_window_ms=60, min_count=2, detection_threshold=0.0, suppression_ms=80)
    audio = Cm.to_dev(lib, segment_audio(n_streams, 5 * fe.cfg.hop, 3))
    want = pushed(TD.streaming().StreamingDetector(net, fe, n_streams, frames_per_step=1, **dkw), audio)
    assert_bitwise(TD.scanner(net, fe, 1, **dkw).scan(audio), want)
    assert_bitwise(TD.scanner(net, fe, 1, max_windows=4, **dkw).scan(audio), want)
    feat = fe(Cm.to_dev(lib, segment_audio(2, fe.n_samples, 5)))
    sd = {k: v for k, v in net.state_dict().items()}
    p64, stats = _split(net, sd)
    x = feat[:, :, HALO:HALO + fe.n_frames].permute(0, 2, 1).cpu().numpy().astype(np.float64)
    ref = O.graph_forward(graph(_detect), {k: torch.tensor(v) for k, v in p64.items()}, stats, torch.tensor(x))
    assert float(np.abs(net.forward_infer(feat)[0].cpu().numpy() - ref["logits"].numpy()).max()) < Cm.LOGIT_TOL


def test_detection_stack_on_a_custom_graph(emu_lib):
    check_detection_stack(emu_lib, 2)


@pytest.mark.gpu
def test_gpu_detection_stack_on_a_custom_graph(hip_lib):
    check_detection_stack(hip_lib, 64)
