"""A configurable DS-CNN ("Hello Edge" depthwise-separable CNN) on the generic 2-D graph engine: the topology of the DS-CNN S / M / L
model classes -- conv_1 + bias, BN without scale, ReLU; per block a depthwise conv + bias, BN, ReLU and a pointwise conv + bias, BN,
ReLU; global average pool; fc1 -- with every size free: depth, block count, conv_1's kernel and stride, the depthwise kernel, the first
block's stride, a dilation.  The dedicated engine (engine.DSCNN) keeps the three published sizes and is faster on them; this builder is
for what it refuses (INTEGRATION.md "Model families").

Variables carry the names of the DS-CNN engine -- `DSCNN/conv_1/{weights,biases}`, `DSCNN/conv_1/batch_norm/*`,
`DSCNN/conv_ds_k/depthwise_conv/{depthwise_weights,biases}`, `.../dw_batch_norm/*`, `.../pointwise_conv/{weights,biases}`,
`.../pw_batch_norm/*`, `DSCNN/fc1/{weights,biases}` -- so a `state_dict` of one loads into the other."""
from __future__ import annotations

from typing import Sequence, Tuple, Union

from .. import runtime
from ..engine import Graph2D
from . import tc_resnet

BN_DECAY, BN_EPS = 0.96, 0.001

Pair = Union[str, int, Sequence[int]]


def pair(v: Pair) -> Tuple[int, int]:
    """"10x4" | 3 | (3, 3) -> (h, w)."""
    if isinstance(v, str):
        a, _, b = v.lower().partition("x")
        return int(a), int(b or a)
    if isinstance(v, int):
        return v, v
    return int(v[0]), int(v[1])


def build_dscnn(g: Graph2D, num_classes: int, depth: int, num_separable: int, conv1_kernel: Pair = (10, 4), conv1_stride: Pair = (2, 2),
                ds_kernel: Pair = (3, 3), ds1_stride: Pair = (1, 1), ds_rate: Pair = (1, 1), scope: str = "DSCNN") -> int:
    """The nodes of one DS-CNN; returns the logits node.  A dilated depthwise kernel needs ds1_stride 1x1 (the node's rule)."""
    bn = lambda x, prefix: g.batch_norm(x, prefix, center=True, scale=False, relu=True, decay=BN_DECAY, eps=BN_EPS)
    net = g.conv(-1, pair(conv1_kernel), depth, f"{scope}/conv_1/weights", stride=pair(conv1_stride), biases_name=f"{scope}/conv_1/biases")
    net = bn(net, f"{scope}/conv_1/batch_norm")
    for i in range(1, num_separable + 1):
        pre = f"{scope}/conv_ds_{i}"
        net = g.depthwise_conv(net, pair(ds_kernel), f"{pre}/depthwise_conv/depthwise_weights", stride=pair(ds1_stride) if i == 1 else (1, 1),
                               rate=pair(ds_rate), biases_name=f"{pre}/depthwise_conv/biases")
        net = bn(net, f"{pre}/dw_batch_norm")
        net = g.conv(net, 1, depth, f"{pre}/pointwise_conv/weights", biases_name=f"{pre}/pointwise_conv/biases")
        net = bn(net, f"{pre}/pw_batch_norm")
    net = g.pool(net, "avg", None)
    # fc1 [depth, num_classes] is the 1 x 1 conv over the pooled node (Graph2D._fit reshapes a loaded matmul weight)
    return g.conv(net, 1, num_classes, f"{scope}/fc1/weights", biases_name=f"{scope}/fc1/biases", tf_shape=(depth, num_classes))


def build_graph(depth: int, num_separable: int, conv1_kernel: Pair, conv1_stride: Pair, ds_kernel: Pair, ds1_stride: Pair, ds_rate: Pair,
                h: int, w: int, num_classes: int, lib=None, device=None) -> Graph2D:
    """A finalized Graph2D of the DS-CNN so defined on an [h x w] feature plane."""
    if depth < 1 or num_separable < 0:
        raise ValueError(f"DS-CNN of depth {depth} with {num_separable} separable blocks")
    g = Graph2D("DSCNN", int(h), int(w), 1, lib=lib if lib is not None else runtime.default_lib(),
                device=device if device is not None else runtime.default_device())
    g.finalize(build_dscnn(g, int(num_classes), int(depth), int(num_separable), conv1_kernel, conv1_stride, ds_kernel, ds1_stride, ds_rate))
    return g


def get_engine(depth: int, num_separable: int, conv1_kernel: Pair, conv1_stride: Pair, ds_kernel: Pair, ds1_stride: Pair, ds_rate: Pair,
               h: int, w: int, num_classes: int) -> Graph2D:
    """build_graph, once per definition and shape (cached like the other families' engines)."""
    key = ("DSCNNGraph", int(depth), int(num_separable), pair(conv1_kernel), pair(conv1_stride), pair(ds_kernel), pair(ds1_stride), pair(ds_rate),
           int(h), int(w), int(num_classes), id(runtime.default_lib()))
    eng = tc_resnet._engines.get(key)
    if eng is None:
        eng = build_graph(depth, num_separable, conv1_kernel, conv1_stride, ds_kernel, ds1_stride, ds_rate, h, w, num_classes)
        tc_resnet._engines[key] = eng
    return eng
