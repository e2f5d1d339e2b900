"""Float64 reference of graphs that hold depthwise convolutions (tests/test_g2d_dw.py): oracle.net2d_ref's pieces -- conv2d, batch_norm,
the pools, _same_pads, _relu, the dropout masks -- plus `dwconv`, tf.nn.depthwise_conv2d with channel multiplier 1 written as
F.conv2d(groups=C) under TF's SAME rule; and an int64 restatement of the forward sum for the exact checks."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import net2d_ref as O


def dwconv(x, w_hwc1, stride=(1, 1), rate=(1, 1), padding="SAME", bias=None):
    """x [N, C, H, W], w [kh, kw, C, 1] (TF's depthwise filter layout at multiplier 1)."""
    kh, kw, c, mult = w_hwc1.shape
    assert mult == 1 and c == x.shape[1], (tuple(w_hwc1.shape), tuple(x.shape))
    if padding == "SAME":
        pt, pb = O._same_pads(x.shape[2], (kh - 1) * rate[0] + 1, stride[0])
        pl, pr = O._same_pads(x.shape[3], (kw - 1) * rate[1] + 1, stride[1])
        x = F.pad(x, (pl, pr, pt, pb))
    return F.conv2d(x, w_hwc1.permute(2, 3, 0, 1), bias, stride=stride, dilation=rate, groups=c)


def graph_forward(spec, params, stats, x, is_training=False, masks=None):
    """oracle.net2d_ref.graph_forward's node list with one more op,
      dwconv    in, k (kh, kw), stride, rate, pad, relu, w, b
    x is [N, H, W] (one input channel) or [N, C, H, W]."""
    new_stats = dict(stats)
    drop = O._Masks(masks)
    x4 = x.unsqueeze(1) if x.dim() == 3 else x
    outs = []
    val = lambda i: x4 if i < 0 else outs[i]
    for n in spec["nodes"]:
        op = n["op"]
        bias = params[n["b"]] if op in ("conv", "dwconv") and n.get("b") else None
        if op == "conv":
            y = O.conv2d(val(n["in"]), params[n["w"]], tuple(n["stride"]), tuple(n["rate"]), n["pad"], bias)
        elif op == "dwconv":
            y = dwconv(val(n["in"]), params[n["w"]], tuple(n["stride"]), tuple(n["rate"]), n["pad"], bias)
        elif op == "bn":
            y = O.batch_norm(val(n["in"]), n["prefix"], params, stats, new_stats, is_training, n.get("decay", 0.997), n.get("eps", 0.001),
                             n["center"], n["scale"])
        elif op == "pool":
            h = val(n["in"])
            k = tuple(n["k"]) if n.get("k") else tuple(h.shape[2:])
            stride, pad = (tuple(n["stride"]), n["pad"]) if n.get("k") else ((1, 1), "VALID")
            y = O.max_pool(h, k, stride, pad) if n["kind"] == "max" else O.avg_pool(h, k, stride, pad)
        elif op == "add":
            y = val(n["a"]) + val(n["b"])
        elif op == "dropout":
            y = drop.apply(val(n["in"]), n["keep"], is_training)
        else:
            raise ValueError(op)
        outs.append(O._relu(y) if n.get("relu") else y)
    logits = outs[spec["logits"]].flatten(1)
    return {"logits": logits, "probs": F.softmax(logits, dim=-1), "new_stats": new_stats}


def out_dim(length, k_eff, stride, pad):
    """(output size, leading pad) of one dimension, TF's rule."""
    if pad == "VALID":
        return (length - k_eff) // stride + 1, 0
    return -(-length // stride), O._same_pads(length, k_eff, stride)[0]


def dw_int64(x, w, stride, rate, pad):
    """The forward sum on integers: x [N, C, H, W] int64, w [kh, kw, C] int64 -> [N, C, OH, OW] int64, one term per tap."""
    n, c, h, wd = x.shape
    kh, kw = w.shape[:2]
    oh, pt = out_dim(h, (kh - 1) * rate[0] + 1, stride[0], pad)
    ow, pl = out_dim(wd, (kw - 1) * rate[1] + 1, stride[1], pad)
    y = np.zeros((n, c, oh, ow), dtype=np.int64)
    for oy in range(oh):
        for ox in range(ow):
            for i in range(kh):
                for j in range(kw):
                    sy, sx = oy * stride[0] + i * rate[0] - pt, ox * stride[1] + j * rate[1] - pl
                    if 0 <= sy < h and 0 <= sx < wd:
                        y[:, :, oy, ox] += x[:, :, sy, sx] * w[i, j][None, :]
    return y
