"""The DS-CNN kernels across the network's configuration space: depths, separable-block counts, conv_1 kernel heights, strides, frame and
coefficient counts, label sets, batches and pointer alignments away from S / M / L at 49 x 10 x 12, so that every fallback and generic
kernel form is compared with the float64 oracle (oracle/dscnn_ref.py) at a shape where it is what runs BY DEFAULT -- eval logits /
probabilities / argmax, train-mode logits / loss / EVERY gradient / moving statistics, one Adam step, run-to-run reproducibility; which
kernel families ran, from the emulator's launch log; writes outside what the C ABI declares; the limits of the training kernels as
refusals; the detection stack on a non-flagship DS-CNN.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`): the same rows, shapes and
batches (the dispatch is host code)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import dscnn_ref as D
from oracle import numpy_ref as R
from tests import common as Cm
from tests.test_net_configs import GRAD_RTOL, MIN_BN_POSITIONS, OPT_TOL, PROB_TOL, STAT_TOL, Guarded, Log, kernel_of, launch_log  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_TOL = 1e-4
TCR_ERR_ARG = -1            # include/tcresnet_hip.h
NEAR = 1e-5                 # ReLU inputs this close to zero: the oracle takes the kernels' side (tcr_dscnn_unit_output)

# net definitions (depth, separable blocks, conv_1 stride, conv_ds_1 stride[, conv_1 kernel height]): engine.DSCNN(net_def=) and
# oracle.dscnn_ref.blocks_from_def take the same tuple
S, M, L = D.SIZE_DEFS["S"], D.SIZE_DEFS["M"], D.SIZE_DEFS["L"]


def m2(depth):              # M-shaped (conv_1 (2,1), conv_ds_1 (2,2): the 25 x 10 -> 13 x 5 maps at 49 x 10), two separable blocks
    return (depth, 2, (2, 1), (2, 2))


def s2(kh=10):              # S-shaped, two separable blocks
    return (64, 2, (2, 2), (1, 1), kh)


M112 = (112, 2, (2, 1), (2, 2))     # M-shaped at 7 tiles, two blocks: the pointwise kernels of 172 (lds6) at less emulator time

# (id, net definition, frames, coefficients, labels, batch, expected paths[, "eval"]).  "eval": the row cannot train (a declared limit,
# asserted as a refusal) and runs the eval checks only.
# Expected paths, one token per group (asserted from the emulator's launch log; a group left out of a row is not asserted):
#   conv1: loop / fused / alone = eval's conv_1: fused with the first depthwise layer in the loop form, in the generic fused form, or
#          dscnn_conv1_kernel alone (launch_dscnn_conv1_dw; the training forward always runs it alone)
#   dw / dwd / dww: rows / rows_s2 / lds2 / lds / plain, or mixed-<a>+<b>... = depthwise forward (eval and training), data gradient and
#          filter gradient over the separable layers (the filter gradient has no LDS form: rows / rows_s2 / plain)
#   pw:    lds6 / lds9 / mfma = the pointwise convs, forward and data gradient (conv1x1_lds_kernel's 6- and 9-tile instances, conv1x1_mfma_kernel)
#   pww:   lds / slices = the pointwise filter gradient: pw_wgrad_* (96-row blocks in LDS) or the generic 80-channel slices (conv_wgrad_mfma*)
#   pool:  block / plain = plane_mean_block_kernel / plane_mean_kernel (eval and training)
#   train: lazy / materialised = ds_lazy(): activations never written / normalised and stored per unit
LAZY_ROWS = "dw:mixed-rows+rows_s2 dwd:mixed-rows+rows_s2 dww:mixed-rows+rows_s2 pww:lds pool:block train:lazy"
S_PATHS = "conv1:fused dw:lds dwd:lds dww:plain pw:mfma pww:slices pool:block train:materialised"      # 25 x 5 maps, 64 channels
TINY = "conv1:fused dw:lds2 dwd:lds dww:plain pw:mfma pww:slices pool:block train:materialised"
ODD_PLANES = "conv1:loop dw:mixed-lds2+lds dwd:lds dww:mixed-rows+rows_s2 pww:lds pool:plain train:lazy"
ROWS = [
    # ---- anchors: S / M / L at 49 x 10 x 12.  Batch 3: 516 / 828 planes are no multiple of 16 -- the depthwise forward and data gradient
    # leave the `rows` kernels (the filter gradient's need c % 4 only), the pooling its block kernel; batch 4: 688 / 1104 planes.
    # ds_lazy() does not look at the batch: M and L train lazily at both.  S (64 channels: 4 tiles) trains on the materialising path.
    ("s_b3", S, 49, 10, 12, 3, S_PATHS),
    ("m_b3", M, 49, 10, 12, 3, "pw:lds6 " + ODD_PLANES),
    ("l_b3", L, 49, 10, 12, 3, "pw:lds9 " + ODD_PLANES),
    ("s_b4", S, 49, 10, 12, 4, S_PATHS),
    ("m_b4", M, 49, 10, 12, 4, "conv1:loop pw:lds6 " + LAZY_ROWS),
    ("l_b4", L, 49, 10, 12, 4, "conv1:loop pw:lds9 " + LAZY_ROWS),
    # ---- depth boundaries at 49 x 10, batch 4, two separable blocks: output tiles 1 (partial) / 2 / 5 / 6 | 7 (last tile 4 wide) / 12 |
    # 13 / 18 | 19; pw_wgrad_fits' cin, cout > 80 between 80 and 84; lazy only where conv1x1_lds_covers (7 .. 18 tiles).
    # 4 channels: below the rows kernels' 16 (forward, data gradient); the filter gradient's take any c % 4 == 0
    ("d4", m2(4), 49, 10, 12, 4, "conv1:loop dw:mixed-lds2+lds dwd:lds dww:mixed-rows+rows_s2 pw:mfma pww:slices pool:block train:materialised"),
    ("d20", m2(20), 49, 10, 12, 4, "conv1:loop dw:mixed-rows+rows_s2 dwd:mixed-rows+rows_s2 dww:mixed-rows+rows_s2 pw:mfma pww:slices pool:block train:materialised"),
    ("d80", m2(80), 49, 10, 12, 4, "conv1:loop dw:mixed-rows+rows_s2 dwd:mixed-rows+rows_s2 dww:mixed-rows+rows_s2 pw:mfma pww:slices pool:block train:materialised"),
    ("d84", m2(84), 49, 10, 12, 4, "conv1:loop dw:mixed-rows+rows_s2 dwd:mixed-rows+rows_s2 dww:mixed-rows+rows_s2 pw:mfma pww:lds pool:block train:materialised"),
    ("d96", m2(96), 49, 10, 12, 4, "conv1:loop dw:mixed-rows+rows_s2 dwd:mixed-rows+rows_s2 dww:mixed-rows+rows_s2 pw:mfma pww:lds pool:block train:materialised"),
    ("d100", m2(100), 49, 10, 12, 4, "conv1:loop pw:lds6 " + LAZY_ROWS),
    ("d192", m2(192), 49, 10, 12, 4, "conv1:loop pw:lds6 " + LAZY_ROWS),
    ("d196", m2(196), 49, 10, 12, 4, "conv1:loop pw:lds9 " + LAZY_ROWS),
    ("d288", m2(288), 49, 10, 12, 4, "conv1:loop pw:lds9 " + LAZY_ROWS),
    # 19 tiles: conv1x1_mfma_kernel at 6 tiles per wave, so no lazy training -- with the LDS pointwise filter gradient (292 > 80)
    ("d292", m2(292), 49, 10, 12, 4, "conv1:loop dw:mixed-rows+rows_s2 dwd:mixed-rows+rows_s2 dww:mixed-rows+rows_s2 pw:mfma pww:lds pool:block train:materialised"),
    # ---- frames.  98 (30 / 10 ms): conv_1's 49 x 10 = 490 positions run alone (> 256); a 112-deep M-shaped net then has 25 x 5 maps: a
    # padded plane of 133 floats > 74, so pw_wgrad_fits declines and the net trains MATERIALISED with lds6 pointwise convs
    ("t98_s", S, 98, 10, 12, 2, S_PATHS),
    ("t98_m112", M112, 98, 10, 12, 2, "conv1:alone dw:lds dwd:lds dww:plain pw:lds6 pww:slices pool:block train:materialised"),
    # 50 (even: conv_1 pads (4, 4) instead of (4, 5)); the M-shaped maps are the hard-coded ones again behind other pads
    ("t50_s", S, 50, 10, 12, 3, S_PATHS),
    ("t50_m112", M112, 50, 10, 12, 4, "conv1:loop pw:lds6 " + LAZY_ROWS),
    # maps smaller than every kernel window: all but one tap of the 10 x 4 conv in the padding
    ("t1_f1", S, 1, 1, 12, 9, TINY),
    ("t2_f3", S, 2, 3, 12, 9, TINY),
    ("t7_f4", S, 7, 4, 12, 9, TINY),
    # ---- coefficients
    ("f13_s", S, 49, 13, 12, 3, S_PATHS),
    # 25 x 40 -> 13 x 20: conv_1 alone (1000 positions); the first depthwise layer's 27 x 41 image and its data gradient's 27 x 42 exceed
    # 1024 elements (64 KB for 16 planes): the plain one-wave-per-plane kernels, whose only oracle comparison this is
    ("f40_m112", M112, 49, 40, 12, 2, "conv1:alone dw:mixed-lds+plain dwd:mixed-lds+plain dww:plain pw:lds6 pww:slices pool:block train:materialised"),
    # 40 x 106 = 4240 floats > 3072: eval only (49 x 20 maps: a 51 x 22 image, the plain depthwise kernel in eval)
    ("t98_f40_s", S, 98, 40, 12, 2, "conv1:alone dw:plain pw:mfma pool:block", "eval"),
    # ---- strides and structure.  (2,1) x (2,1): the <0, 0> instances of the depthwise gradients
    ("st11_12", (64, 2, (1, 1), (1, 2)), 21, 10, 12, 3, S_PATHS),
    ("st21_21", (64, 2, (2, 1), (2, 1)), 49, 10, 12, 3, S_PATHS),
    ("nsep1", (64, 1, (2, 2), (1, 1)), 49, 10, 12, 3, S_PATHS),
    ("nsep8", (64, 8, (2, 2), (1, 1)), 49, 10, 12, 3, S_PATHS),
    ("kh1", s2(1), 49, 10, 12, 3, S_PATHS),
    ("kh3", s2(3), 49, 10, 12, 3, S_PATHS),
    ("kh12", s2(12), 49, 10, 12, 3, S_PATHS),                   # exactly 48 taps
    ("kh13", s2(13), 49, 10, 12, 3, "conv1:fused dw:lds pw:mfma pool:block", "eval"),       # 52 taps: eval only
    ("kh16", s2(16), 49, 10, 12, 3, "conv1:fused dw:lds pw:mfma pool:block", "eval"),
    # ---- labels (46: the head's maximum)
    ("c2", s2(), 49, 10, 2, 3, S_PATHS),
    ("c35", s2(), 49, 10, 35, 3, S_PATHS),
    ("c46", s2(), 49, 10, 46, 3, S_PATHS),
    # ---- batches: 1, 17, 33 (dw_wgrad_chunks: 33 utterances = chunks of 17 and 16) on an S-wide net (the plain filter gradient) and on
    # a 112-deep M-shaped one (the rows filter gradients; 112 b planes are a multiple of 16 at every batch: the rows forward kernels too)
    ("s_b1", s2(), 49, 10, 12, 1, S_PATHS),
    ("s_b17", s2(), 49, 10, 12, 17, S_PATHS),
    ("s_b33", s2(), 49, 10, 12, 33, S_PATHS),
    ("w112_b1", M112, 49, 10, 12, 1, "conv1:loop pw:lds6 " + LAZY_ROWS),
    ("w112_b17", M112, 49, 10, 12, 17, "conv1:loop pw:lds6 " + LAZY_ROWS),
    ("w112_b33", M112, 49, 10, 12, 33, "conv1:loop pw:lds6 " + LAZY_ROWS),
]
ROW_IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}

OPTIM_ROWS = ["s_b3", "d292"]                                   # one Adam step (a lazy-free small net, a materialised wide one)
GUARD_ROWS = ["t1_f1", "f40_m112", "m_b4"]                      # writes outside the declared buffers
# C-ABI calls whose every pointer starts one float behind a 16-byte boundary: {row: paths that differ from the row's aligned ones}
OFF16 = {"dw": "mixed-lds2+lds", "dwd": "lds", "dww": "plain", "pool": "plain"}
UNALIGNED_ROWS = {"m_b4": OFF16, "d196": OFF16}

# every launch name a row met (emulator): test_every_dscnn_launch_is_covered reads it after the rows have run
LAUNCHED = set()
# check_launch names of dscnn.hip / dscnn_bwd.hip that no row may reach, each with its reason
EXEMPT = {}


def paths_of(row):
    return dict(tok.split(":") for tok in row[6].split())


def trains(row):
    return len(row) < 8 or row[7] != "eval"


def blocks_of(row):
    return D.blocks_from_def(*row[1])


def shapes_of(row):
    """[(h, w)] of conv_1's and every separable block's output map."""
    h, w, out = row[2], row[3], []
    for b in blocks_of(row):
        h, w = -(-h // b.stride[0]), -(-w // b.stride[1])
        out.append((h, w))
    return out


def unit_keys(blocks):
    """(oracle cache key, BN scope) per BN unit, in the library's unit order."""
    keys = []
    for blk in blocks:
        keys += [(blk.scope + "/out", f"DSCNN/{blk.scope}/batch_norm")] if blk.type != "separable" else \
            [(blk.scope + "/mid", f"DSCNN/{blk.scope}/dw_batch_norm"), (blk.scope + "/out", f"DSCNN/{blk.scope}/pw_batch_norm")]
    return keys


# ---- the launch log -> path tokens -----------------------------------------------------------------------------------------------------
def one_of(names, table, what):
    """The token of the kernels of `table` = {kernel: token} among `names`: one token, or mixed-a+b in the table's order."""
    got = [tok for k, tok in table.items() if k in names]
    got = list(dict.fromkeys(got))
    assert got, ("no launch of", what, sorted(names))
    return got[0] if len(got) == 1 else "mixed-" + "+".join(got)


DW_FWD = {"dscnn_depthwise_rows_kernel": "rows", "dscnn_depthwise_rows_s2_kernel": "rows_s2", "dscnn_depthwise_lds2_kernel": "lds2",
          "dscnn_depthwise_lds_kernel": "lds", "dscnn_depthwise_kernel": "plain"}
DW_DGRAD = {"dscnn_dw_dgrad_rows_kernel": "rows", "dscnn_dw_dgrad_rows_s2_kernel": "rows_s2", "dscnn_dw_dgrad_lds_kernel": "lds",
            "dscnn_dw_dgrad_kernel": "plain"}
DW_WGRAD = {"dscnn_dw_wgrad_rows_kernel": "rows", "dscnn_dw_wgrad_rows_s2_kernel": "rows_s2", "dscnn_dw_wgrad_kernel": "plain"}
CONV1 = {"dscnn_conv1_dw_loop_kernel": "loop", "dscnn_conv1_dw_kernel": "fused", "dscnn_conv1_kernel": "alone"}
POOL = {"plane_mean_block_kernel": "block", "plane_mean_kernel": "plain"}
PW_WGRAD = {"pw_wgrad_glds_kernel": "lds", "pw_wgrad_lds_p_kernel": "lds", "pw_wgrad_lds_kernel": "lds", "conv_wgrad_mfma4_kernel": "slices",
            "conv_wgrad_mfma_kernel": "slices"}


def pw_tokens(entries):
    """lds6 / lds9 by the first template argument of the logged conv1x1_lds_kernel instance (its tile count per wave), mfma otherwise."""
    got = []
    for e in entries:
        k = kernel_of(e)
        if k == "conv1x1_mfma_kernel":
            got.append("mfma")
        elif k == "conv1x1_lds_kernel":
            assert " = " in e, ("the launch log has no demangled instance for", e)
            got.append("lds" + e.split(" = ", 1)[1].split("conv1x1_lds_kernel<", 1)[1].split(",")[0].strip())
    got = list(dict.fromkeys(got))
    assert got, "no pointwise launch in the log"
    return got[0] if len(got) == 1 else "mixed-" + "+".join(got)


def names_of(*logs):
    names = {kernel_of(e) for g in logs for e in g.entries}
    LAUNCHED.update(names)
    return names


def eval_paths(row, g):
    names = names_of(g)
    out = {"conv1": one_of(names, CONV1, "conv_1"), "pool": one_of(names, POOL, "the pooling"), "pw": pw_tokens(g.entries)}
    if names & set(DW_FWD):
        out["dw"] = one_of(names, DW_FWD, "the depthwise forward")
    return out


def train_paths(row, ge, gf, gb):
    """The tokens of a row's eval, training forward and backward together."""
    ne, nf, nb = names_of(ge), names_of(gf), names_of(gb)
    assert "dscnn_conv1_kernel" in nf and not nf & {"dscnn_conv1_dw_loop_kernel", "dscnn_conv1_dw_kernel"}
    return {"conv1": one_of(ne, CONV1, "conv_1"), "dw": one_of(ne | nf, DW_FWD, "the depthwise forward"),
            "dwd": one_of(nb, DW_DGRAD, "the depthwise data gradient"), "dww": one_of(nb, DW_WGRAD, "the depthwise filter gradient"),
            "pw": pw_tokens(ge.entries + gf.entries + gb.entries), "pww": one_of(nb, PW_WGRAD, "the pointwise filter gradient"),
            "pool": one_of(ne | nf, POOL, "the pooling"), "train": "materialised" if any(n.startswith("chan_reduce") for n in nf) else "lazy"}


def assert_paths(lib, row, got, override=None):
    """The families the row was written for ran, the others of each group did not (each group has exactly one token)."""
    if lib.kind != "emu":
        return
    want = paths_of(row)
    want.update(override or {})
    for k, v in got.items():
        if k in want:
            assert want[k] == v, (row[0], k, "expected", want[k], "ran", v)


def assert_exactly_the_tokens_kernels(row, names):
    """Of dscnn.hip's and dscnn_bwd.hip's kernels the row launched exactly those its tokens stand for (test_every_dscnn_launch_is_covered)."""
    if not row[6]:
        return
    got, want = names & source_launch_names(), implied_names(paths_of(row), trains(row))
    assert got == want, (row[0], "launched", sorted(got - want), "not launched", sorted(want - got))


# ---- one row ------------------------------------------------------------------------------------------------------------------------
_SETUP = {}


def features(batch, h, w, seed=300):
    return np.random.RandomState(seed).uniform(-2.0, 2.0, (batch, h, w)).astype(np.float32)


def row_setup(row):
    """Oracle side of a row: blocks, float32-rounded parameters / statistics as float64, random features, eval and train forwards."""
    name = row[0]
    if name in _SETUP:
        return _SETUP[name]
    _, _, h, w, nc, batch = row[:6]
    blocks = blocks_of(row)
    p, s = D.init_params(blocks, num_classes=nc, seed=5, randomize=True)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    s = {k: v.astype(np.float32).astype(np.float64) for k, v in s.items()}
    x = features(batch, h, w)
    x64 = x.astype(np.float64)
    labels = R.synth_labels(batch, nc).astype(np.float64)
    st = dict(blocks=blocks, p=p, s=s, x=x, labels=labels, ev=D.forward(blocks, p, s, x64, False))
    if trains(row):
        st["tr"] = D.forward(blocks, p, s, x64, True)
        st["loss"] = D.loss(st["tr"]["logits"], labels)
    _SETUP.clear()                      # (one row at a time)
    _SETUP[name] = st
    return st


def make_row_net(lib, row, st):
    net = T.DSCNN(None, row[2], row[3], row[4], net_def=row[1], lib=lib, device=Cm.device_of(lib))
    reload(net, st)
    return net


def reload(net, st):
    sd = dict(st["p"])
    sd.update(st["s"])
    net.load_state_dict(sd)


def planar(lib, x):
    return T.features_to_planar(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(Cm.device_of(lib)), lib=lib)


def oracle_grads(row, st, unit_act):
    """The oracle's gradients, on the kernels' side of the ReLU inputs within NEAR of zero.  unit_act(unit) -> [B, C, P] post-ReLU."""
    blocks, p, tr = st["blocks"], st["p"], st["tr"]
    masks, near = {}, 0
    for ui, (ck, bn) in enumerate(unit_keys(blocks)):
        pre = tr["cache"][bn]["xhat"] + p[bn + "/beta"]                    # [B, H, W, C]: the ReLU's input
        close = np.abs(pre) < NEAR
        near += int(close.sum())
        if close.any():
            act = unit_act(ui)
            kpos = np.transpose(act.reshape(pre.shape[0], pre.shape[3], pre.shape[1], pre.shape[2]), (0, 2, 3, 1)) > 0
            masks[ck] = np.where(close, kpos, pre > 0)
    return D.backward(blocks, p, tr, st["labels"], masks=masks), near


def grad_errors(got_of, tensors, gref, what):
    """Every gradient tensor of the net: the biases ahead of a BN exactly 0, the others within GRAD_RTOL of max(|ref|, 1e-3)."""
    worst, checked = 0.0, 0
    for k, ref in gref.items():
        got = got_of(k).reshape(ref.shape).astype(np.float64)
        checked += 1
        if k.endswith("/biases") and "fc1" not in k:
            assert np.all(got == 0.0), (what, k, "a bias ahead of a train-mode BN has gradient exactly 0")
            continue
        e = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-3))
        worst = max(worst, e)
        assert e < GRAD_RTOL, f"{what}: {k}: grad rel err {e}"
    trainable = [k for k, ti in tensors.items() if ti.arena == 0]
    assert checked == len(gref) == len(trainable) and set(gref) == set(trainable), (what, checked, len(gref), len(trainable))
    return worst


def stat_errors(stat_of, new_stats, what):
    worst = 0.0
    for k, ref in new_stats.items():
        e = float(np.abs(stat_of(k) - ref).max() / max(1.0, np.abs(ref).max()))
        worst = max(worst, e)
        assert e < STAT_TOL, f"{what}: {k}: moving statistic err {e}"
    return worst


def check_eval(lib, row, st, net, feat, errs):
    name, ev = row[0], st["ev"]
    with Log(lib) as g:
        logits, probs = [v.clone() for v in net.forward_infer(feat)]
    lg = logits.cpu().numpy()
    errs["eval_logits"] = float(np.abs(lg - ev["logits"]).max())
    errs["eval_probs"] = float(np.abs(probs.cpu().numpy() - ev["probs"]).max())
    assert errs["eval_logits"] < Cm.LOGIT_TOL and errs["eval_probs"] < PROB_TOL, (name, errs)
    assert np.array_equal(lg.argmax(1), ev["logits"].argmax(1)), name
    l2, p2 = net.forward_infer(feat)
    assert torch.equal(logits, l2) and torch.equal(probs, p2), (name, "second forward_infer differs")
    return g


def check_train(lib, row, st, net, feat, errs, ge):
    name, batch = row[0], row[5]
    tr, labels = st["tr"], st["labels"]
    lab = Cm.to_dev(lib, labels)
    stats0 = net.stats.clone()
    with Log(lib) as gf:
        tl, tp, loss = [v.clone() for v in net.forward_train(feat, lab)]
    with Log(lib) as gb:
        g1 = net.backward().clone()
    if lib.kind == "emu":
        fam = train_paths(row, ge, gf, gb)
        print(name, "paths", " ".join(f"{k}:{v}" for k, v in fam.items()))
        assert_paths(lib, row, fam)
        assert_exactly_the_tokens_kernels(row, names_of(ge, gf, gb))
    errs["train_logits"] = float(np.abs(tl.cpu().numpy() - tr["logits"]).max())
    errs["train_probs"] = float(np.abs(tp.cpu().numpy() - tr["probs"]).max())
    errs["loss"] = abs(float(loss) / batch - st["loss"])
    print(name, "train forward", {k: errs[k] for k in ("train_logits", "train_probs", "loss")})
    assert errs["train_logits"] < Cm.LOGIT_TOL and errs["train_probs"] < PROB_TOL and errs["loss"] < LOSS_TOL, (name, errs)
    errs["stats"] = stat_errors(lambda k: net._view(k).cpu().numpy(), tr["new_stats"], name)
    gref, near = oracle_grads(row, st, lambda ui: net.unit_output(ui, batch).cpu().numpy())
    errs["relu_near"] = near
    errs["grads"] = grad_errors(lambda k: net.grad_view(k).cpu().numpy(), net.tensors, gref, name)
    pads = torch.ones(net.n_param, dtype=torch.bool)
    for ti in net.tensors.values():
        if ti.arena == 0:
            pads[ti.offset:ti.offset + ti.size] = False
    assert not bool(g1.cpu()[pads].any()), (name, "gradient arena not zero between its tensors")
    print(name, "train", {k: errs[k] for k in ("grads", "stats", "relu_near")})
    # run-to-run: bitwise (no float atomics, whatever the streams do)
    net.stats.copy_(stats0)
    tl2, _, loss2 = net.forward_train(feat, lab)
    assert torch.equal(tl, tl2) and float(loss) == float(loss2), (name, "second forward_train differs")
    assert torch.equal(g1, net.backward()), (name, "second backward differs")
    if name in OPTIM_ROWS:
        # tf.train.AdamOptimizer, t = 1, on the kernels' own gradient: lr_t = lr sqrt(1 - b2) / (1 - b1); m = (1 - b1) g; v = (1 - b2) g^2
        lr, wd, b1, b2, eps = 1e-3, 0.001, 0.9, 0.999, 1e-8
        net.slots.clear()
        w = net.params.cpu().numpy().astype(np.float64)
        gv = g1.cpu().numpy().astype(np.float64)
        gv[:net.n_decay] += wd * w[:net.n_decay]
        net.adam_step(lr, 1, b1, b2, eps, weight_decay=wd)
        m, v = (1 - b1) * gv, (1 - b2) * gv * gv
        want = w - lr * np.sqrt(1 - b2) / (1 - b1) * m / (np.sqrt(v) + eps)
        errs["adam"] = float(np.abs(net.params.cpu().numpy() - want).max())
        assert errs["adam"] < OPT_TOL, (name, "adam", errs["adam"])
        assert float(np.abs(net.slots["Adam"].cpu().numpy() - m).max()) < OPT_TOL and float(np.abs(net.slots["Adam_1"].cpu().numpy() - v).max()) < OPT_TOL
        net.slots.clear()
    reload(net, st)


def check_refused_training(lib, row, net, feat, st):
    """A row past a declared limit of the training kernels: the first training call refuses with TCR_ERR_ARG and names the limit, nothing
    is launched, and eval of the same net keeps working (it ran just before and runs again behind the refusal)."""
    batch, nc = row[5], row[4]
    assert lib.tcr_dscnn_train_workspace_bytes(net._h, batch) == 0
    msg = lib.tcr_last_error().decode()
    assert "tcr_dscnn training" in msg and ("3072" in msg or "conv1_kh" in msg), msg
    ws = torch.zeros(1 << 16, dtype=torch.float32, device=net.device)
    out = torch.zeros(2 * batch * nc + 2, dtype=torch.float32, device=net.device)
    lab = Cm.to_dev(lib, st["labels"])
    with Log(lib) as g:
        rc = lib.tcr_dscnn_forward_train(net._h, net.params.data_ptr(), net.stats.data_ptr(), feat.data_ptr(), lab.data_ptr(), batch, batch, 0.0,
                                         ws.data_ptr(), ws.numel() * 4, out.data_ptr(), out[batch * nc:].data_ptr(), out[2 * batch * nc:].data_ptr(),
                                         net._stream())
    assert rc == TCR_ERR_ARG and lib.tcr_last_error().decode() == msg and not g.entries, (rc, lib.tcr_last_error(), g.entries)
    assert not bool(out.any()) and not bool(ws.any())
    with pytest.raises(T.TcrError, match="tcr_dscnn training"):
        net.forward_train(feat, lab)
    return msg


def record(kind, lib, name, errs):
    print("DSCNN_CONFIGS_ERR", json.dumps({"kind": kind, "lib": lib.kind, "row": name, "errs": {k: float(f"{v:.4g}") for k, v in errs.items()}}))


def check_row(lib, row):
    """One row against the oracle.  Returns its worst errors."""
    name, _, h, w, nc, batch = row[:6]
    st = row_setup(row)
    net = make_row_net(lib, row, st)
    feat = planar(lib, st["x"])
    errs = {}
    ge = check_eval(lib, row, st, net, feat, errs)
    if trains(row):
        oh, ow = shapes_of(row)[-1]
        assert batch * oh * ow >= MIN_BN_POSITIONS, (name, batch, oh, ow)
        check_train(lib, row, st, net, feat, errs, ge)
    else:
        if lib.kind == "emu":
            fam = eval_paths(row, ge)
            print(name, "paths", " ".join(f"{k}:{v}" for k, v in fam.items()))
            assert_paths(lib, row, fam)
            assert_exactly_the_tokens_kernels(row, names_of(ge))
        check_refused_training(lib, row, net, feat, st)
        lo, _ = net.forward_infer(feat)
        assert float(np.abs(lo.cpu().numpy() - st["ev"]["logits"]).max()) < Cm.LOGIT_TOL
    record("rows", lib, name, errs)
    return errs


@pytest.mark.parametrize("name", ROW_IDS)
def test_config_row(emu_lib, name):
    check_row(emu_lib, ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_IDS)
def test_gpu_config_row(hip_lib, name):
    check_row(hip_lib, ROW[name])


# ---- the table itself -----------------------------------------------------------------------------------------------------------------
def source_launch_names():
    """Every check_launch("...") name of dscnn.hip and dscnn_bwd.hip, from the source text."""
    names = set()
    for f in ("dscnn.hip", "dscnn_bwd.hip"):
        with open(os.path.join(ROOT, "tc-resnet_amd", "csrc", f)) as fh:
            names |= set(re.findall(r'check_launch\("([A-Za-z0-9_]+)"\)', fh.read()))
    return names


def tokens(v):
    return v[len("mixed-"):].split("+") if v.startswith("mixed-") else [v]


def implied_names(paths, train):
    """The dscnn.hip / dscnn_bwd.hip kernels a row's tokens stand for."""
    inv = lambda table: {tok: k for k, tok in table.items()}
    out = {inv(CONV1)[paths["conv1"]]} | {inv(POOL)[t] for t in tokens(paths["pool"])}
    out |= {inv(DW_FWD)[t] for t in tokens(paths["dw"])} if "dw" in paths else set()
    if train:
        out |= {"dscnn_conv1_kernel", "dscnn_conv1_wgrad_kernel"}
        out |= {inv(DW_DGRAD)[t] for t in tokens(paths["dwd"])} | {inv(DW_WGRAD)[t] for t in tokens(paths["dww"])}
    return out


def test_rows_take_every_listed_branch():
    """The table itself: both sides of every dispatch predicate (a row that leaves takes its branch with it)."""
    assert len(set(ROW_IDS)) == len(ROWS)
    P = {r[0]: paths_of(r) for r in ROWS}
    have = lambda **kv: any(all(p.get(k) == v for k, v in kv.items()) for p in P.values())
    toks = lambda grp: {t for p in P.values() if grp in p for t in tokens(p[grp])}
    assert all(have(conv1=v) for v in ("loop", "fused", "alone"))
    assert toks("dw") == {"rows", "rows_s2", "lds2", "lds", "plain"} and toks("dwd") == {"rows", "rows_s2", "lds", "plain"}
    assert toks("dww") == {"rows", "rows_s2", "plain"} and have(dw="plain") and have(dw="lds") and have(dw="lds2")
    assert all(have(pw=v) for v in ("lds6", "lds9", "mfma")) and have(pww="lds") and have(pww="slices") and have(pool="block") and have(pool="plain")
    # lazy / materialised x the pointwise kernels and filter gradients: materialised at a depth whose pointwise convs are lds6, and with
    # the LDS filter gradient; lazy at lds6 and lds9
    assert have(train="materialised", pw="lds6", pww="slices") and have(train="materialised", pw="mfma", pww="lds")
    assert have(train="lazy", pw="lds6") and have(train="lazy", pw="lds9") and have(train="lazy", pool="plain") and have(train="lazy", pool="block")
    assert have(train="materialised", dw="mixed-lds+plain", dwd="mixed-lds+plain")
    # the anchors, the depth boundaries (output tiles 6 | 7, 12 | 13, 18 | 19; a last tile of 4 channels; 80 | 84), the shapes
    assert {(r[1], r[5]) for r in ROWS if r[2:5] == (49, 10, 12)} >= {(n, b) for n in (S, M, L) for b in (3, 4)}
    depth = {r[1][0]: P[r[0]] for r in ROWS if r[1][1:] == m2(0)[1:] and r[2:6] == (49, 10, 12, 4)}
    assert {4, 20, 80, 84, 96, 100, 192, 196, 288, 292} <= set(depth)
    assert [depth[d]["pw"] for d in (96, 100, 192, 196, 288, 292)] == ["mfma", "lds6", "lds6", "lds9", "lds9", "mfma"]
    assert (depth[80]["pww"], depth[84]["pww"]) == ("slices", "lds") and 100 % 16 == 4
    assert {(98, 10), (50, 10), (1, 1), (2, 3), (7, 4), (49, 13), (49, 40), (98, 40)} <= {(r[2], r[3]) for r in ROWS}
    assert {2, 35, 46} <= {r[4] for r in ROWS} and {1, 17, 33} <= {r[5] for r in ROWS if r[1] == s2()} and {1, 17, 33} <= {r[5] for r in ROWS if r[1] == M112}
    assert {1, 8} <= {r[1][1] for r in ROWS} and {1, 3, 12, 13, 16} <= {(list(r[1]) + [10])[4] for r in ROWS}
    assert {((1, 1), (1, 2)), ((2, 1), (2, 1))} <= {(r[1][2], r[1][3]) for r in ROWS}
    # no row past batch 33; train-mode BN over enough positions; the rows that cannot train are exactly those past a declared limit
    assert all(r[5] <= 33 for r in ROWS) and all(r[5] * shapes_of(r)[-1][0] * shapes_of(r)[-1][1] >= MIN_BN_POSITIONS for r in ROWS if trains(r))
    for r in ROWS:
        kh = (list(r[1]) + [10])[4]
        assert trains(r) == (kh <= 12 and r[3] * (r[2] + 8) <= 3072), r[0]
    for rows, need in ((GUARD_ROWS, 3), (OPTIM_ROWS, 2), (list(UNALIGNED_ROWS), 2)):
        assert len(rows) >= need and all(n in ROW and trains(ROW[n]) for n in rows)
    assert "t1_f1" in GUARD_ROWS and "f40_m112" in GUARD_ROWS
    # the unaligned rows start from the rows kernels, the block pooling and both LDS pointwise instances, and leave the first two
    assert all(P[n]["dw"] == "mixed-rows+rows_s2" and P[n]["pool"] == "block" for n in UNALIGNED_ROWS) and {P[n]["pw"] for n in UNALIGNED_ROWS} == {"lds6", "lds9"}
    assert all(v["dw"] == "mixed-lds2+lds" and v["dwd"] == "lds" and v["dww"] == "plain" and v["pool"] == "plain" for v in UNALIGNED_ROWS.values())


def test_every_dscnn_launch_is_covered():
    """Every kernel dscnn.hip / dscnn_bwd.hip can launch is what some row runs by default.  A row's tokens are asserted against the
    emulator's launch log when the row runs (check_row: exactly the kernels its tokens stand for), so the table speaks for the log; where
    rows ran in this process before this test, what they launched is checked against the table once more."""
    source = source_launch_names()
    assert len(source) >= 18, source
    covered = set()
    for r in ROWS:
        covered |= implied_names(paths_of(r), trains(r))
    for n, over in UNALIGNED_ROWS.items():
        p = paths_of(ROW[n])
        p.update(over)
        covered |= implied_names(p, True)
    assert not set(EXEMPT) - source, ("exempt names that the sources no longer have", set(EXEMPT) - source)
    missing = source - covered - set(EXEMPT)
    assert not missing, ("no row of tests/test_dscnn_configs.py reaches", sorted(missing))
    assert (LAUNCHED & source) <= covered, sorted((LAUNCHED & source) - covered)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    dev = Cm.device_of(lib)

    def refused(what, net_def=S, h=49, w=10, nc=12):
        with pytest.raises(T.TcrError) as e:
            T.DSCNN(None, h, w, nc, net_def=net_def, lib=lib, device=dev)
        assert "tcr_dscnn_create" in str(e.value) and what in str(e.value), str(e.value)

    refused("depth 6 must be a positive multiple of 4", (6, 2, (2, 2), (1, 1)))
    refused("depth 0", (0, 2, (2, 2), (1, 1)))
    refused("n_separable 9", (64, 9, (2, 2), (1, 1)))
    refused("n_separable 0", (64, 0, (2, 2), (1, 1)))
    refused("num_classes 47 outside 1 .. 46", nc=47)
    refused("num_classes 0 outside 1 .. 46", nc=0)
    T.DSCNN(None, 49, 10, 46, net_def=S, lib=lib, device=dev)
    refused("17 x 4", (64, 2, (2, 2), (1, 1), 17))
    refused("0 x 4", (64, 2, (2, 2), (1, 1), 0))
    for s1, sds in (((3, 1), (1, 1)), ((1, 3), (1, 1)), ((2, 2), (3, 1)), ((2, 2), (1, 4)), ((0, 1), (1, 1)), ((2, 2), (1, 0))):
        refused("strides must be 1 or 2", (64, 2, s1, sds))
    refused("h_in", h=0)
    refused("w_in", w=0)
    # the training limits, from the first training call (eval of these nets: the rows kh13, kh16, t98_f40_s)
    for net_def, h, w, what in ((s2(13), 49, 10, "conv1_kh 13 > 12"), (s2(16), 49, 10, "conv1_kh 16 > 12"), (S, 98, 40, "40 x 106 > 3072"),
                                (S, 300, 10, "10 x 308 > 3072"), (S, 89, 32, "32 x 97 > 3072")):
        net = T.DSCNN(None, h, w, 12, net_def=net_def, lib=lib, device=dev)
        assert lib.tcr_dscnn_workspace_bytes(net._h, 2) > 0
        assert lib.tcr_dscnn_train_workspace_bytes(net._h, 2) == 0
        msg = lib.tcr_last_error().decode()
        assert "tcr_dscnn training" in msg and what in msg and "eval only" in msg, msg
        with pytest.raises(T.TcrError, match="tcr_dscnn training"):
            net.train_workspace(2)
    # ... and exactly at them: 12 kernel rows; 32 coefficients x (88 + 8) frames = 3072 floats
    for net_def, h, w in ((s2(12), 49, 10), (S, 88, 32)):
        net = T.DSCNN(None, h, w, 12, net_def=net_def, lib=lib, device=dev)
        assert w * (h + 8) <= 3072 and lib.tcr_dscnn_train_workspace_bytes(net._h, 2) > 0


def test_refusals(emu_lib):
    check_refusals(emu_lib)


def test_dw_wgrad_plan(emu_lib):
    """The depthwise filter gradient's host arithmetic (tcr_dscnn_dw_wgrad_plan: what launch_dscnn_dw_wgrad computes): chunks of about 32
    utterances, at most 128 of them -- so a chunk grows with batch / 128 and chunk x positions can leave the range in which the plain
    kernel's float-reciprocal index split is exact (fast_div, tcr_common.h: below 2^22); from there on the kernel divides.  A restatement
    of fast_div in float32 shows why the bound matters."""
    def plan(batch, pos):
        c, u, f = C.c_int(), C.c_int(), C.c_int()
        emu_lib.check(emu_lib.tcr_dscnn_dw_wgrad_plan(batch, pos, C.byref(c), C.byref(u), C.byref(f)), "tcr_dscnn_dw_wgrad_plan")
        return c.value, u.value, f.value

    assert plan(1, 65) == (1, 1, 1) and plan(32, 65) == (1, 32, 1) and plan(33, 65) == (2, 17, 1) and plan(4096, 65) == (128, 32, 1)
    assert plan(4097, 65) == (125, 33, 1)                       # 128 chunks at most: from here the utterances per chunk grow
    for batch, pos in ((4096, 125), (8 * 4096, 250), (65535 * 16, 65), (65535 * 16, 3920), (1 << 20, 4), (524288, 1024)):
        c, u, f = plan(batch, pos)
        assert c <= 128 and c * u >= batch and (c - 1) * u < batch
        assert f == (1 if u * pos < (1 << 22) else 0), (batch, pos, c, u, f)
    assert plan(524288, 1024)[2] == 0 and plan(524288 - 128, 1024)[2] == 1      # 4096 x 1024 = 2^22: the first chunk size that divides
    assert emu_lib.tcr_dscnn_dw_wgrad_plan(0, 65, None, None, None) == TCR_ERR_ARG
    # fast_div restated: exact below 2^22 on a sample of the worst cases (n just below and at multiples of d), wrong beyond 2^24
    def fast_div(n, d):
        q = (((n.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / d.astype(np.float32))).astype(np.float32)).astype(np.int64)
        return q + np.where((q + 1) * d <= n, 1, np.where(q * d > n, -1, 0))
    rng = np.random.RandomState(0)
    d = rng.randint(1, 4000, 200000).astype(np.int64)
    k = rng.randint(1, 1 << 22, 200000).astype(np.int64) // d
    for n in (k * d, np.maximum(k * d - 1, 0), np.minimum(k * d + d - 1, (1 << 22) - 1)):
        assert np.array_equal(fast_div(n, d), n // d)
    n = np.arange((1 << 27) - 4096, 1 << 27, dtype=np.int64)
    assert not np.array_equal(fast_div(n, np.full_like(n, 3)), n // 3)


# ---- writes stay inside what the API declares; pointers one float off ------------------------------------------------------------------------
def abi_buffers(lib, net, row, st, shift):
    nc, batch = row[4], row[5]
    h = net._h
    sizes = (("logits", batch * nc), ("probs", batch * nc), ("loss", 1), ("grads", net.n_param), ("stats", net.n_stat),
             ("ws0", lib.tcr_dscnn_workspace_bytes(h, batch) // 4), ("ws1", lib.tcr_dscnn_train_workspace_bytes(h, batch) // 4))
    bufs = {k: Guarded(lib, n, shift) for k, n in sizes}
    assert bufs["ws0"].n > 0 and bufs["ws1"].n > 0
    bufs["stats"].body.copy_(net.stats)
    return bufs


def abi_pass(lib, net, row, bufs, P, name, what):
    """tcr_dscnn_forward_infer / _forward_train / _backward through the C ABI on `bufs` (P: the read-only operands' pointers); the logs."""
    batch = row[5]
    h, stream = net._h, net._stream()

    def intact(call):
        bad = [k for k, b in bufs.items() if not b.intact()]
        assert not bad, (name, what, call, "wrote outside", bad)

    ws = bufs["ws0"]
    with Log(lib) as ge:
        lib.check(lib.tcr_dscnn_forward_infer(h, P["params"], bufs["stats"].ptr(), P["feat"], batch, ws.ptr(), ws.n * 4, bufs["logits"].ptr(),
                                              bufs["probs"].ptr(), stream), "tcr_dscnn_forward_infer")
    intact("tcr_dscnn_forward_infer")
    ev = (bufs["logits"].body.clone(), bufs["probs"].body.clone())
    # a DECLARED size one float short is refused before anything is launched (the allocation keeps its full size and its guards)
    rc = lib.tcr_dscnn_forward_infer(h, P["params"], bufs["stats"].ptr(), P["feat"], batch, ws.ptr(), ws.n * 4 - 4, bufs["logits"].ptr(),
                                     bufs["probs"].ptr(), stream)
    assert rc != 0 and b"workspace" in lib.tcr_last_error()
    ws = bufs["ws1"]
    with Log(lib) as gf:
        lib.check(lib.tcr_dscnn_forward_train(h, P["params"], bufs["stats"].ptr(), P["feat"], P["labels"], batch, batch, 0.0, ws.ptr(), ws.n * 4,
                                              bufs["logits"].ptr(), bufs["probs"].ptr(), bufs["loss"].ptr(), stream), "tcr_dscnn_forward_train")
    intact("tcr_dscnn_forward_train")
    rc = lib.tcr_dscnn_backward(h, P["params"], P["feat"], batch, ws.ptr(), ws.n * 4 - 4, bufs["grads"].ptr(), stream)
    assert rc != 0 and b"workspace" in lib.tcr_last_error()
    with Log(lib) as gb:
        lib.check(lib.tcr_dscnn_backward(h, P["params"], P["feat"], batch, ws.ptr(), ws.n * 4, bufs["grads"].ptr(), stream), "tcr_dscnn_backward")
    intact("tcr_dscnn_backward")
    return ev, (ge, gf, gb)


def check_guards(lib, row):
    """The three passes through the C ABI with every written buffer exactly as large as declared (the workspaces: tcr_dscnn_workspace_bytes
    / tcr_dscnn_train_workspace_bytes, passed as their size) between guard regions: the guards keep their pattern, the results are bitwise
    the engine's own, and the gradient arena -- handed over full of the pattern -- comes back zero outside the tensors."""
    name, nc, batch = row[0], row[4], row[5]
    st = row_setup(row)
    net = make_row_net(lib, row, st)
    feat = planar(lib, st["x"])
    lab = Cm.to_dev(lib, st["labels"])
    want_eval = [v.clone() for v in net.forward_infer(feat)]
    stats0 = net.stats.clone()
    want_train = [v.clone() for v in net.forward_train(feat, lab)]
    want_grads = net.backward().clone()
    want_stats = net.stats.clone()
    net.stats.copy_(stats0)
    bufs = abi_buffers(lib, net, row, st, 0)
    ev, _ = abi_pass(lib, net, row, bufs, {"params": net.params.data_ptr(), "feat": feat.data_ptr(), "labels": lab.data_ptr()}, name, "guards")
    assert torch.equal(ev[0].view(batch, nc), want_eval[0]) and torch.equal(ev[1].view(batch, nc), want_eval[1]), (name, "tcr_dscnn_forward_infer")
    assert torch.equal(bufs["logits"].body.view(batch, nc), want_train[0]) and torch.equal(bufs["probs"].body.view(batch, nc), want_train[1])
    assert float(bufs["loss"].body[0]) == float(want_train[2]) and torch.equal(bufs["stats"].body, want_stats), (name, "tcr_dscnn_forward_train")
    got = bufs["grads"].body
    assert torch.equal(got, want_grads), (name, "tcr_dscnn_backward", float((got - want_grads).abs().max()))
    pads = torch.ones(net.n_param, dtype=torch.bool)
    for ti in net.tensors.values():
        if ti.arena == 0:
            pads[ti.offset:ti.offset + ti.size] = False
    assert int(pads.sum()) >= 64 and not bool(got.cpu()[pads].any()), (name, "gradient arena not zero outside its tensors")


@pytest.mark.parametrize("name", GUARD_ROWS)
def test_writes_stay_inside_declared_buffers(emu_lib, name):
    check_guards(emu_lib, ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GUARD_ROWS)
def test_gpu_writes_stay_inside_declared_buffers(hip_lib, name):
    check_guards(hip_lib, ROW[name])


def check_unaligned(lib, name):
    """Every pointer of the three passes -- parameters, statistics, features, labels, workspaces, outputs, gradients -- one float behind a
    16-byte boundary (a C-ABI caller owes the library 4-byte alignment only): against the oracle with the row's tolerances, guards
    intact, and on the emulator the forms that need 16-byte operands not launched (the depthwise rows kernels, the block pooling)."""
    row = ROW[name]
    nc, batch = row[4], row[5]
    st = row_setup(row)
    net = make_row_net(lib, row, st)
    bufs = abi_buffers(lib, net, row, st, 1)
    feat0 = planar(lib, st["x"])
    ro = {"params": Guarded(lib, net.n_param, 1), "feat": Guarded(lib, feat0.numel(), 1), "labels": Guarded(lib, batch * nc, 1)}
    for k, src in (("params", net.params), ("feat", feat0.reshape(-1)), ("labels", Cm.to_dev(lib, st["labels"]).reshape(-1))):
        ro[k].body.copy_(src)
    assert all(b.ptr() % 16 == 4 for b in list(bufs.values()) + list(ro.values()))
    ev, (ge, gf, gb) = abi_pass(lib, net, row, bufs, {k: b.ptr() for k, b in ro.items()}, name, "unaligned")
    assert all(b.intact() for b in ro.values())
    if lib.kind == "emu":
        fam = train_paths(row, ge, gf, gb)
        print(name, "unaligned paths", " ".join(f"{k}:{v}" for k, v in fam.items()))
        assert_paths(lib, row, fam, UNALIGNED_ROWS[name])
    errs = {"eval_logits": float(np.abs(ev[0].view(batch, nc).cpu().numpy() - st["ev"]["logits"]).max()),
            "eval_probs": float(np.abs(ev[1].view(batch, nc).cpu().numpy() - st["ev"]["probs"]).max()),
            "train_logits": float(np.abs(bufs["logits"].body.view(batch, nc).cpu().numpy() - st["tr"]["logits"]).max()),
            "train_probs": float(np.abs(bufs["probs"].body.view(batch, nc).cpu().numpy() - st["tr"]["probs"]).max()),
            "loss": abs(float(bufs["loss"].body[0]) / batch - st["loss"])}
    assert errs["eval_logits"] < Cm.LOGIT_TOL and errs["eval_probs"] < PROB_TOL, (name, "unaligned eval", errs)
    assert errs["train_logits"] < Cm.LOGIT_TOL and errs["train_probs"] < PROB_TOL and errs["loss"] < LOSS_TOL, (name, "unaligned train", errs)
    stats = bufs["stats"].body.cpu().numpy()
    view = lambda arena, k: arena[net.tensors[k].offset:net.tensors[k].offset + net.tensors[k].size]
    errs["stats"] = stat_errors(lambda k: view(stats, k), st["tr"]["new_stats"], name + " (unaligned)")

    def unit_act(ui):           # the ABI's own view of the unit, in the unaligned workspace
        off, c, pos, pad = C.c_int64(), C.c_int(), C.c_int(), C.c_int()
        lib.check(lib.tcr_dscnn_unit_output(net._h, ui, batch, C.byref(off), C.byref(c), C.byref(pos), C.byref(pad)), "tcr_dscnn_unit_output")
        ws = bufs["ws1"]
        lib.check(lib.tcr_dscnn_materialize_unit(net._h, ui, batch, ws.ptr(), ws.n * 4, net._stream()), "tcr_dscnn_materialize_unit")
        return ws.body[off.value:off.value + batch * c.value * pad.value].view(batch, c.value, pad.value)[:, :, T._lib.HALO:T._lib.HALO + pos.value].cpu().numpy()

    gref, near = oracle_grads(row, st, unit_act)
    grads = bufs["grads"].body.cpu().numpy()
    errs["grads"] = grad_errors(lambda k: view(grads, k), net.tensors, gref, name + " (unaligned)")
    assert all(b.intact() for b in bufs.values())
    record("unaligned", lib, name, errs)
    return errs


@pytest.mark.parametrize("name", list(UNALIGNED_ROWS))
def test_pointers_one_float_off(emu_lib, name):
    check_unaligned(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNALIGNED_ROWS))
def test_gpu_pointers_one_float_off(hip_lib, name):
    check_unaligned(hip_lib, name)


# ---- GPU only: the loop kernel's group size ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_loop_kernel_ragged_groups(hip_lib):
    """dscnn_conv1_dw_loop_kernel walks upw = min(8, batch x channel groups / (3 x CUs)) utterances per workgroup: 1 up to batch 170 on
    DS-CNN-L (9 channel groups, 256 CUs), 2 at 173 (a last group of one), 8 at 4099 (a last group of three).  64 distinct utterances
    cycled: every row bitwise its utterance's row at batch 64, the 64 within LOGIT_TOL of the oracle."""
    lib = hip_lib
    blocks = D.net_def("L")
    p, s = D.init_params(blocks, seed=5)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    s = {k: v.astype(np.float32).astype(np.float64) for k, v in s.items()}
    x = features(64, 49, 10, seed=301)
    net = T.DSCNN("L", 49, 10, 12, lib=lib, device=Cm.device_of(lib))
    reload(net, dict(p=p, s=s))
    feat = planar(lib, x)
    lo, pr = [v.clone() for v in net.forward_infer(feat)]
    ref = D.forward(blocks, p, s, x.astype(np.float64), False)
    errs = {"eval_logits": float(np.abs(lo.cpu().numpy() - ref["logits"]).max()), "eval_probs": float(np.abs(pr.cpu().numpy() - ref["probs"]).max())}
    assert errs["eval_logits"] < Cm.LOGIT_TOL and errs["eval_probs"] < PROB_TOL, errs
    assert np.array_equal(lo.cpu().numpy().argmax(1), ref["logits"].argmax(1))
    for batch in (173, 4099):
        idx = torch.arange(batch, device=feat.device) % 64
        l2, p2 = net.forward_infer(feat[idx].contiguous())
        assert torch.equal(l2, lo[idx]) and torch.equal(p2, pr[idx]), (batch, float((l2 - lo[idx]).abs().max()))
    record("rows", lib, "l_eval_b64_b173_b4099", errs)


# ---- the detection stack on a non-flagship DS-CNN ------------------------------------------------------------------------------------------
def check_detection_stack(lib, n_streams):
    """DS-CNN-S behind a 30 ms / 10 ms front-end (98 frames x 10 coefficients), k = 1: every push's logits / probabilities are bitwise
    forward_infer of the stream windows, and a short scan is bitwise the pushes -- INTEGRATION.md's claim for every family."""
    from tests import test_detect_families as TD
    from tests.test_scan import assert_bitwise, pushed
    from tests.test_streaming import segment_audio
    fe, net = TD.dscnn(lib, "S", win=480, hop=160)
    assert (fe.n_frames, fe.n_coef) == (98, 10)
    TD.run_pushes(lib, fe, net, n_streams, 1, 3, {2: [1]}, average_window_ms=30, min_count=1, suppression_ms=20, detection_threshold=0.0)
    dkw = dict(average_window_ms=30, min_count=2, detection_threshold=0.0, suppression_ms=40)
    audio = Cm.to_dev(lib, segment_audio(n_streams, 5 * fe.cfg.hop, 3))
    want = pushed(TD.streaming().StreamingDetector(net, fe, n_streams, frames_per_step=1, **dkw), audio)
    assert_bitwise(TD.scanner(net, fe, 1, **dkw).scan(audio), want)
    assert_bitwise(TD.scanner(net, fe, 1, max_windows=4, **dkw).scan(audio), want)


def test_detection_stack_on_a_non_flagship_dscnn(emu_lib):
    check_detection_stack(emu_lib, 2)


@pytest.mark.gpu
def test_gpu_detection_stack_on_a_non_flagship_dscnn(hip_lib):
    check_detection_stack(hip_lib, 64)
