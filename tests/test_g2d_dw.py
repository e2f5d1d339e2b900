"""The depthwise convolution of the 2-D graph engine (csrc/net2d_dw.hip, tcr_g2d_depthwise_conv, engine.Graph2D.depthwise_conv) across
its configuration space: tests/g2d_dw_configs.py's rows against the float64 reference of tests/g2d_dw_ref.py -- eval logits and
probabilities, training-mode logits / loss / moving statistics, EVERY gradient, one Adam step over the decayed set, then the same passes
once more through the C ABI between poisoned guards with every pointer one float behind a 16-byte boundary.  Without a tolerance: the
forward on integers against an int64 sum and a one-hot input against the shifted tap image (tests/g2d_dw_configs.py::EXACT), backward
twice, the staged run, the emulator's workgroups in reverse.  The helpers, tolerances and the ReLU-kink rule are
tests/test_g2d_configs.py's.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`): the same rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import dscnn_ref as D
from oracle import net2d_ref as O
from oracle import numpy_ref as R
from tests import common as Cm
from tests import g2d_dw_configs as K
from tests import g2d_dw_ref as W
from tests import test_g2d_configs as TG
from tests.test_g2d_configs import GRAD_RTOL, LOSS_TOL, TOFF, TSEED
from tests.test_models2d import _randomise, _split
from tests.test_net_configs import MIN_BN_POSITIONS, OPT_TOL, PROB_TOL, Log, kernel_of

DW_KERNELS = {"dw2d_kernel", "dw2d_wgrad_kernel"}
_SPECS = {}


def spec_of(row):
    if row[0] not in _SPECS:
        _SPECS[row[0]] = K.graph(row[4])
    return _SPECS[row[0]]


def opts_of(row):
    return row[6] if len(row) > 6 else {}


def build_graph(lib, spec, h, w, c=1):
    g = T.Graph2D("", h, w, c, lib=lib, device=Cm.device_of(lib))
    for i, n in enumerate(spec["nodes"]):
        op = n["op"]
        if op == "conv":
            got = g.conv(n["in"], n["k"], n["cout"], n["w"], stride=n["stride"], rate=n["rate"], padding=n["pad"], relu=n["relu"], biases_name=n["b"])
        elif op == "dwconv":
            got = g.depthwise_conv(n["in"], n["k"], n["w"], stride=n["stride"], rate=n["rate"], padding=n["pad"], relu=n["relu"], biases_name=n["b"])
        elif op == "bn":
            got = g.batch_norm(n["in"], n["prefix"], center=n["center"], scale=n["scale"], relu=n["relu"])
        elif op == "pool":
            got = g.pool(n["in"], n["kind"], n["k"], n["stride"], n["pad"])
        else:
            assert op == "add", op
            got = g.add(n["a"], n["b"], relu=n["relu"])
        assert got == i, (op, got, i)
    g.finalize(spec["logits"])
    return g


def shapes_of(spec, h, w, c=1):
    """Every node's (C, H, W), from the reference's own ops on zeros."""
    shapes = []
    for n in spec["nodes"]:
        ci, ih, iw = (c, h, w) if n.get("in", n.get("a")) < 0 else shapes[n.get("in", n.get("a"))]
        x = torch.zeros((1, 1, ih, iw), dtype=torch.float64)
        if n["op"] in ("conv", "dwconv"):
            y = O.conv2d(x, torch.zeros(tuple(n["k"]) + (1, 1), dtype=torch.float64), tuple(n["stride"]), tuple(n["rate"]), n["pad"])
            shapes.append((n["cout"] if n["op"] == "conv" else ci, y.shape[2], y.shape[3]))
        elif n["op"] == "pool":
            y = O.avg_pool(x, tuple(n["k"]), tuple(n["stride"]), n["pad"]) if n["k"] else x[:, :, :1, :1]
            shapes.append((ci, y.shape[2], y.shape[3]))
        else:
            shapes.append((ci, ih, iw))
    return shapes


def dw_nodes(row):
    """(node, input shape, output shape) of the row's depthwise convolutions."""
    spec, (h, w) = spec_of(row), row[1:3]
    sh = shapes_of(spec, h, w)
    return [(n, (1, h, w) if n["in"] < 0 else sh[n["in"]], sh[i]) for i, n in enumerate(spec["nodes"]) if n["op"] == "dwconv"]


def row_setup(lib, row, seed=0):
    name, h, w, batch = row[:4]
    spec = spec_of(row)
    eng = build_graph(lib, spec, h, w)
    sd = _randomise(eng, seed + 1)
    p, s = _split(eng, sd)
    x = TG.features(batch, h, w, 300 + seed)
    labels = R.synth_labels(batch, num_classes=eng.num_classes).astype(np.float64)
    for i, n in enumerate(spec["nodes"]):
        if n["op"] == "bn":
            assert batch * eng.shape(i)[1] * eng.shape(i)[2] >= MIN_BN_POSITIONS, (name, i)
    return dict(spec=spec, eng=eng, sd=sd, p=p, s=s, x=x, xt=torch.tensor(x.astype(np.float64)), labels=labels, masks=None)


def oracle_eval(st):
    tp = {k: torch.tensor(v) for k, v in st["p"].items()}
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in W.graph_forward(st["spec"], tp, st["s"], st["xt"], False, None).items()}


def oracle_train(st, kept, errs=None, name=""):
    """tests/test_g2d_configs.py::oracle_train on this file's reference: the ReLU-kink allowance is a condition on the float64 reference."""
    with O.follow_kinks(kept) as log:
        out, model, _tot, grads = O.loss_and_grads(lambda pp: W.graph_forward(st["spec"], pp, st["s"], st["xt"], True, None), st["p"], st["labels"])
    near, total, followed = log["near"], log["total"], log["followed"]
    assert near <= 2 + 1e-4 * total and followed <= near, (name, "ReLU inputs within tau of zero", near, "of", total, "followed", followed)
    if errs is not None:
        errs["relu_near"] = near
    return out, model, grads


def expected_dw_launches(row):
    """{(instance of dw2d_kernel)} a row's eval + training step launches, from tests/g2d_dw_configs.py::plan."""
    want = set()
    for n, (ci, ih, iw), (co, oh, ow) in dw_nodes(row):
        kh, (dh, _), (sh, _) = n["k"][0], n["rate"], n["stride"]
        nt, _ = K.plan(False, ih, iw, oh, ow, kh, dh, sh)
        want.add(f"dw2d_kernel<{nt}, {16 * nt}, false>")
        if n["in"] >= 0:
            nt, _ = K.plan(True, ih, iw, oh, ow, kh, dh, sh)
            want.add(f"dw2d_kernel<{nt}, {16 * nt}, true>")
    return want


def assert_launches(lib, row, logs):
    if lib.kind != "emu":
        return
    entries = [e for g in logs for e in g.entries]
    assert DW_KERNELS <= {kernel_of(e) for e in entries}, (row[0], sorted({kernel_of(e) for e in entries}))
    got = {e.split(" = ", 1)[1].split("tcr::")[1].split("(")[0] for e in entries if kernel_of(e) == "dw2d_kernel" and " = " in e}
    assert got == expected_dw_launches(row), (row[0], sorted(got), sorted(expected_dw_launches(row)))
    assert any("wgrad_reduce_kernel" in e for e in entries), row[0]


def check_adam(eng, errs):
    """One tf.train.AdamOptimizer step (t = 1) with weight decay on the kernels' own gradient against the oracle's step; the decayed set
    by NAME (oracle.numpy_ref.is_l2_param): the depthwise weights and biases are in it."""
    lr, wd = 1e-3, 0.01
    names = eng.trainable_names()
    dws = [k for k in names if "depthwise_weights" in k]
    assert dws and all(R.is_l2_param(k) and eng.tensors[k].offset + eng.tensors[k].size <= eng.n_decay for k in dws)
    w = {k: eng._view(k).cpu().numpy().astype(np.float64) for k in names}
    g = {k: eng.grad_view(k).cpu().numpy().astype(np.float64) + (wd * w[k] if R.is_l2_param(k) else 0.0) for k in names}
    zeros = {k: np.zeros_like(v) for k, v in w.items()}
    want, m, v = D.adam_step(w, zeros, zeros, g, lr, 1)
    eng.slots.clear()
    eng.adam_step(lr, 1, weight_decay=wd)
    view = lambda arena, k: arena.cpu().numpy()[eng.tensors[k].offset:eng.tensors[k].offset + eng.tensors[k].size].reshape(w[k].shape)
    errs["adam"] = max(float(np.abs(view(eng.params, k) - want[k]).max()) for k in names)
    slot = max(max(float(np.abs(view(eng.slots["Adam"], k) - m[k]).max()), float(np.abs(view(eng.slots["Adam_1"], k) - v[k]).max())) for k in names)
    assert errs["adam"] < OPT_TOL and slot < OPT_TOL, ("adam", errs["adam"], slot)
    eng.slots.clear()


def compare(name, what, batch, nc, ev, tr, loss, stat_of, grad_of, st, kept, errs):
    """Eval (logits, probs), training (logits, probs), loss sum, statistics and gradients of one run against the reference."""
    eng = st["eng"]
    ref = oracle_eval(st)
    e = {"eval_logits": float(np.abs(ev[0] - ref["logits"]).max()), "eval_probs": float(np.abs(ev[1] - ref["probs"]).max())}
    print(name, what, "eval", e)
    assert e["eval_logits"] < Cm.LOGIT_TOL and e["eval_probs"] < PROB_TOL, (name, what, e)
    assert np.array_equal(ev[0].argmax(1), ref["logits"].argmax(1)), (name, what)
    out, model, grads = oracle_train(st, kept, e, name)
    e["train_logits"] = float(np.abs(tr[0] - out["logits"]).max())
    e["train_probs"] = float(np.abs(tr[1] - out["probs"]).max())
    e["loss"] = abs(loss / batch - model)
    print(name, what, "train forward", e)
    assert e["train_logits"] < Cm.LOGIT_TOL and e["train_probs"] < PROB_TOL and e["loss"] < LOSS_TOL, (name, what, e)
    e["stats"] = TG.stat_errors(stat_of, out["new_stats"], f"{name} ({what})")
    e["grads"] = TG.grad_errors(grad_of, eng.tensors, grads, f"{name} ({what})")
    print(name, what, "train", {k: e[k] for k in ("grads", "stats", "relu_near")})
    errs.update({f"{what}_{k}" if what != "engine" else k: v for k, v in e.items()})


def check_row(lib, row):
    name, h, w, batch = row[:4]
    st = row_setup(lib, row)
    eng = st["eng"]
    nc = eng.num_classes
    assert nc == opts_of(row).get("nc", 12)
    feat = TG.planar(lib, st["x"])
    errs = {}
    with Log(lib) as ge:
        logits, probs = [v.clone() for v in eng.forward_infer(feat)]
    l2, p2 = eng.forward_infer(feat)
    assert torch.equal(logits, l2) and torch.equal(probs, p2), (name, "second forward_infer differs")
    lab = Cm.to_dev(lib, st["labels"])
    stats0 = eng.stats.clone()
    with Log(lib) as gf:
        tl, tp, loss = [v.clone() for v in eng.forward_train(feat, lab, seed=TSEED, sample_offset=TOFF)]
    kept = [(eng.node_output(n, batch, True) > 0).cpu() for n in eng.relu_nodes]
    with Log(lib) as gb:
        g1 = eng.backward().clone()
    assert_launches(lib, row, (ge, gf, gb))
    compare(name, "engine", batch, nc, (logits.cpu().numpy(), probs.cpu().numpy()), (tl.cpu().numpy(), tp.cpu().numpy()), float(loss),
            lambda k: eng._view(k).cpu().numpy(), lambda k: eng.grad_view(k).cpu().numpy(), st, kept, errs)
    assert not bool(g1.cpu()[TG.pad_mask(eng)].any()), (name, "gradient arena not zero between its tensors")
    # run-to-run: bitwise
    stats1 = eng.stats.clone()
    eng.stats.copy_(stats0)
    tl2, _, loss2 = eng.forward_train(feat, lab, seed=TSEED, sample_offset=TOFF)
    assert torch.equal(tl, tl2) and float(loss) == float(loss2) and torch.equal(eng.stats, stats1), (name, "second forward_train differs")
    assert torch.equal(g1, eng.backward()), (name, "second backward differs")
    # once more at the C ABI: guards around every buffer, every pointer 4 bytes behind a 16-byte boundary
    eng.stats.copy_(stats0)
    bufs, ev, logs = TG.abi_steps(lib, row, st, 1)
    assert_launches(lib, row, logs)
    kept = [(TG.node_act(lib, eng, bufs["ws1"], n, batch) > 0).cpu() for n in eng.relu_nodes]
    view = lambda arena, k: arena.cpu().numpy()[eng.tensors[k].offset:eng.tensors[k].offset + eng.tensors[k].size]
    compare(name, "abi", batch, nc, tuple(v.view(batch, nc).cpu().numpy() for v in ev),
            tuple(bufs[k].body.view(batch, nc).cpu().numpy() for k in ("logits", "probs")), float(bufs["loss"].body[0]),
            lambda k: view(bufs["stats"].body, k), lambda k: view(bufs["grads"].body, k), st, kept, errs)
    pads = TG.pad_mask(eng)
    assert not bool(bufs["grads"].body.cpu()[pads].any()), (name, "gradient arena not zero outside its tensors (C ABI)")
    eng.stats.copy_(stats0)
    check_adam(eng, errs)
    print("G2D_DW_CONFIGS_ERR", __import__("json").dumps({"lib": lib.kind, "row": name, "errs": {k: float(f"{v:.4g}") for k, v in errs.items()}}))
    return errs


@pytest.mark.parametrize("name", K.ROW_IDS)
def test_config_row(emu_lib, name):
    check_row(emu_lib, K.ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.ROW_IDS)
def test_gpu_config_row(hip_lib, name):
    check_row(hip_lib, K.ROW[name])


# ---- the table itself ---------------------------------------------------------------------------------------------------------------
def derived_classes(row):
    """The classes a row's own spec gives it (what it may state)."""
    name, h, w, batch = row[:4]
    have = {f"b:{batch}"}
    spec = spec_of(row)
    for n, (ci, ih, iw), (co, oh, ow) in dw_nodes(row):
        kh, kw = n["k"]
        have |= {f"plane:{ih}x{iw}", f"k:{kh}x{kw}", f"stride:{n['stride'][0]}x{n['stride'][1]}", f"rate:{n['rate'][0]}x{n['rate'][1]}", f"c:{ci}",
                 f"bias:{int(bool(n['b']))}", f"relu:{int(n['relu'])}", "in:-1" if n["in"] < 0 else "in:node"}
        if n["pad"] == "VALID":
            have.add("valid")
            if (kh, kw) == (ih, iw):
                have.add("k:valid=plane")
        if n["pad"] == "SAME" and (kh - 1) * n["rate"][0] + 1 > ih:
            have.add("window>plane")
        nt, t = K.plan(False, ih, iw, oh, ow, kh, n["rate"][0], n["stride"][0])
        if nt == 256:
            assert opts_of(row).get("T") == t, (name, "the row states its forward row tile", t)
            have |= {f"rows:{lbl}" for lbl, rows in (("T-1", t - 1), ("T", t), ("T+1", t + 1), ("2T+1", 2 * t + 1)) if oh == rows}
            have |= {"rows:T<32"} if t < K.ROW_TILE else set()
        if n["in"] >= 0:
            nt, t = K.plan(True, ih, iw, oh, ow, kh, n["rate"][0], n["stride"][0])
            have |= {"rows:dgrad-2T+1"} if nt == 256 and ih == 2 * t + 1 else set()
        readers = [m for m in spec["nodes"] if n["in"] >= 0 and n["in"] in (m.get("in"), m.get("a"), m.get("b"))]
        have |= {"fanout"} if len(readers) > 1 and any(m["op"] == "conv" for m in readers) else set()
    for i, n in enumerate(spec["nodes"]):
        if n["op"] == "bn" and n["center"] and not n["scale"] and spec["nodes"][n["in"]]["op"] == "dwconv":
            have.add("bn:center")
    return have | {"separable", "shards"}


def test_rows_hold_the_listed_cases():
    """Host only: every row's stated classes are what its spec has, the table reaches every class of REQUIRED, the stated row tiles are
    the restated arithmetic's, and the rows stay small."""
    assert len(set(K.ROW_IDS)) == len(K.ROWS)
    assert "tcr_g2d_depthwise_conv" in T._lib.ABI_SYMBOLS          # (the table is about a node the binding knows)
    reached = set()
    for row in K.ROWS:
        stated = set(row[5].split())
        assert stated <= derived_classes(row), (row[0], sorted(stated - derived_classes(row)))
        reached |= stated
        assert row[3] <= 17 or row[0] == "b513", row[0]
        assert all(ci <= 65 or row[0] == "c276" for _, (ci, _, _), _ in dw_nodes(row)), row[0]
    assert not set(K.REQUIRED) - reached, sorted(set(K.REQUIRED) - reached)
    assert K.ROW["b513"][1:4] == (2, 2, 513) and K.plan(False, 98, 40, 98, 40, 3, 1, 1) == (256, 32) and K.plan(False, 40, 130, 40, 130, 3, 1, 1) == (256, 29)
    assert K.plan(False, 25, 5, 25, 5, 3, 1, 1) == (64, 25) and K.plan(True, 65, 9, 33, 9, 3, 1, 2) == (256, 32)
    assert all(n in K.ROW for n in [K.SHARD_ROW, K.STAGED_ROW] + K.ORDER_ROWS)


def test_kernel_names_and_symbol(emu_lib):
    """The kernel names the launch log shows are in the library's table; the symbol is bound."""
    names = set()
    i = 0
    while emu_lib.tcr_kernel_name(i) is not None:
        names.add(emu_lib.tcr_kernel_name(i).decode())
        i += 1
    assert DW_KERNELS <= names and "tcr_g2d_depthwise_conv" in T._lib.ABI_SYMBOLS and emu_lib.tcr_abi_version() == 3


# ---- exact: integers, one-hot -------------------------------------------------------------------------------------------------------
def infer_abi(lib, eng, x):
    """tcr_g2d_forward_infer on a ready input [B, C, H*W + 2*HALO] (a graph of any input channel count)."""
    b = x.shape[0]
    ws = eng.workspace(b, False)
    logits, probs = eng._outputs(b)
    lib.check(lib.tcr_g2d_forward_infer(eng._h, eng.params.data_ptr(), eng.stats.data_ptr(), x.data_ptr(), b, ws.data_ptr(), ws.numel() * 4,
                                        logits.data_ptr(), probs.data_ptr(), eng._stream()), "tcr_g2d_forward_infer")
    return logits, probs


def to_planes(lib, x):
    """[B, C, H, W] -> the engine's input layout."""
    b, c, h, w = x.shape
    out = torch.zeros((b, c, h * w + 2 * TG.HALO), dtype=torch.float32)
    out[:, :, TG.HALO:TG.HALO + h * w] = torch.as_tensor(x, dtype=torch.float32).reshape(b, c, h * w)
    return out.to(Cm.device_of(lib))


def check_exact(lib, geo):
    """The node's own output (node_output) on integers: bitwise the int64 sum -- |x|, |w| <= 8, so every partial sum is an integer below
    2^24 and a float fmaf chain is exact in any order, i.e. every difference is an index error -- and a one-hot input against taps of
    distinct integers: the shifted tap image."""
    h, w, c, k, stride, rate, pad = geo
    g = T.Graph2D("", h, w, c, lib=lib, device=Cm.device_of(lib))
    node = g.depthwise_conv(-1, k, "dw/depthwise_weights", stride=stride, rate=rate, padding=pad)
    g.finalize(g.conv(g.pool(node, "avg"), (1, 1), 2, "fc/weights", biases_name="fc/biases"))
    rng = np.random.RandomState(h * 131 + w)
    batch = 2
    taps = k[0] * k[1]
    for what in ("integers", "one-hot"):
        if what == "integers":
            wi = rng.randint(-8, 9, (k[0], k[1], c)).astype(np.int64)
            xi = rng.randint(-8, 9, (batch, c, h, w)).astype(np.int64)
        else:
            wi = (1 + np.arange(taps * c).reshape(k[0], k[1], c)).astype(np.int64)          # distinct, < 2^24
            xi = np.zeros((batch, c, h, w), dtype=np.int64)
            for n in range(batch):
                for ch in range(c):
                    xi[n, ch, rng.randint(h), rng.randint(w)] = 1
        g._view("dw/depthwise_weights").copy_(torch.as_tensor(wi.astype(np.float32)).reshape(k[0], k[1], c, 1).to(g.device))
        infer_abi(lib, g, to_planes(lib, xi))
        got = g.node_output(node, batch, False).cpu().numpy()
        want = W.dw_int64(xi, wi, stride, rate, pad)
        assert got.shape == want.shape, (geo, got.shape, want.shape)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), (geo, what, np.argwhere(got != want)[:4])
        if what == "one-hot" and pad == "SAME" and stride == (1, 1):
            assert (want != 0).any(axis=(2, 3)).all(), geo                                  # (the checked image is not empty)


@pytest.mark.parametrize("geo", K.EXACT, ids=lambda g: "{}x{}_c{}_k{}x{}_s{}{}_r{}{}_{}".format(*g[:3], *g[3], *g[4], *g[5], g[6]))
def test_exact_forward(emu_lib, geo):
    check_exact(emu_lib, geo)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", K.EXACT, ids=lambda g: "{}x{}_c{}_k{}x{}_s{}{}_r{}{}_{}".format(*g[:3], *g[3], *g[4], *g[5], g[6]))
def test_gpu_exact_forward(hip_lib, geo):
    check_exact(hip_lib, geo)


# ---- a graph created with c = 3, at the C ABI --------------------------------------------------------------------------------------------
def check_c3(lib):
    """A depthwise conv reading a THREE-channel network input, driven through the C ABI (the engine's feature re-layout is single-channel):
    eval logits against the reference."""
    h, w, c, batch = 6, 5, 3, 4
    s = K.DwSpec()
    logits = s.head(s.conv(s.dw(-1, (3, 3), bias=True, relu=True), (3, 3), 6, relu=True))
    spec = {"nodes": s.nodes, "logits": logits}
    eng = build_graph(lib, spec, h, w, c)
    assert eng.tensors["n0/depthwise_weights"].size == 27 and eng.tf_shape("n0/depthwise_weights") == (3, 3, 3, 1) and eng.shape(0) == (3, 6, 5)
    sd = _randomise(eng, 4)
    p, st = _split(eng, sd)
    x = np.random.RandomState(9).uniform(-2, 2, (batch, c, h, w)).astype(np.float32)
    lg, pr = infer_abi(lib, eng, to_planes(lib, x))
    ref = W.graph_forward(spec, {k: torch.tensor(v) for k, v in p.items()}, st, torch.tensor(x.astype(np.float64)))
    assert float(np.abs(lg.cpu().numpy() - ref["logits"].numpy()).max()) < Cm.LOGIT_TOL
    assert float(np.abs(pr.cpu().numpy() - ref["probs"].numpy()).max()) < PROB_TOL


def test_three_channel_input(emu_lib):
    check_c3(emu_lib)


@pytest.mark.gpu
def test_gpu_three_channel_input(hip_lib):
    check_c3(hip_lib)


# ---- invariances --------------------------------------------------------------------------------------------------------------------
def check_staged(lib):
    """The cross-replica BN hand-off with an identity hook on one replica: bitwise the unstaged step."""
    row = K.ROW[K.STAGED_ROW]
    st = row_setup(lib, row)
    eng = st["eng"]
    feat, lab = TG.planar(lib, st["x"]), Cm.to_dev(lib, st["labels"])
    outs, seen = [], []
    for hook in (None, lambda sums: seen.append(sums.numel())):
        eng.load_state_dict(st["sd"])
        logits, probs, loss = eng.forward_train(feat, lab, seed=TSEED, sync_hook=hook)
        grads = eng.backward().clone()
        outs.append((logits.clone(), probs.clone(), loss.clone(), grads, eng.stats.clone()))
    assert len(seen) == 2 * (lib.tcr_g2d_num_stages(eng._h) - 1) > 0
    for a, c, what in zip(outs[0], outs[1], ("logits", "probs", "loss", "grads", "moving stats")):
        assert torch.equal(a, c), f"staged {what} differ from the unstaged run"


def test_staged_equals_unstaged(emu_lib):
    check_staged(emu_lib)


@pytest.mark.gpu
def test_gpu_staged_equals_unstaged(hip_lib):
    check_staged(hip_lib)


def check_shards(lib):
    """Two shards of 3 with global_batch = 6 against the whole batch of 6 on a BN-free graph: logits bitwise the whole run's rows, the
    gradients' sum within GRAD_RTOL, the losses' sum within LOSS_TOL."""
    row = K.ROW[K.SHARD_ROW]
    name, batch = row[0], row[3]
    st = row_setup(lib, row)
    eng = st["eng"]
    assert not any(n["op"] == "bn" for n in st["spec"]["nodes"]) and batch == 6
    feat, lab = TG.planar(lib, st["x"]), Cm.to_dev(lib, st["labels"])
    tl, _, loss = [v.clone() for v in eng.forward_train(feat, lab, seed=TSEED, sample_offset=0)]
    kept = [(eng.node_output(n, batch, True) > 0).cpu() for n in eng.relu_nodes]
    whole = eng.backward().clone()
    total, losses = torch.zeros_like(whole), 0.0
    for off in (0, 3):
        sl, _, slo = eng.forward_train(feat[off:off + 3].contiguous(), lab[off:off + 3].contiguous(), seed=TSEED, sample_offset=off, global_batch=batch)
        assert torch.equal(sl, tl[off:off + 3]), (name, "shard at", off)
        total += eng.backward()
        losses += float(slo)
    assert abs(losses - float(loss)) < LOSS_TOL * batch
    _out, _model, grads = oracle_train(st, kept, None, name)
    view = lambda arena, k: arena.cpu().numpy()[eng.tensors[k].offset:eng.tensors[k].offset + eng.tensors[k].size]
    TG.grad_errors(lambda k: view(whole, k), eng.tensors, grads, name)
    TG.grad_errors(lambda k: view(total, k), eng.tensors, grads, name + " (sum of the shards)")
    worst = max(float(np.abs(view(total, k) - view(whole, k)).max() / max(np.abs(view(whole, k)).max(), 1e-3)) for k in grads)
    assert worst < GRAD_RTOL, (name, worst)


def test_shards_sum_to_the_whole_batch(emu_lib):
    check_shards(emu_lib)


@pytest.mark.gpu
def test_gpu_shards_sum_to_the_whole_batch(hip_lib):
    check_shards(hip_lib)


@pytest.mark.parametrize("name", K.ORDER_ROWS)
def test_workgroups_last_to_first(emu_lib, name):
    """The emulator runs a launch's workgroups last to first (tcr_emu_block_order): bitwise the forward order -- no workgroup reads
    what another one of its launch writes, none relies on running before another."""
    lib, row = emu_lib, K.ROW[name]
    st = row_setup(lib, row)
    eng = st["eng"]
    feat, lab = TG.planar(lib, st["x"]), Cm.to_dev(lib, st["labels"])
    lib._dll.tcr_emu_block_order.restype, lib._dll.tcr_emu_block_order.argtypes = C.c_int, [C.c_int]
    outs = []
    try:
        for reverse in (0, 1):
            lib._dll.tcr_emu_block_order(reverse)
            eng.load_state_dict(st["sd"])
            ev = [v.clone() for v in eng.forward_infer(feat)]
            tr = [v.clone() for v in eng.forward_train(feat, lab, seed=TSEED)]
            outs.append(ev + tr + [eng.backward().clone(), eng.stats.clone()])
    finally:
        lib._dll.tcr_emu_block_order(0)
    for a, b in zip(*outs):
        assert torch.equal(a, b), name


def test_graph_is_released_when_the_last_reference_drops(emu_lib):
    """A graph -- with or without the depthwise builder used -- holds no reference to itself: its native handle and arenas go with the
    last reference, not with a later pass of the cyclic collector; the builder is no attribute of the class or of the instance."""
    import gc
    import weakref
    was = gc.isenabled()
    gc.disable()
    try:
        for use in (False, True):
            g = T.Graph2D("", 6, 5, 1, lib=emu_lib, device=Cm.device_of(emu_lib))
            node = g.depthwise_conv(-1, (3, 3), "dw/depthwise_weights") if use else g.conv(-1, (3, 3), 4, "c/weights")
            g.finalize(g.conv(g.pool(node, "avg"), (1, 1), 2, "fc/weights"))
            assert "depthwise_conv" not in vars(g) and callable(g.depthwise_conv)
            with pytest.raises(AttributeError, match="no_such_builder"):
                g.no_such_builder
            ref = weakref.ref(g)
            del g
            assert ref() is None, ("a Graph2D outlived its last reference", use)
    finally:
        if was:
            gc.enable()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(emu_lib):
    """Every construction-time refusal of tcr_g2d_depthwise_conv with its message; nothing is added to the graph and nothing is launched."""
    lib = emu_lib
    dev = Cm.device_of(lib)

    def refused(call, *what):
        with pytest.raises(T.TcrError) as e:
            call()
        assert all(w in str(e.value) for w in what), str(e.value)
        assert all(w.encode() in lib.tcr_last_error() for w in what)

    with Log(lib) as log:
        g = T.Graph2D("", 6, 5, 2, lib=lib, device=dev)
        refused(lambda: g.depthwise_conv(-1, (3, 3), "w", stride=(2, 1), rate=(1, 2)), "tcr_g2d_depthwise_conv", "dilation needs stride 1")
        refused(lambda: g.depthwise_conv(-1, (7, 3), "w", padding="VALID"), "tcr_g2d_depthwise_conv: 7x3 kernel does not fit the 6x5 input")
        refused(lambda: g.depthwise_conv(-1, (2, 2), "w", rate=(1, 5), padding="VALID"), "does not fit")
        refused(lambda: g.depthwise_conv(-1, (0, 3), "w"), "tcr_g2d_depthwise_conv: bad argument")
        refused(lambda: g.depthwise_conv(-1, (3, 3), "w", stride=(0, 1)), "tcr_g2d_depthwise_conv: bad argument")
        refused(lambda: g.depthwise_conv(-1, (3, 3), ""), "tcr_g2d_depthwise_conv: bad argument")
        refused(lambda: g.depthwise_conv(0, (3, 3), "w"), "tcr_g2d_depthwise_conv", "bad graph / input id")
        refused(lambda: g.depthwise_conv(-1, (33, 32), "w"), f"33x32 kernel has more than {K.MAX_TAPS} taps")
        assert not g.initializers and lib.tcr_g2d_workspace_bytes(g._h, 1, 0) == 0
        wide = T.Graph2D("", 40, 1100, 1, lib=lib, device=dev)
        refused(lambda: wide.depthwise_conv(-1, (4, 1), "w"), f"a window of 4 rows on a plane 1100 wide needs more than the {K.LDS_FLOATS} floats a tile stages")
        assert wide.depthwise_conv(-1, (3, 1), "w") == 0                                   # 3 x 1100 floats fit
        a = g.depthwise_conv(-1, (3, 3), "a/depthwise_weights")
        assert a == 0 and g.shape(a) == (2, 6, 5)                                           # the refusals added nothing
        g.finalize(g.conv(g.pool(a, "avg"), (1, 1), 3, "fc/weights"))
        refused(lambda: g.depthwise_conv(a, (3, 3), "late"), "bad graph / input id")
        assert g.tf_shape("a/depthwise_weights") == (3, 3, 2, 1) and g.tensors["a/depthwise_weights"].arena == 0
    assert not log.entries, log.entries
