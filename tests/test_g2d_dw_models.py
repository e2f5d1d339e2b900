"""The configurable DS-CNN on the 2-D graph engine (audio_nets/ds_cnn.py::build_graph, factory DSCNNModel): the S definition as a twin of
engine.DSCNN("S") against oracle.dscnn_ref; the definitions the DS-CNN engine refuses -- built, evaluated and trained one step against
the oracle, next to the engine's refusal; the model class through training, evaluation, freezing and a scan.  Tolerances and helpers are
tests/test_g2d_configs.py's.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import dscnn_ref as D
from oracle import numpy_ref as R
from tests import common as Cm
from tests import test_g2d_configs as TG
from tests.test_g2d_configs import LOSS_TOL
from tests.test_net_configs import PROB_TOL

TAU = 1e-5      # oracle.net2d_ref.KINK_LOG's: a ReLU input this close to zero may fall on either side in float32


def f32(d):
    return {k: np.asarray(v, np.float32) for k, v in d.items()}


def make_twin(lib, blocks, h, w, seed, **kw):
    from tcresnet_amd.audio_nets import ds_cnn
    p, s = D.init_params(blocks, 12, seed=seed)
    p, s = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}, {k: v.astype(np.float32).astype(np.float64) for k, v in s.items()}
    conv1, seps = blocks[0], blocks[1:]
    args = dict(depth=conv1.depth, num_separable=len(seps), conv1_kernel=conv1.kernel, conv1_stride=conv1.stride,
                ds_kernel=seps[0].kernel, ds1_stride=seps[0].stride, ds_rate=(1, 1))
    args.update(kw)
    twin = ds_cnn.build_graph(h=h, w=w, num_classes=12, lib=lib, device=Cm.device_of(lib), **args)
    twin.load_state_dict(f32({**p, **s}))
    return twin, p, s


def check_against_oracle(lib, twin, blocks, p, s, h, w, batch, what):
    """Eval logits / probabilities, then training forward + backward of the twin against oracle.dscnn_ref, the ReLU inputs within TAU of
    zero taken on the twin's side (at most 2 + 1e-4 of them, on the float64 reference alone); then one Adam step runs."""
    x = np.random.RandomState(7).uniform(-2.0, 2.0, (batch, h, w)).astype(np.float32)
    x64 = x.astype(np.float64)
    feat = TG.planar(lib, x)
    labels = R.synth_labels(batch).astype(np.float64)
    ref = D.forward(blocks, p, s, x64, False)
    lg, pr = twin.forward_infer(feat)
    e = {"eval_logits": float(np.abs(lg.cpu().numpy() - ref["logits"]).max()), "eval_probs": float(np.abs(pr.cpu().numpy() - ref["probs"]).max())}
    assert e["eval_logits"] < Cm.LOGIT_TOL and e["eval_probs"] < PROB_TOL, (what, e)
    tl, tp, loss = [v.clone() for v in twin.forward_train(feat, Cm.to_dev(lib, labels), seed=3)]
    fwd = D.forward(blocks, p, s, x64, True)
    # the twin's ReLU nodes in build order: conv_1's BN, then per block the depthwise BN ("mid") and the pointwise BN ("out")
    keys = [("conv_1/out", "DSCNN/conv_1/batch_norm")]
    for b in blocks[1:]:
        keys += [(f"{b.scope}/mid", f"DSCNN/{b.scope}/dw_batch_norm"), (f"{b.scope}/out", f"DSCNN/{b.scope}/pw_batch_norm")]
    assert len(keys) == len(twin.relu_nodes)
    masks, near, total = {}, 0, 0
    for (key, prefix), node in zip(keys, twin.relu_nodes):
        z = fwd["cache"][prefix]["xhat"] + p[prefix + "/beta"]
        kept = (twin.node_output(node, batch, True) > 0).cpu().numpy().transpose(0, 2, 3, 1)
        close = np.abs(z) < TAU
        near, total = near + int(close.sum()), total + z.size
        masks[key] = np.where(close, kept, z > 0)
    assert near <= 2 + 1e-4 * total, (what, "ReLU inputs within tau of zero", near, "of", total)
    grads = D.backward(blocks, p, fwd, labels, masks)
    e["train_logits"] = float(np.abs(tl.cpu().numpy() - fwd["logits"]).max())
    e["loss"] = abs(float(loss) / batch - D.loss(fwd["logits"], labels))
    assert e["train_logits"] < Cm.LOGIT_TOL and e["loss"] < LOSS_TOL, (what, e)
    e["stats"] = TG.stat_errors(lambda k: twin._view(k).cpu().numpy(), {k: v for k, v in fwd["new_stats"].items()}, what)
    twin.backward()
    e["grads"] = TG.grad_errors(lambda k: twin.grad_view(k).cpu().numpy(), twin.tensors, grads, what)
    before = twin.params.clone()
    twin.adam_step(1e-3, 1)
    assert bool(torch.isfinite(twin.params).all()) and not torch.equal(before, twin.params), what
    print("G2D_DW_TWIN_ERR", what, e)
    return e


def check_twin(lib):
    """DS-CNN-S at 49 x 10, 12 classes: one state_dict in engine.DSCNN("S") and in the graph twin (loaded into the twin and back); both
    eval forwards within LOGIT_TOL of the oracle; the twin's training step against the oracle's backward."""
    blocks = D.net_def("S")
    twin, p, s = make_twin(lib, blocks, 49, 10, 3)
    eng = T.DSCNN("S", 49, 10, 12, lib=lib, device=Cm.device_of(lib))
    eng.load_state_dict(twin.state_dict())                                  # the twin's dict loads into the engine ...
    sd = eng.state_dict()
    assert set(sd) == set(twin.state_dict()) and all(np.array_equal(np.ravel(sd[k]), np.ravel(v)) for k, v in twin.state_dict().items())
    assert twin.tf_shape("DSCNN/conv_ds_1/depthwise_conv/depthwise_weights") == (3, 3, 64, 1) and twin.state_dict()["DSCNN/fc1/weights"].shape == (64, 12)
    twin.load_state_dict(sd)                                                # ... and back
    x = np.random.RandomState(7).uniform(-2.0, 2.0, (3, 49, 10)).astype(np.float32)
    ref = D.forward(blocks, p, s, x.astype(np.float64), False)
    lg = eng.forward_infer(TG.planar(lib, x))[0]
    assert float(np.abs(lg.cpu().numpy() - ref["logits"]).max()) < Cm.LOGIT_TOL
    check_against_oracle(lib, twin, blocks, p, s, 49, 10, 3, "twin S")


def test_twin_of_dscnn_s(emu_lib):
    check_twin(emu_lib)


@pytest.mark.gpu
def test_gpu_twin_of_dscnn_s(hip_lib):
    check_twin(hip_lib)


def dscnn_refuses(lib, h, w, depth, nsep, conv1=(10, 4), *what):
    """tcr_dscnn_create with this definition: refused with `what` in the message (None: created; the handle is returned)."""
    cfg = T.engine.DSCNNCfg(h, w, 12, depth, nsep, conv1[0], conv1[1], 2, 2, 1, 1, 0.96, 0.001)
    handle = C.c_void_p()
    rc = lib.tcr_dscnn_create(C.byref(cfg), C.byref(handle))
    if not what:
        assert rc == 0, lib.tcr_last_error()
        lib.tcr_dscnn_destroy(handle)
        return
    assert rc < 0 and all(w_.encode() in lib.tcr_last_error() for w_ in what), (rc, lib.tcr_last_error())


# (id, h, w, batch, depth, separable blocks, conv_1 kernel, depthwise kernel)
BEYOND = [("depth30", 25, 10, 3, 30, 2, (10, 4), (3, 3)), ("nine_blocks", 25, 10, 3, 8, 9, (10, 4), (3, 3)), ("conv1_10x8", 25, 10, 3, 8, 2, (10, 8), (3, 3)),
          ("ds_5x5", 25, 10, 3, 8, 2, (10, 4), (5, 5)), ("ds_9x1", 25, 10, 3, 8, 2, (10, 4), (9, 1)), ("train_98x40", 98, 40, 2, 8, 2, (10, 4), (3, 3))]


def check_beyond(lib, case):
    """A definition the DS-CNN engine refuses: the graph builds, evaluates and trains one step against the oracle; next to it the refusal.
    For the 5 x 5 and 9 x 1 depthwise kernels the refusal is not `tcr_dscnn_create`'s: tcr_dscnn_cfg has no field for a depthwise kernel,
    so no call can ask the engine for one.  What is asserted instead: the configuration has no such field, the engine built from the
    rest of the definition holds 3 x 3 depthwise weights, and it refuses the graph's state_dict with the shape mismatch in the message."""
    name, h, w, batch, depth, nsep, conv1, dsk = case
    blocks = [D.DsBlock("conv", depth, conv1, (2, 2), "conv_1")] + [D.DsBlock("separable", depth, dsk, (1, 1), f"conv_ds_{i}") for i in range(1, nsep + 1)]
    twin, p, s = make_twin(lib, blocks, h, w, 5)
    check_against_oracle(lib, twin, blocks, p, s, h, w, batch, name)
    if name == "depth30":
        dscnn_refuses(lib, h, w, depth, nsep, conv1, "depth 30 must be a positive multiple of 4")
    elif name == "nine_blocks":
        dscnn_refuses(lib, h, w, depth, nsep, conv1, "n_separable 9 out of range")
    elif name == "conv1_10x8":
        dscnn_refuses(lib, h, w, depth, nsep, conv1, "conv_1 kernel must be kh x 4 (got 10 x 8)")
    elif name.startswith("ds_"):
        # its depthwise kernel is 3 x 3 by construction: the configuration has no field for another
        assert not [f for f, _ in T.engine.DSCNNCfg._fields_ if f.startswith("ds_k") or f.startswith("dw_k")]
        dscnn_refuses(lib, h, w, depth, nsep, conv1)
        eng = T.DSCNN(None, h, w, 12, lib=lib, device=Cm.device_of(lib), net_def=(depth, nsep, (2, 2), (1, 1)))
        assert eng.tf_shape("DSCNN/conv_ds_1/depthwise_conv/depthwise_weights") == (3, 3, depth, 1)
        with pytest.raises(T.TcrError, match=rf"depthwise_weights: shape \({dsk[0]}, {dsk[1]}, {depth}, 1\) != \(3, 3, {depth}, 1\)"):
            eng.load_state_dict(twin.state_dict())
    else:
        eng = T.DSCNN(None, h, w, 12, lib=lib, device=Cm.device_of(lib), net_def=(depth, nsep, (2, 2), (1, 1)))
        with pytest.raises(T.TcrError, match="3072 floats"):
            eng.train_workspace(batch)


@pytest.mark.parametrize("case", BEYOND, ids=[c[0] for c in BEYOND])
def test_definitions_the_dscnn_engine_refuses(emu_lib, case):
    check_beyond(emu_lib, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", BEYOND, ids=[c[0] for c in BEYOND])
def test_gpu_definitions_the_dscnn_engine_refuses(hip_lib, case):
    check_beyond(hip_lib, case)


# ---- the public layers ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def rt(request):
    from tcresnet_amd import runtime
    from tcresnet_amd.audio_nets import tc_resnet
    lib = request.getfixturevalue("emu_lib" if request.param == "emu" else "hip_lib")
    runtime.set_default(lib, "cpu" if request.param == "emu" else "cuda")
    tc_resnet.reset_engines()
    yield lib
    runtime.set_default(None, None)
    tc_resnet.reset_engines()


def test_available_nets_unchanged():
    from tcresnet_amd.factory import audio_nets
    assert audio_nets._available_nets == ["KWSModel", "Res8Model", "Res8NarrowModel", "Res15Model", "Res15NarrowModel", "DSCNNSModel", "DSCNNMModel",
                                          "DSCNNLModel", "TCResNet8Model", "TCResNet14Model", "ResNet2D8Model", "ResNet2D8PoolModel"]
    assert audio_nets._extension_nets == ["DSCNNModel"] and issubclass(audio_nets.DSCNNModel, audio_nets._GraphModel)


def test_model_class_trains_evaluates_freezes_and_scans(rt, tmp_path):
    """DSCNNModel through the command lines: three optimisation steps on the synthetic dataset, evaluation from the checkpoint, freeze.py
    and FrozenModel.load rebuilding the same engine from the scalar flags (equal logits), then a frozen artifact with its front-end:
    three steps of a scan are bitwise forward_infer on the clips cut from the signal."""
    from tcresnet_amd import deploy, evaluate_audio, freeze, train_audio
    from tcresnet_amd.audio_nets import ds_cnn, tc_resnet
    from tcresnet_amd.factory import audio_nets
    from tests.test_boundary import REF_EVAL_CMD, REF_TRAIN_CMD, _model_args
    from tests.test_streaming import segment_audio
    dev = Cm.device_of(rt)
    flags = "DSCNNModel --depth 32 --num_separable 2 --conv1_kernel 6x4 --conv1_stride 2x1 --ds_kernel 5x3 --ds1_stride 1x1 --ds_rate 1x1"
    fe_flags, mf = "--window_size_ms 60 --window_stride_ms 60", "--num_mfccs 12"
    swap = lambda cmd: (cmd.replace("--window_size_ms 40 --window_stride_ms 20", fe_flags).replace("--num_mfccs 40", mf)
                        .replace("TCResNet8Model --weight_decay 0.001 --width_multiplier 1.0", flags))
    cmd = (swap(REF_TRAIN_CMD).replace("--optimizer mom --momentum 0.9", "--optimizer adam").replace("--lr_list 0.1 0.01 0.001", "--lr_list 0.001 0.001 0.001"))
    tr = train_audio.train(train_audio.parse_arguments(cmd.format(d=tmp_path).split()))
    assert tr.global_step == 3 and np.isfinite(float(tr.model.total_loss))
    eng = tr.model.engine
    assert isinstance(eng, T.Graph2D) and eng.tf_shape("DSCNN/conv_ds_2/depthwise_conv/depthwise_weights") == (5, 3, 32, 1)
    h, w = eng.h_in, eng.w_in
    out = evaluate_audio.main(evaluate_audio.parse_arguments(swap(REF_EVAL_CMD).format(d=tmp_path).split()))
    assert out["step"] == 3 and out["num_evaluated"] == 6 and np.isfinite(out["total_loss"])
    fcmd = (f"--checkpoint_path {tmp_path / 'DSCNNModel-3'} --output_name output/softmax --num_classes 12 --preprocess_method no_preprocessing "
            f"--height {h} --width {w} --channels 1 {fe_flags} {mf} {flags}")
    path = freeze.freeze(freeze.parse_arguments(fcmd.split()))
    trained = ds_cnn.get_engine(32, 2, "6x4", "2x1", "5x3", "1x1", "1x1", h, w, 12)        # (the cached engine the checkpoint was restored into)
    x = torch.randn(3, h, w, 1, device=dev)
    want_logits, want_probs = [v.clone() for v in trained.forward_infer(T.features_to_planar(x, lib=rt))]
    tc_resnet.reset_engines()
    frozen = deploy.FrozenModel.load(path, lib=rt, device=dev)
    assert frozen.meta["model"] == "DSCNNModel" and frozen.meta["args"]["ds_kernel"] == "5x3" and frozen.engine is not trained
    got_logits, got_probs = frozen.engine.forward_infer(T.features_to_planar(x, lib=rt))
    assert torch.equal(got_logits, want_logits) and torch.equal(frozen(x), want_probs)
    # with the front-end: scan a short signal
    args = _model_args(window_size_ms=60.0, window_stride_ms=60.0, num_mfccs=12, weight_decay=0.0, depth=32, num_separable=2, conv1_kernel="6x4",
                       conv1_stride="2x1", ds_kernel="5x3", ds1_stride="1x1", ds_rate="1x1")
    model = audio_nets.DSCNNModel(args)
    model.build_deployable_model(include_preprocess=True)
    model.engine.load_state_dict(trained.state_dict())
    art = model.freeze()
    art.meta["frontend"]["method"] = "mfcc"             # (the training front-end: the float64 deploy path has no streaming instance)
    art.save(str(tmp_path / "with_pre.pb"))
    tc_resnet.reset_engines()
    fz = deploy.FrozenModel.load(str(tmp_path / "with_pre.pb"), lib=rt, device=dev)
    fe, net = fz.frontend, fz.engine
    step, steps = fe.cfg.hop, 20
    audio = Cm.to_dev(rt, segment_audio(2, steps * step, 3))
    scan = fz.scanner(frames_per_step=1, average_window_ms=120, min_count=1, detection_threshold=0.0, suppression_ms=120).scan(audio)
    logits, probs = scan[0], scan[1]
    assert logits.shape[:2] == (2, steps)
    padded = torch.cat([torch.zeros((2, fe.n_samples), dtype=torch.float32, device=audio.device), audio], dim=1)
    for i in (0, 7, steps - 1):
        clip = padded[:, (i + 1) * step:(i + 1) * step + fe.n_samples].contiguous()
        lo, pr = net.forward_infer(fe(clip))
        assert torch.equal(logits[:, i], lo) and torch.equal(probs[:, i], pr), (i, float((logits[:, i] - lo).abs().max()))
