"""The frozen table's weight image (tcr_net_fold_weights; kernels.h "weight image"): every conv layer's weights in the order a lane of the
fused eval kernel reads its matrix fragments, [layer][row tile m][tap j][c4 / 4][lane][width], so that the time-major kernel
(TCResNet8-1.0 at 49 frames, groups of 8) takes four channel quads of a tap with one 16-byte load.  Every MFMA sees the same operands in
the same order: logits and probabilities are BITWISE those of the 4-byte loads from `params` (TCR_TUNE_NET_FUSED = 13) and of the generic
runtime-shape kernel (3), on the GPU and on the emulator.

Groups of 8 are forced (TCR_TUNE_FUSED_GROUP) so that  batch 1, 7: dummy utterance slots;  8: one full group;  9: a full group and a tail
group of one;  21: several groups.  The edge case puts large features in the first two and last two frames only (the tiles with dead
taps, whose jobs start at a tap other than 0).  The default group policy at batch 1 and 64, 98 frames and TCResNet14-1.5 run kernels that
do not read the image: they must agree as before.

The contract of the flag: a table folded by tcr_net_fold_bn alone runs the old path; with the image folded the conv weights come from the
TABLE, so a weight written into `params` behind a kept table changes nothing until the caller folds again.

On the CPU the image is compared with a numpy gather of `params` by the index formula of include/tcresnet_hip.h, for every layer of
TCResNet8-1.0 and TCResNet14-1.5: the clamped rows (Cout = 24, 36, 72: no multiple of 16) and the narrow last groups (C4 = 6, 10: two
wide; C4 = 9: one wide) included."""
import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R

KNOB_NET_FUSED, KNOB_FUSED_GROUP = 3, 4
ARMS = (13, 3)
MAGIC = 0x474D4957
CONV1_0 = "TCResNet8/block1/conv1_0/weights"


def device_of(lib):
    return torch.device("cuda" if lib.kind == "hip" else "cpu")


def make_net(lib, scope="TCResNet8", width=1.0, frames=49, seed=4):
    net = T.TCResNet(scope, R.tcresnet_channels(scope, width), 40, frames, 12, lib=lib, device=device_of(lib))
    arch = R.make_tcresnet(scope, width)
    p, s = R.init_params(arch, seed)
    R.randomize_bn(arch, p, s)
    sd = dict(p); sd.update(s)
    net.load_state_dict(sd)
    return net


def random_features(lib, batch, frames=49, seed=0):
    x = np.random.RandomState(41 + batch + seed).uniform(-2, 2, (batch, frames, 40)).astype(np.float32)
    return T.features_to_planar(torch.from_numpy(x).to(device_of(lib)), lib=lib)


def edge_features(lib, batch):
    x = np.zeros((batch, 49, 40), np.float32)
    x[:, [0, 1, 47, 48], :] = np.random.RandomState(5).uniform(-40, 40, (batch, 4, 40)).astype(np.float32)
    return T.features_to_planar(torch.from_numpy(x).to(device_of(lib)), lib=lib)


class Knobs:
    def __init__(self, lib, group=0, arm=0):
        self.lib, self.group, self.arm = lib, group, arm

    def __enter__(self):
        self.lib.tcr_tune(KNOB_FUSED_GROUP, self.group)
        self.lib.tcr_tune(KNOB_NET_FUSED, self.arm)

    def __exit__(self, *exc):
        self.lib.tcr_tune(KNOB_NET_FUSED, 0)
        self.lib.tcr_tune(KNOB_FUSED_GROUP, 0)


def run(lib, net, x, group, arm, table=None):
    with Knobs(lib, group, arm):
        lg, pr = net.forward_infer(x) if table is None else net.forward_frozen(x, table)
        return lg.clone(), pr.clone()


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def flag_of(table, net):
    head = header_offset(net)
    return int(table[head:head + 1].cpu().numpy().view(np.uint32)[0])


def check_arms(lib, net, x, group):
    ref = run(lib, net, x, group, 0)
    assert flag_of(net._folded_table(), net) == MAGIC          # the engine's cached table carries the image
    lg, pr = ref
    assert lg.shape == (x.shape[0], 12) and torch.isfinite(lg).all() and float(lg.abs().max()) > 0
    assert torch.allclose(pr.sum(1), torch.ones_like(pr[:, 0]), atol=1e-5)
    for arm in ARMS:
        out = run(lib, net, x, group, arm)
        dl, dp = float((out[0] - lg).abs().max()), float((out[1] - pr).abs().max())
        print(f"batch {x.shape[0]} group {group} arm {arm}: max |d logits| {dl:.3g}, max |d probs| {dp:.3g}")
        assert same(out, ref), (x.shape[0], group, arm, dl, dp)
    return ref


def check_refold(lib):
    """load_state_dict with one conv weight changed: the engine folds again, the output changes and is again the generic kernel's."""
    net = make_net(lib)
    x = random_features(lib, 9)
    before = check_arms(lib, net, x, 8)
    w = net.state_dict()[CONV1_0]
    w[3, 0, 5, 17] += 0.5           # (tap 3, input channel 5, output channel 17: second row tile, second channel quad)
    net.load_state_dict({CONV1_0: w}, strict=False)
    after = check_arms(lib, net, x, 8)
    assert not torch.equal(after[0], before[0])


def check_flag_contract(lib):
    net = make_net(lib)
    x = random_features(lib, 9)
    ref = run(lib, net, x, 8, 0)
    # flag clear: the table of tcr_net_fold_bn alone runs the old path
    plain = net.fold_bn()
    assert flag_of(plain, net) == 0
    assert same(run(lib, net, x, 8, 0, plain), ref)
    # flag set: a kept table is the source of the conv weights, `params` is not
    kept = net._folded_table().clone()
    assert flag_of(kept, net) == MAGIC
    assert same(run(lib, net, x, 8, 0, kept), ref)
    with torch.no_grad():
        net._view(CONV1_0)[3, 0, 5, 17] += 0.5
    assert same(run(lib, net, x, 8, 0, kept), ref)                          # the documented contract: unchanged until folded again
    changed = run(lib, net, x, 8, 0, net.fold_bn())                         # the same weights through `params`
    assert not torch.equal(changed[0], ref[0])
    assert same(run(lib, net, x, 8, 0), changed)                            # the engine saw the write (tensor version) and folded again
    assert same(run(lib, net, x, 8, 13, kept), changed)                     # arm 13 reads `params` whatever the table carries


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 7, 8, 9, 21])
def test_image_loads_are_bitwise_the_dword_arm_and_the_generic_kernel(hip_lib, batch):
    check_arms(hip_lib, make_net(hip_lib), random_features(hip_lib, batch), 8)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 7, 8, 9, 21])
def test_features_at_the_edges_only(hip_lib, batch):
    check_arms(hip_lib, make_net(hip_lib), edge_features(hip_lib, batch), 8)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 64])
def test_default_group_policy(hip_lib, batch):
    check_arms(hip_lib, make_net(hip_lib), random_features(hip_lib, batch), 0)


@pytest.mark.gpu
def test_98_frames_still_agree(hip_lib):
    check_arms(hip_lib, make_net(hip_lib, frames=98), random_features(hip_lib, 9, frames=98), 0)


@pytest.mark.gpu
def test_tcresnet14_still_agrees(hip_lib):
    check_arms(hip_lib, make_net(hip_lib, "TCResNet14", 1.5), random_features(hip_lib, 9), 0)


@pytest.mark.gpu
def test_refold_after_load_state_dict(hip_lib):
    check_refold(hip_lib)


@pytest.mark.gpu
def test_flag_contract(hip_lib):
    check_flag_contract(hip_lib)


# ---- emulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [7, 9])
def test_image_loads_are_bitwise_on_the_emulator(emu_lib, batch):
    check_arms(emu_lib, make_net(emu_lib), random_features(emu_lib, batch), 8)


def test_features_at_the_edges_only_on_the_emulator(emu_lib):
    check_arms(emu_lib, make_net(emu_lib), edge_features(emu_lib, 9), 8)


def test_refold_on_the_emulator(emu_lib):
    check_refold(emu_lib)


def test_flag_contract_on_the_emulator(emu_lib):
    check_flag_contract(emu_lib)


def conv_units(net):
    """(name, k, cin, cout) of the BN'd conv layers in forward order: conv0, then per block [down], conv_0, conv_1."""
    scope = net.scope
    units = [f"{scope}/conv0"]
    for i in range(len(net.channels) - 1):
        if net.channels[i + 1] != net.channels[i]:
            units.append(f"{scope}/block{i}/down")
        units += [f"{scope}/block{i}/conv{i}_0", f"{scope}/block{i}/conv{i}_1"]
    out = []
    for u in units:
        k, _, cin, cout = net.tf_shape(u + "/weights")
        out.append((u, k, cin, cout))
    return out


def header_offset(net):
    """floats of the scale / shift block: per unit scale[c_pad], shift[c_pad], c_pad = Cout rounded up to 64; rounded up to 4"""
    n = sum(2 * ((cout + 63) // 64 * 64) for _, _, _, cout in conv_units(net))
    return (n + 3) // 4 * 4


def expected_image(net):
    sd = net.state_dict()
    parts = []
    for name, k, cin, cout in conv_units(net):
        w = sd[name + "/weights"].reshape(k, cin, cout)
        C4, nrt = cin // 4, (cout + 15) // 16
        img = np.full(nrt * k * C4 * 64, np.nan, np.float32)
        m, j, c4, lane = np.meshgrid(np.arange(nrt), np.arange(k), np.arange(C4), np.arange(64), indexing="ij")
        g = c4 // 4
        wd = np.minimum(4, C4 - 4 * g)
        at = ((m * k + j) * C4 + 4 * g) * 64 + lane * wd + (c4 - 4 * g)
        q, r = lane >> 4, lane & 15
        assert len(np.unique(at)) == img.size                                   # the formula fills the layer's image exactly once
        img[at] = w[j, 4 * c4 + q, np.minimum(16 * m + r, cout - 1)]
        parts.append(img)
    return np.concatenate(parts)


@pytest.mark.parametrize("scope,width", [("TCResNet8", 1.0), ("TCResNet14", 1.5)])
def test_image_is_the_gather_of_params_by_the_index_formula(emu_lib, scope, width):
    net = make_net(emu_lib, scope, width)
    head = header_offset(net)
    want = expected_image(net)
    assert int(emu_lib.tcr_net_frozen_floats(net._h)) == head + 4 + want.size
    table = net.fold_bn()
    raw = table.cpu().numpy()
    assert not raw[head:].any()                                                 # fold_bn alone: flag clear, no image
    emu_lib.check(emu_lib.tcr_net_fold_weights(net._h, net.params.data_ptr(), table.data_ptr(), None), "tcr_net_fold_weights")
    got = table.cpu().numpy()
    assert np.array_equal(got[:head], raw[:head])                               # scale / shift keep their offsets and contents
    assert list(got[head:head + 4].view(np.uint32)) == [MAGIC, want.size, 0, 0]
    assert np.array_equal(got[head + 4:], want)
    if scope == "TCResNet8":
        assert want.size == 16 * (3 * 40 + 2 * (16 + 9 * 16 + 9 * 24 + 24 + 9 * 24 + 9 * 32) + 3 * (32 + 9 * 32 + 9 * 48))


def test_engine_folds_both_under_one_key(emu_lib):
    net = make_net(emu_lib)
    table = net._folded_table()
    assert flag_of(table, net) == MAGIC and net._folded_table() is table
    assert np.array_equal(table.cpu().numpy()[header_offset(net) + 4:], expected_image(net))


def test_a_table_shorter_than_frozen_floats_is_refused(emu_lib):
    net = make_net(emu_lib)
    x = random_features(emu_lib, 2)
    short = net.fold_bn()[:header_offset(net)].clone()                          # scale / shift only: the size before the image existed
    with pytest.raises(T.TcrError, match="tcr_net_frozen_floats"):
        net.forward_frozen(x, short)
    with pytest.raises(T.TcrError, match="tcr_net_frozen_floats"):
        net.model_ref(short)


def test_an_artifact_of_scale_and_shift_only_gets_its_image_on_load(emu_lib):
    from tcresnet_amd import deploy
    net = make_net(emu_lib)
    head = header_offset(net)
    assert head == net.n_stat                                                   # what export_frozen keeps of fold_bn()
    meta = {"format": deploy.FORMAT, "model": "TCResNet8Model", "family": "tcresnet", "scope": net.scope, "channels": net.channels,
            "num_classes": 12, "include_preprocess": False, "height": 49, "width": 40, "bn_decay": float(net.cfg.bn_decay),
            "bn_eps": float(net.cfg.bn_eps), "inputs": [{"name": "input", "shape": [1, 49, 40, 1]}],
            "output": {"name": "output/softmax", "shape": [1, 12]}}
    consts = {k: v for k, v in net.state_dict().items() if k.endswith("/weights")}
    consts["__folded_batch_norm__"] = net.fold_bn()[:head].cpu().numpy()
    model = deploy.FrozenModel(meta, consts, lib=emu_lib, device=net.device)
    table = model.frozen_ss.cpu().numpy()
    assert table.size == int(emu_lib.tcr_net_frozen_floats(net._h))
    assert list(table[head:head + 4].view(np.uint32)) == [MAGIC, table.size - head - 4, 0, 0]
    assert np.array_equal(table[head + 4:], expected_image(net))
    feats = np.random.RandomState(3).uniform(-2, 2, (9, 49, 40, 1)).astype(np.float32)
    with Knobs(emu_lib, 8, 0):
        probs = model(torch.from_numpy(feats)).clone()
    assert torch.equal(probs, run(emu_lib, net, T.features_to_planar(torch.from_numpy(feats), lib=emu_lib), 8, 3)[1])
