"""The eval network kernels' per-job bookkeeping (fused.hip: fused_job_s, fused_layer_r -- scale / shift and rolled-path weights through
buffer descriptors, a lane's four output channels clamped as one quad, one store address per tile with a channel pitch that is 0 in the
lanes that store into the pad) moves no output bit: it touches no activation, no weight value and no MFMA order.  Logits and
probabilities are compared BITWISE between the default kernel and the A/B arms of TCR_TUNE_NET_FUSED that share the changed walkers in
other combinations (8 jobs of two tiles dealt round-robin, 9 units without the weight lookahead, 10 the round-6 walk in conv0_1, 11 the
resident walk at either frame count) and the generic runtime-shape kernel (3), which the change does not touch.

Groups of 8 utterances are forced (TCR_TUNE_FUSED_GROUP) for the batches below, so that
  batch 1 - 3:  runs of zero or one unit and a clamped last tile in every block; with 7 output frames (block 2 at 49 frames) a tile of 16
                positions spans more than two utterances, or a clamped tail of one;
  batch 5, 13:  a ragged number of positions modulo 32: the stride-1 layers end in a tile of consecutive positions;
  batch 8, 9:   a full group, and a full group plus a group of one;  batch 21: a ragged third group;
  every batch:  24 output channels (block 0) leave the upper half of row tile 1 beyond Cout -- those lanes store into the pad.
At the default group policy batch 1 and 64 take the small-batch kernel (one utterance per workgroup, weights in LDS: the pointer form of
the rolled-path weights) -- compared against the generic kernel (3).  TCResNet14-1.5's static kernel shares the walkers."""
import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R

KNOB_NET_FUSED, KNOB_FUSED_GROUP = 3, 4
ARMS = (3, 8, 9, 10, 11)


def outputs_of_arms(lib, model, width, batch, t, group, arms, seed=11):
    dev = torch.device("cuda" if lib.kind == "hip" else "cpu")
    rng = np.random.RandomState(seed + batch)
    x = T.features_to_planar(torch.from_numpy(rng.uniform(-2, 2, (batch, t, 40)).astype(np.float32)).to(dev), lib=lib)
    net = T.TCResNet(model, R.tcresnet_channels(model, width), 40, t, 12, lib=lib, device=dev)
    net.init_xavier(5)
    outs = {}
    try:
        lib.tcr_tune(KNOB_FUSED_GROUP, group)
        for knob in (0,) + tuple(arms):
            lib.tcr_tune(KNOB_NET_FUSED, knob)
            lg, pr = net.forward_infer(x)
            outs[knob] = (lg.clone(), pr.clone())
    finally:
        lib.tcr_tune(KNOB_NET_FUSED, 0)
        lib.tcr_tune(KNOB_FUSED_GROUP, 0)
    return outs


def check_bitwise(lib, model, width, batch, t, group, arms):
    outs = outputs_of_arms(lib, model, width, batch, t, group, arms)
    lg, pr = outs[0]
    assert lg.shape == (batch, 12) and torch.isfinite(lg).all() and float(lg.abs().max()) > 0
    assert torch.allclose(pr.sum(1), torch.ones_like(pr[:, 0]), atol=1e-5)
    for knob in arms:
        dl, dp = float((outs[knob][0] - lg).abs().max()), float((outs[knob][1] - pr).abs().max())
        print(f"{model}-{width} batch {batch} T {t} group {group} arm {knob}: max |d logits| {dl:.3g}, max |d probs| {dp:.3g}")
        assert torch.equal(outs[knob][0], lg), (batch, t, knob, "logits", dl)
        assert torch.equal(outs[knob][1], pr), (batch, t, knob, "probabilities", dp)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [49, 98])
@pytest.mark.parametrize("batch", [1, 2, 3, 5, 8, 9, 13, 21])
def test_every_arm_is_bitwise_the_default_at_groups_of_eight(hip_lib, batch, t):
    check_bitwise(hip_lib, "TCResNet8", 1.0, batch, t, 8, ARMS)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [49, 98])
@pytest.mark.parametrize("batch", [1, 64])
def test_every_arm_is_bitwise_the_default_at_the_default_group_policy(hip_lib, batch, t):
    check_bitwise(hip_lib, "TCResNet8", 1.0, batch, t, 0, ARMS)


@pytest.mark.gpu
def test_tcresnet14_static_kernel_is_bitwise_the_generic_kernel(hip_lib):
    check_bitwise(hip_lib, "TCResNet14", 1.5, 9, 49, 8, (3,))


@pytest.mark.parametrize("t", [49, 98])
@pytest.mark.parametrize("batch", [1, 9])
def test_every_arm_is_bitwise_the_default_on_the_emulator(emu_lib, batch, t):
    check_bitwise(emu_lib, "TCResNet8", 1.0, batch, t, 8, ARMS)
