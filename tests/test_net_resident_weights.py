"""The eval network kernel's resident-weight walk (fused.hip: fused_layer_r, fused_resident_request; conv0_1 of TCResNet8-1.0's
static kernel; the default at 49 frames, TCR_TUNE_NET_FUSED = 11 at either frame count) against the round-6 walk (10; the default at 98
frames) and the generic `net_fused_kernel` (3): every form accumulates an output tile tap-major, channel quads inner, out of the same fragments, and the columns
of the implicit GEMM are independent, so logits and probabilities are BITWISE equal -- on the GPU and, for two batches, on the emulator.

Groups of 8 utterances are forced (TCR_TUNE_FUSED_GROUP: small batches would otherwise run one utterance per workgroup), so that
  batch 1: 25 positions in block 0 = two position tiles, four units -- half the waves have an empty run and still reach the barriers
           with their weight requests retired;
  batch 7 / 8: a short and a full group;  batch 9: a second group of one;  batch 21: a ragged third group.
Runs are re-dealt so that none straddles two row tiles (kernels.h: fused_deal_run); the dealing function is checked on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R

KNOB_NET_FUSED, KNOB_FUSED_GROUP = 3, 4
ARMS = (11, 10, 3)          # the resident walk, the round-6 walk, the generic kernel


def outputs_of_every_arm(lib, batch, t, seed=9):
    dev = torch.device("cuda" if lib.kind == "hip" else "cpu")
    rng = np.random.RandomState(seed)
    x = T.features_to_planar(torch.from_numpy(rng.uniform(-2, 2, (batch, t, 40)).astype(np.float32)).to(dev), lib=lib)
    net = T.TCResNet("TCResNet8", R.tcresnet_channels("TCResNet8", 1.0), 40, t, 12, lib=lib, device=dev)
    net.init_xavier(3)
    outs = {}
    try:
        lib.tcr_tune(KNOB_FUSED_GROUP, 8)
        for knob in (0,) + ARMS:
            lib.tcr_tune(KNOB_NET_FUSED, knob)
            lg, pr = net.forward_infer(x)
            outs[knob] = (lg.clone(), pr.clone())
    finally:
        lib.tcr_tune(KNOB_NET_FUSED, 0)
        lib.tcr_tune(KNOB_FUSED_GROUP, 0)
    return outs


def check_bitwise(lib, batch, t):
    outs = outputs_of_every_arm(lib, batch, t)
    lg, pr = outs[0]
    assert lg.shape == (batch, 12) and torch.isfinite(lg).all() and float(lg.abs().max()) > 0
    assert torch.allclose(pr.sum(1), torch.ones_like(pr[:, 0]), atol=1e-5)
    for knob in ARMS:
        assert torch.equal(outs[knob][0], lg), (batch, t, knob, "logits", float((outs[knob][0] - lg).abs().max()))
        assert torch.equal(outs[knob][1], pr), (batch, t, knob, "probabilities", float((outs[knob][1] - pr).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("t", [49, 98])
@pytest.mark.parametrize("batch", [1, 7, 8, 9, 21])
def test_resident_walk_is_bitwise_the_old_walk_and_the_generic_kernel(hip_lib, batch, t):
    check_bitwise(hip_lib, batch, t)


@pytest.mark.parametrize("t", [49, 98])
@pytest.mark.parametrize("batch", [1, 9])
def test_resident_walk_is_bitwise_on_the_emulator(emu_lib, batch, t):
    check_bitwise(emu_lib, batch, t)


@pytest.mark.parametrize("nw", [4, 8, 16])
@pytest.mark.parametrize("nrt,nt16", [(2, 2), (1, 13), (2, 13), (2, 25)])          # U = 4, 13, 26, 50 units
def test_units_are_dealt_once_and_no_run_spans_two_row_tiles(emu_lib, nrt, nt16, nw):
    seen = np.zeros((nrt, nt16), np.int64)
    length = np.zeros(nw, np.int64)
    for wave in range(nw):
        out = (C.c_int * 3)()
        assert emu_lib.tcr_fused_deal_run(nrt, nt16, nw, wave, out) == 0
        m, c0, c1 = out[0], out[1], out[2]
        assert 0 <= m < nrt and 0 <= c0 <= c1 <= nt16, (wave, m, c0, c1)       # one row tile, a run inside its columns
        seen[m, c0:c1] += 1
        length[wave] = c1 - c0
    assert np.all(seen == 1), seen
    assert length.max() - length.min() <= 1, length
    simd = np.array([length[s::4].sum() for s in range(4)])                   # a SIMD hosts waves s, s + 4, ...
    assert simd.max() - simd.min() <= 1, (simd, length)                       # the longer runs are rotated from row tile to row tile
    bad = (C.c_int * 3)()
    assert emu_lib.tcr_fused_deal_run(3, 5, 8, 0, bad) == -1 and emu_lib.tcr_fused_deal_run(2, 5, 8, 8, bad) == -1
