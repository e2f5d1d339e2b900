"""The eval network kernel's time-major plan (fused.hip: fused_layer_tm; the default for groups of 8 utterances of TCResNet8-1.0 at 49
frames): positions ordered 8 * frame + utterance, LDS rows [channel][frame + halo][8], and the taps that read only SAME-padding zeros
for both frames of a 16-position tile not issued.  A skipped MFMA would have added products of finite weights with zeros to an
accumulator that starts at +0, and the live taps keep their order, so logits and probabilities are BITWISE those of the utterance-major
walk (TCR_TUNE_NET_FUSED = 12) and of the generic runtime-shape kernel (3) -- on the GPU (which also checks that the matrix cores pass an
untouched accumulator through unchanged) and on the emulator.

Groups of 8 are forced (TCR_TUNE_FUSED_GROUP) so that  batch 1, 7: dummy utterance slots;  8: one full group;  9: a full group and a tail
group of one;  16, 21: several groups.  At the default group policy batches 1 and 64 run one utterance per workgroup: the old walk.
The edge case puts large features in the first two and last two frames only: an off-by-one tap range changes every output.
The host's layout, the dead-tap table and the deal of the jobs are checked on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R

KNOB_NET_FUSED, KNOB_FUSED_GROUP = 3, 4
ARMS = (12, 3)
# TCResNet8-1.0 at 49 frames: (k, stride, cin, cout, tin) of the ten layers, and the six nine-tap layers of the issue's table
LAYERS = [(3, 1, 40, 16, 49), (1, 2, 16, 24, 49), (9, 2, 16, 24, 49), (9, 1, 24, 24, 25), (1, 2, 24, 32, 25), (9, 2, 24, 32, 25),
          (9, 1, 32, 32, 13), (1, 2, 32, 48, 13), (9, 2, 32, 48, 13), (9, 1, 48, 48, 7)]
NINE_TAP = {2: (6, 117, 48), 3: (10, 117, 120), 5: (6, 63, 72), 6: (10, 63, 160), 8: (6, 36, 144), 9: (10, 36, 360)}     # dead, all, MFMAs dropped


def same_pad_lo(k, s, tin):
    tout = (tin + s - 1) // s
    return max((tout - 1) * s + k - tin, 0) // 2


def make_net(lib, dev, random_bn):
    net = T.TCResNet("TCResNet8", R.tcresnet_channels("TCResNet8", 1.0), 40, 49, 12, lib=lib, device=dev)
    if random_bn:
        arch = R.make_tcresnet("TCResNet8", 1.0)
        p, s = R.init_params(arch, 4)
        R.randomize_bn(arch, p, s)
        sd = dict(p); sd.update(s)
        net.load_state_dict(sd)
    else:
        net.init_xavier(7)
    return net


def plan_of(lib, net, batch):
    out = (C.c_int * 64)()
    n = lib.tcr_net_fused_plan(net._h, batch, out, 64)
    assert n >= 6, n
    return list(out[:n])


def outputs_of_arms(lib, batch, group, feats=None, random_bn=False):
    dev = torch.device("cuda" if lib.kind == "hip" else "cpu")
    if feats is None:
        feats = np.random.RandomState(23 + batch).uniform(-2, 2, (batch, 49, 40)).astype(np.float32)
    x = T.features_to_planar(torch.from_numpy(feats).to(dev), lib=lib)
    net = make_net(lib, dev, random_bn)
    outs, tm = {}, {}
    try:
        lib.tcr_tune(KNOB_FUSED_GROUP, group)
        for knob in (0,) + ARMS:
            lib.tcr_tune(KNOB_NET_FUSED, knob)
            tm[knob] = plan_of(lib, net, batch)[0]
            lg, pr = net.forward_infer(x)
            outs[knob] = (lg.clone(), pr.clone())
    finally:
        lib.tcr_tune(KNOB_NET_FUSED, 0)
        lib.tcr_tune(KNOB_FUSED_GROUP, 0)
    return outs, tm


def check_bitwise(lib, batch, group, time_major, **kw):
    outs, tm = outputs_of_arms(lib, batch, group, **kw)
    assert tm[0] == (1 if time_major else 0) and tm[12] == 0 and tm[3] == 0, tm        # which walk ran
    lg, pr = outs[0]
    assert lg.shape == (batch, 12) and torch.isfinite(lg).all() and float(lg.abs().max()) > 0
    assert torch.allclose(pr.sum(1), torch.ones_like(pr[:, 0]), atol=1e-5)
    for knob in ARMS:
        dl, dp = float((outs[knob][0] - lg).abs().max()), float((outs[knob][1] - pr).abs().max())
        print(f"batch {batch} group {group} arm {knob}: max |d logits| {dl:.3g}, max |d probs| {dp:.3g}")
        assert torch.equal(outs[knob][0], lg), (batch, knob, "logits", dl)
        assert torch.equal(outs[knob][1], pr), (batch, knob, "probabilities", dp)


def edge_features(batch):
    x = np.zeros((batch, 49, 40), np.float32)
    x[:, [0, 1, 47, 48], :] = np.random.RandomState(5).uniform(-40, 40, (batch, 4, 40)).astype(np.float32)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 7, 8, 9, 16, 21])
def test_time_major_is_bitwise_the_old_walk_and_the_generic_kernel(hip_lib, batch):
    check_bitwise(hip_lib, batch, 8, True)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 64])
def test_the_default_group_policy_keeps_the_old_walk_at_small_batches(hip_lib, batch):
    check_bitwise(hip_lib, batch, 0, False)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [9, 16])
def test_features_at_the_edges_only(hip_lib, batch):
    check_bitwise(hip_lib, batch, 8, True, feats=edge_features(batch), random_bn=True)


@pytest.mark.parametrize("batch", [1, 7, 8, 9, 16, 21])
def test_time_major_is_bitwise_on_the_emulator(emu_lib, batch):
    check_bitwise(emu_lib, batch, 8, True)


@pytest.mark.parametrize("batch", [1, 64])
def test_the_default_group_policy_keeps_the_old_walk_on_the_emulator(emu_lib, batch):
    check_bitwise(emu_lib, batch, 0, False)


def test_features_at_the_edges_only_on_the_emulator(emu_lib):
    check_bitwise(emu_lib, 9, 8, True, feats=edge_features(9), random_bn=True)


def test_layout_pitches_and_two_workgroups_per_cu(emu_lib):
    net = make_net(emu_lib, torch.device("cpu"), False)
    tm, group, waves, lds, per_cu, n_layers, *rows = plan_of(emu_lib, net, 4096)
    assert (tm, group, waves, n_layers) == (1, 8, 8, 10)
    assert 2 * lds <= 160 * 1024 and per_cu >= 2, (lds, per_cu)               # lds_of(8) <= 81 920 B
    for i, (k, s, cin, cout, tin) in enumerate(LAYERS):
        out_p, in_p, res_p, reader = rows[4 * i:4 * i + 4]
        tout = (tin + s - 1) // s
        if reader == 0:                                     # shortcut outputs, the pooled block output: no halo, no pad
            assert out_p == 8 * tout, (i, out_p)
        else:
            assert out_p >= 8 * (tout + 8) and out_p % 32 == (16 if reader == 1 else 8), (i, out_p, reader)
        if i > 0:
            assert in_p >= 8 * (tin + 8) and in_p % 32 == (16 if s == 1 else 8), (i, in_p, s)     # its own reads are conflict-free
        if i in (3, 6, 9):
            assert res_p == 8 * tout, (i, res_p)
    emu_lib.tcr_tune(KNOB_NET_FUSED, 12)
    try:
        assert plan_of(emu_lib, net, 4096)[:2] == [0, 8]
    finally:
        emu_lib.tcr_tune(KNOB_NET_FUSED, 0)


def brute_force_live(k, s, tin, tile):
    """taps of a tile that read at least one real input frame, over (tap, frame)"""
    tout, pad_lo = (tin + s - 1) // s, same_pad_lo(k, s, tin)
    return [j for j in range(k) if any(0 <= t * s + j - pad_lo < tin for t in (2 * tile, 2 * tile + 1) if t < tout)]


def test_dead_tap_table_is_the_brute_force_count(emu_lib):
    dropped_all = 0
    for i, (k, s, cin, cout, tin) in enumerate(LAYERS):
        tout = (tin + s - 1) // s
        dead = 0
        for tile in range((tout + 1) // 2):
            out = (C.c_int * 2)()
            assert emu_lib.tcr_fused_tm_taps(k, s, tin, same_pad_lo(k, s, tin), tile, out) == 0
            live = brute_force_live(k, s, tin, tile)
            assert live == list(range(out[0], out[1] + 1)), (i, tile, live, out[0], out[1])
            dead += k - len(live)
        if i in NINE_TAP:
            n_dead, n_all, mfmas = NINE_TAP[i]
            assert (dead, k * ((tout + 1) // 2)) == (n_dead, n_all), (i, dead)
            assert dead * ((cout + 15) // 16) * (cin // 4) == mfmas, i
            dropped_all += mfmas
        elif k == 1:
            assert dead == 0
    assert dropped_all == 904
    bad = (C.c_int * 2)()
    assert emu_lib.tcr_fused_tm_taps(9, 1, 7, 4, 4, bad) == -1


@pytest.mark.parametrize("nw", [4, 8, 16])
def test_jobs_are_dealt_once_and_walk_the_live_taps_of_their_tiles(emu_lib, nw):
    for i, (k, s, cin, cout, tin) in enumerate(LAYERS[1:], 1):
        tout, pad_lo = (tin + s - 1) // s, same_pad_lo(k, s, tin)
        nrt, nt16 = (cout + 15) // 16, (tout + 1) // 2
        seen = np.zeros((nrt, nt16), np.int64)
        cost = np.zeros(nw, np.int64)
        issued, biggest = 0, 0
        for wave in range(nw):
            jobs, mfma = (C.c_uint * 8)(), C.c_int(0)
            n = emu_lib.tcr_fused_tm_deal(k, s, cin, cout, tin, pad_lo, nw, wave, jobs, 8, C.byref(mfma))
            assert 0 <= n <= 8, (i, wave, n)
            for w in jobs[:n]:
                m, c, pair, lo, hi = w & 15, w >> 4 & 63, w >> 10 & 1, w >> 11 & 15, w >> 15 & 15
                live = set()
                for cc in range(c, c + 1 + pair):
                    live |= set(brute_force_live(k, s, tin, cc))
                    seen[m, cc] += 1
                # no live tap of a tile is skipped, and no tap is walked that is dead for every tile of the job
                assert sorted(live) == list(range(lo, hi + 1)), (i, wave, c, pair, lo, hi, live)
                c_job = (hi - lo + 1) * (8 if pair else 7) + 8          # kernels.h: a pair's tap, a single tile's tap, the prologue
                cost[wave] += c_job
                biggest = max(biggest, c_job)
                issued += (hi - lo + 1) * (1 + pair) * (cin // 4)
        assert np.all(seen == 1), (i, seen)
        full = nrt * nt16 * k * (cin // 4)
        assert issued == mfma.value == full - NINE_TAP.get(i, (0, 0, 0))[2], (i, issued, mfma.value, full)         # every dead tap is skipped
        simd = np.array([cost[s_::4].sum() for s_ in range(4)])               # a SIMD hosts waves s, s + 4, ...
        assert simd.max() - simd.min() <= biggest, (i, simd, cost)            # longest-first dealing: within one job
