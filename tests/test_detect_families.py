"""Streaming detection, scans, many-step pushes and sweeps on DS-CNN and 2-D graph models (tcr_model_ref and the _m entries of
include/tcresnet_hip.h): a push's logits / probs are bitwise the engine's `forward_infer` of the stream windows at batch S, the
detector follows its rule, a scan is bitwise the pushes of a fresh detector, `push_many` is bitwise the pushes, and the entries
without _m are the _m entries with a TC-ResNet reference.  Emulator (`-m "not gpu"`, small models) and MI355X (`-m gpu`)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import assert_bitwise, pushed
from tests.test_streaming import Clips, RefDetector, compare_detector, segment_audio, setup, write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET = dict(average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=200)


def randomise(eng, seed):
    """Non-trivial values for the BN / bias variables and moving statistics (weights keep their initializer)."""
    rng = np.random.RandomState(seed)
    sd = {k: v for k, v in eng.state_dict().items() if k in eng.tensors}
    for k, v in sd.items():
        ti = eng.tensors[k]
        if ti.kind == 0:
            continue
        if ti.kind in (1, 4):
            sd[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith("bias") or k.endswith("biases"):
            sd[k] = rng.uniform(-0.05, 0.05, v.shape).astype(np.float32)
        else:
            sd[k] = rng.uniform(-0.5, 0.5, v.shape).astype(np.float32)
    eng.load_state_dict(sd)


def dscnn(lib, size="S", win=640, hop=320, mfccs=10, seed=0):
    fe = Cm.make_frontend(lib, win, hop, num_mfccs=mfccs)
    net = T.DSCNN(size, fe.n_frames, fe.n_coef, 12, lib=lib, device=Cm.device_of(lib))
    net.init_xavier(seed)
    randomise(net, seed + 1)
    return fe, net


def kws_graph(lib, arch, win=640, hop=320, mfccs=10, classes=12, seed=0):
    from tcresnet_amd.audio_nets import kws
    fe = Cm.make_frontend(lib, win, hop, num_mfccs=mfccs)
    g = T.Graph2D("", fe.n_frames, fe.n_coef, 1, lib=lib, device=Cm.device_of(lib))
    settings = {"spectrogram_length": fe.n_frames, "fingerprint_width": fe.n_coef, "fingerprint_size": fe.n_frames * fe.n_coef,
                "label_count": classes, "sample_rate": 16000, "window_stride_samples": hop}
    g.finalize(kws.build_model(g, settings, arch))
    randomise(g, seed + 1)
    return fe, g


def res_graph(lib, variant, win, hop, mfccs=40, seed=0):
    from tcresnet_amd.audio_nets import res
    fe = Cm.make_frontend(lib, win, hop, num_mfccs=mfccs)
    g = T.Graph2D("Res", fe.n_frames, fe.n_coef, 1, lib=lib, device=Cm.device_of(lib))
    layers, channels, pool, dil = res._VARIANTS[variant]
    g.finalize(res.build_resnet(g, 12, layers, channels, pool, dil))
    randomise(g, seed + 1)
    return fe, g


MODELS = {"dscnn_s": lambda lib: dscnn(lib), "tiny_conv": lambda lib: kws_graph(lib, "tiny_conv"),
          "single_fc": lambda lib: kws_graph(lib, "single_fc")}


def streaming():
    from tcresnet_amd import streaming as St
    return St


def scanner(net, fe, k, **kw):
    from tcresnet_amd import scanning as Sc
    return Sc.KeywordScanner(net, fe, frames_per_step=k, **kw)


def run_pushes(lib, fe, net, S, k, steps, resets, seed=0, **det_kw):
    """Every push: window bitwise the offline front-end of the stream's last clip, logits / probs bitwise forward_infer of those
    windows at batch S, the detector bitwise the NumPy restatement."""
    St = streaming()
    det = St.StreamingDetector(net, fe, S, frames_per_step=k, **det_kw)
    ref = RefDetector(S, det.average_steps, det_kw.get("min_count", 3), det.suppression_steps, det_kw.get("detection_threshold", 0.5))
    clips = Clips(lib, S, fe.n_samples)
    rng = np.random.RandomState(seed)
    for i in range(steps):
        x = Cm.to_dev(lib, rng.uniform(-1, 1, (S, k * fe.cfg.hop)) * rng.uniform(0.01, 0.6, (S, 1)))
        idx = resets.get(i, ())
        if idx:
            det.reset(idx)
        out = det.push(x)
        feat = fe(clips.step(x, idx))
        assert torch.equal(det.window(), feat)
        lo, pr = net.forward_infer(feat)
        assert torch.equal(out.logits, lo) and torch.equal(out.probs, pr)
        compare_detector(out, ref.step(out.probs.cpu().numpy(), idx))
    return det, clips


# ---- emulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["dscnn_s", "tiny_conv"])
def test_push_bitwise_forward_infer_and_rule(emu_lib, model):
    fe, net = MODELS[model](emu_lib)
    det, clips = run_pushes(emu_lib, fe, net, 3, 2, 6, {3: [1]}, average_window_ms=120, min_count=2, suppression_ms=40,
                            detection_threshold=0.0)
    # no fold: an in-place weight update is seen by the next push
    with torch.no_grad():
        net.params.mul_(1.03)
    x = Cm.to_dev(emu_lib, np.random.RandomState(9).uniform(-0.5, 0.5, (3, 2 * fe.cfg.hop)))
    out = det.push(x)
    assert torch.equal(out.logits, net.forward_infer(fe(clips.step(x)))[0])


@pytest.mark.parametrize("model", ["dscnn_s", "tiny_conv", "single_fc"])
def test_scan_and_push_many_equal_pushes(emu_lib, model):
    """scan == the pushes of a fresh detector (all six outputs); push_many in two calls (a reset in front of the second) == the
    pushes, and leaves the pushes' state.  max_windows = 5 with 13 steps: several chunks of three-step groups, a one-step last
    group, and streams whose window is carried across chunks."""
    St = streaming()
    fe, net = MODELS[model](emu_lib)
    S, k, steps = 2, 1, 13
    step = k * fe.cfg.hop
    audio = segment_audio(S, steps * step, 3)
    x = Cm.to_dev(emu_lib, audio)
    want = pushed(St.StreamingDetector(net, fe, S, frames_per_step=k, **DET), x)
    assert_bitwise(scanner(net, fe, k, max_windows=5, **DET).scan(x), want)
    assert_bitwise(scanner(net, fe, k, **DET).scan(x), want)
    a = St.StreamingDetector(net, fe, S, frames_per_step=k, max_windows=5, **DET)
    b = St.StreamingDetector(net, fe, S, frames_per_step=k, **DET)
    cut = 6 * step
    o1 = a.push_many(x[:, :cut].contiguous())
    a.reset([1])
    o2 = a.push_many(x[:, cut:].contiguous())
    p1 = pushed(b, x[:, :cut].contiguous())
    b.reset([1])
    p2 = pushed(b, x[:, cut:].contiguous())
    assert_bitwise(o1, p1)
    assert_bitwise(o2, p2)
    assert torch.equal(a.window(), b.window())
    tail = Cm.to_dev(emu_lib, audio[:, :step] * 0.5)
    for ta, tb in zip([t.clone() for t in a.push(tail)], b.push(tail)):
        assert torch.equal(ta, tb)


def test_sweep_on_dscnn_scan(emu_lib):
    fe, net = dscnn(emu_lib)
    audio = Cm.to_dev(emu_lib, segment_audio(2, 12 * fe.cfg.hop, 5))
    sc = scanner(net, fe, 1, **DET)
    out = sc.scan(audio)
    thr = [0.0, 0.2, 0.5]
    res = sc.sweep(out, thr, return_fired=True)
    for t, th in enumerate(thr):
        one = scanner(net, fe, 1, **dict(DET, detection_threshold=th)).scan(audio)
        assert torch.equal(res.fired[t].to(torch.int32), one.is_new)


def test_prepared_and_weight_rules(emu_lib):
    St = streaming()
    fe, net = dscnn(emu_lib)
    S = 2
    a, b = St.StreamingDetector(net, fe, S, min_count=1), St.StreamingDetector(net, fe, S, min_count=1)
    buf = torch.zeros((S, fe.cfg.hop))
    call = b.prepared(buf)
    rng = np.random.RandomState(2)
    for i in range(3):
        x = Cm.to_dev(emu_lib, rng.uniform(-0.5, 0.5, (S, fe.cfg.hop)))
        if i == 1:
            a.reset([0])
            b.reset([0])
        oa = [t.clone() for t in a.push(x)]
        buf.copy_(x)
        for ta, tb in zip(oa, call()):
            assert torch.equal(ta, tb)
    net.params = net.params.clone()
    with pytest.raises(T.TcrError, match="rebound"):
        call()
    b.prepared(buf)()
    with pytest.raises(T.TcrError, match="frozen_ss"):
        St.StreamingDetector(net, fe, S, frozen_ss=torch.zeros(8))
    with pytest.raises(T.TcrError, match="frozen_ss"):
        scanner(net, fe, 1, frozen_ss=torch.zeros(8))
    g = T.Graph2D("", fe.n_frames, fe.n_coef, 1, lib=emu_lib, device="cpu")
    with pytest.raises(T.TcrError, match="not finalized"):
        St.StreamingDetector(g, fe, S)


def test_m_entries_with_tcresnet_ref_equal_the_old_entries(emu_lib):
    lib = emu_lib
    fe, net, _, _, _ = setup(lib)
    ss = net.fold_bn()
    ref = T._lib.ModelRef(0, net._h.value, net.params.data_ptr(), ss.data_ptr())
    cfg, det = C.byref(fe.cfg), T._lib.DetectCfg(3, 2, 1, 0.0)
    S, k = 2, 2
    nstate = lib.tcr_stream_state_bytes(cfg, net._h, S, k, C.byref(det))
    nws = lib.tcr_stream_workspace_bytes(cfg, net._h, S, k)
    assert nstate > 0 and nstate == lib.tcr_stream_state_bytes_m(cfg, C.byref(ref), S, k, C.byref(det))
    assert nws > 0 and nws == lib.tcr_stream_workspace_bytes_m(cfg, C.byref(ref), S, k)
    nscan = lib.tcr_scan_workspace_bytes(cfg, net._h, k, 8)
    assert nscan > 0 and nscan == lib.tcr_scan_workspace_bytes_m(cfg, C.byref(ref), k, 8)
    states = [torch.zeros(nstate // 4), torch.zeros(nstate // 4)]
    wss = [torch.zeros(nws // 4), torch.zeros(nws // 4)]
    lib.check(lib.tcr_stream_init(cfg, fe.plan.data_ptr(), net._h, S, k, C.byref(det), states[0].data_ptr(), wss[0].data_ptr(), nws, None))
    lib.check(lib.tcr_stream_init_m(cfg, fe.plan.data_ptr(), C.byref(ref), S, k, C.byref(det), states[1].data_ptr(), wss[1].data_ptr(), nws,
                                    None))
    assert torch.equal(states[0].view(torch.int32), states[1].view(torch.int32))     # (bytes: the detector integers)
    rng = np.random.RandomState(4)
    reset = torch.tensor([0, 1], dtype=torch.uint8)

    def outs(m):
        return [torch.full((S, m, 12), -1.0), torch.full((S, m, 12), -1.0), torch.full((S, m, 12), -1.0),
                torch.full((S, m), -7, dtype=torch.int32), torch.full((S, m), -1.0), torch.full((S, m), -7, dtype=torch.int32)]
    for i in range(3):
        x = Cm.to_dev(lib, rng.uniform(-0.5, 0.5, (S, k * fe.cfg.hop)))
        rp = reset.data_ptr() if i == 2 else None
        o = [outs(1), outs(1)]
        lib.check(lib.tcr_stream_step(cfg, fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), S, k, C.byref(det), x.data_ptr(),
                                      rp, states[0].data_ptr(), wss[0].data_ptr(), nws, *(t.data_ptr() for t in o[0]), None))
        lib.check(lib.tcr_stream_step_m(cfg, fe.plan.data_ptr(), C.byref(ref), S, k, C.byref(det), x.data_ptr(), rp, states[1].data_ptr(),
                                        wss[1].data_ptr(), nws, *(t.data_ptr() for t in o[1]), None))
        for a, b in zip(*o):
            assert torch.equal(a, b)
        assert torch.equal(states[0].view(torch.int32), states[1].view(torch.int32))     # (bytes: the detector integers)
    m = 3
    x = Cm.to_dev(lib, rng.uniform(-0.5, 0.5, (S, m * k * fe.cfg.hop)))
    sws = torch.zeros(nscan // 4)
    o = [outs(m), outs(m)]
    lib.check(lib.tcr_stream_scan(cfg, fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), S, x.shape[1], k, C.byref(det),
                                  x.data_ptr(), reset.data_ptr(), states[0].data_ptr(), sws.data_ptr(), nscan, *(t.data_ptr() for t in o[0]),
                                  None))
    lib.check(lib.tcr_stream_scan_m(cfg, fe.plan.data_ptr(), C.byref(ref), S, x.shape[1], k, C.byref(det), x.data_ptr(), reset.data_ptr(),
                                    states[1].data_ptr(), sws.data_ptr(), nscan, *(t.data_ptr() for t in o[1]), None))
    for a, b in zip(*o):
        assert torch.equal(a, b)
    assert torch.equal(states[0].view(torch.int32), states[1].view(torch.int32))     # (bytes: the detector integers)
    o = [outs(m), outs(m)]
    lib.check(lib.tcr_scan(cfg, fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), S, x.shape[1], k, C.byref(det), x.data_ptr(),
                           sws.data_ptr(), nscan, *(t.data_ptr() for t in o[0]), None))
    lib.check(lib.tcr_scan_m(cfg, fe.plan.data_ptr(), C.byref(ref), S, x.shape[1], k, C.byref(det), x.data_ptr(), sws.data_ptr(), nscan,
                             *(t.data_ptr() for t in o[1]), None))
    for a, b in zip(*o):
        assert torch.equal(a, b)
    # the wrappers keep their own names in the messages
    assert lib.tcr_stream_state_bytes(cfg, net._h, 0, k, C.byref(det)) == 0
    assert lib.tcr_last_error() == b"tcr_stream_state_bytes: the number of streams must be positive (got 0)"
    assert lib.tcr_stream_state_bytes_m(cfg, C.byref(ref), 0, k, C.byref(det)) == 0
    assert lib.tcr_last_error() == b"tcr_stream_state_bytes_m: the number of streams must be positive (got 0)"


def test_m_entries_refuse(emu_lib):
    lib = emu_lib
    fe, net = dscnn(lib)
    cfg, det = C.byref(fe.cfg), C.byref(T._lib.DetectCfg(3, 2, 1, 0.5))
    ref = T._lib.ModelRef(1, net._h.value, net.params.data_ptr(), net.stats.data_ptr())
    assert lib.tcr_stream_state_bytes_m(cfg, C.byref(ref), 2, 1, det) > 0
    assert lib.tcr_scan_workspace_bytes_m(cfg, C.byref(ref), 1, 4096 * 255) > 0
    assert lib.tcr_scan_workspace_bytes_m(cfg, C.byref(ref), 1, 65535 * 16 + 1024) == 0
    assert b"too large" in lib.tcr_last_error()
    assert lib.tcr_stream_workspace_bytes_m(cfg, C.byref(ref), 65535 * 16 + 1, 1) == 0
    assert b"windows one call" in lib.tcr_last_error()
    bad = T._lib.ModelRef(7, net._h.value, net.params.data_ptr(), net.stats.data_ptr())
    assert lib.tcr_stream_state_bytes_m(cfg, C.byref(bad), 2, 1, det) == 0
    assert lib.tcr_last_error() == (b"tcr_stream_state_bytes_m: unknown model family 7 (TCR_FAMILY_TCRESNET, TCR_FAMILY_DSCNN or "
                                    b"TCR_FAMILY_G2D)")
    null = T._lib.ModelRef(1, None, net.params.data_ptr(), net.stats.data_ptr())
    assert lib.tcr_scan_workspace_bytes_m(cfg, C.byref(null), 1, 16) == 0
    assert b"null front-end configuration or network" in lib.tcr_last_error()
    fe40 = Cm.make_frontend(lib, 640, 320)
    assert lib.tcr_stream_workspace_bytes_m(C.byref(fe40.cfg), C.byref(ref), 2, 1) == 0
    assert lib.tcr_last_error() == b"tcr_stream_workspace_bytes_m: the front-end yields 40 x 49 features, the network expects 10 x 49"
    g = T.Graph2D("", fe.n_frames, fe.n_coef, 1, lib=lib, device="cpu")
    unfinished = T._lib.ModelRef(2, g._h.value, net.params.data_ptr(), net.stats.data_ptr())
    assert lib.tcr_stream_state_bytes_m(cfg, C.byref(unfinished), 2, 1, det) == 0
    assert b"not finalized" in lib.tcr_last_error()
    _, wide = kws_graph(lib, "single_fc", classes=300)
    wref = T._lib.ModelRef(2, wide._h.value, wide.params.data_ptr(), wide.stats.data_ptr())
    assert lib.tcr_stream_state_bytes_m(cfg, C.byref(wref), 2, 1, det) == 0
    assert b"at most 256 classes (got 300)" in lib.tcr_last_error()
    # a null arena in a step / scan
    noaux = T._lib.ModelRef(1, net._h.value, net.params.data_ptr(), None)
    p = torch.zeros(64)
    assert lib.tcr_scan_m(cfg, fe.plan.data_ptr(), C.byref(noaux), 1, 320, 1, det, p.data_ptr(), p.data_ptr(), 256,
                          *([p.data_ptr()] * 6), None) == -1
    assert lib.tcr_last_error() == b"tcr_scan_m: null argument"


def test_frozen_model_refusals_name_the_families():
    from tcresnet_amd import deploy
    import types
    for fam in ("dscnn", "graph2d"):
        for fn in (deploy.FrozenModel.streaming, lambda m, *a: deploy.FrozenModel.scanner(m)):
            with pytest.raises(ValueError, match="TC-ResNet, DS-CNN and 2-D graph artifacts exported with include_preprocess"):
                fn(types.SimpleNamespace(meta={"family": fam}, frontend=None), 2)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
def frontend_meta(fe):
    return {"sample_rate": 16000, "clip_duration_ms": 1000, "window_size_samples": int(fe.cfg.win), "window_stride_samples": int(fe.cfg.hop),
            "num_mel_bins": 64, "num_mfccs": int(fe.cfg.n_coef), "lower_edge_hertz": 80.0, "upper_edge_hertz": 7600.0, "method": "mfcc"}


def frozen_dscnn(net, fe, size, path):
    from tcresnet_amd import deploy
    meta = {"format": deploy.FORMAT, "model": f"DSCNN{size}Model", "family": "dscnn", "size": size, "num_classes": 12,
            "include_preprocess": True, "height": fe.n_frames, "width": fe.n_coef, "channels": 1,
            "inputs": [{"name": "input/audio/before_preprocessing", "shape": [1, fe.n_samples, 1]}],
            "output": {"name": "output/softmax", "shape": [1, 12]}, "frontend": frontend_meta(fe)}
    return deploy.FrozenModel(meta, net.state_dict(), lib=net.lib, device=net.device).save(path)


def frozen_kws(net, fe, arch, path):
    from tcresnet_amd import deploy
    meta = {"format": deploy.FORMAT, "model": "KWSModel", "family": "graph2d", "num_classes": 12, "include_preprocess": True,
            "height": fe.n_frames, "width": fe.n_coef, "channels": 1,
            "args": {"num_classes": 12, "sample_rate": 16000, "window_stride_ms": fe.cfg.hop / 16.0, "architecture": arch},
            "inputs": [{"name": "input/audio/before_preprocessing", "shape": [1, fe.n_samples, 1]}],
            "output": {"name": "output/softmax", "shape": [1, 12]}, "frontend": frontend_meta(fe)}
    return deploy.FrozenModel(meta, net.state_dict(), lib=net.lib, device=net.device).save(path)


@pytest.mark.gpu
def test_gpu_forward_infer_rows_do_not_depend_on_the_batch(hip_lib):
    """What the scan / push parity rests on: DS-CNN-L and 2-D graphs give bitwise rows at batches 1, 7, 70 and 4096."""
    nets = [dscnn(hip_lib, "L"), res_graph(hip_lib, "Res8", 480, 160), kws_graph(hip_lib, "low_latency_svdf", mfccs=40)]
    g = torch.Generator(device="cuda").manual_seed(0)
    for fe, net in nets:
        wav = ((torch.rand((4096, fe.n_samples), device="cuda", generator=g) * 2 - 1) * 0.5).contiguous()
        feat = fe(wav)
        lo, pr = net.forward_infer(feat)
        lo, pr = lo.clone(), pr.clone()
        for b in (1, 7, 70):
            for start in (0, 4096 - b):
                l2, p2 = net.forward_infer(feat[start:start + b].contiguous())
                assert torch.equal(l2, lo[start:start + b]) and torch.equal(p2, pr[start:start + b]), (type(net).__name__, b, start)


@pytest.mark.gpu
def test_gpu_dscnn_l_4096_streams_random_resets(hip_lib):
    St = streaming()
    fe, net = dscnn(hip_lib, "L")
    S, steps = 4096, 40
    det = St.StreamingDetector(net, fe, S)
    clips = Clips(hip_lib, S, fe.n_samples)
    g = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.RandomState(3)
    for i in range(steps):
        x = (torch.rand((S, fe.cfg.hop), device="cuda", generator=g) * 2 - 1) * 0.5
        idx = np.nonzero(rng.uniform(size=S) < 0.01)[0] if i % 7 == 3 else ()
        if len(idx):
            det.reset(idx)
        out = det.push(x)
        clip = clips.step(x, idx)
        if (i + 1) % 10 == 0:
            feat = fe(clip)
            assert torch.equal(det.window(), feat)
            lo, pr = net.forward_infer(feat)
            assert torch.equal(out.logits, lo) and torch.equal(out.probs, pr)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["res8_3010", "low_latency_svdf_4020"])
def test_gpu_graph2d_scan_and_push_many_equal_pushes(hip_lib, model):
    St = streaming()
    fe, net = res_graph(hip_lib, "Res8", 480, 160) if model == "res8_3010" else kws_graph(hip_lib, "low_latency_svdf", mfccs=40)
    S, k, steps = 8, 2, 60
    step = k * fe.cfg.hop
    x = Cm.to_dev(hip_lib, segment_audio(S, steps * step, 13))
    want = pushed(St.StreamingDetector(net, fe, S, frames_per_step=k, **DET), x)
    assert_bitwise(scanner(net, fe, k, **DET).scan(x), want)
    assert_bitwise(scanner(net, fe, k, max_windows=7, **DET).scan(x), want)
    a = St.StreamingDetector(net, fe, S, frames_per_step=k, max_windows=32, **DET)
    cut = 23 * step
    o1, o2 = a.push_many(x[:, :cut].contiguous()), a.push_many(x[:, cut:].contiguous())
    for f, w in zip(o1, want):
        assert torch.equal(f, w[:, :23])
    for f, w in zip(o2, want):
        assert torch.equal(f, w[:, 23:])


@pytest.mark.gpu
def test_gpu_dscnn_l_scan_does_not_depend_on_the_chunking(hip_lib):
    fe, net = dscnn(hip_lib, "L")
    x = Cm.to_dev(hip_lib, segment_audio(8, 3 * 60 * 16000, 17))
    a = scanner(net, fe, 1, **DET).scan(x)
    b = scanner(net, fe, 1, max_windows=4096 * 8, **DET).scan(x)
    assert_bitwise(a, b)
    pick = [0, 4500, 8999]
    feat = fe(torch.stack([torch.cat([torch.zeros(fe.n_samples, device="cuda"), x[3]])[(i + 1) * 320:(i + 1) * 320 + fe.n_samples]
                           for i in pick]).contiguous())
    assert torch.equal(a.logits[3, pick], net.forward_infer(feat)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["dscnn", "graph2d"])
def test_gpu_frozen_model_round_trips(hip_lib, tmp_path, family):
    St = streaming()
    from tcresnet_amd import deploy
    if family == "dscnn":
        fe, net = dscnn(hip_lib, "S")
        path = frozen_dscnn(net, fe, "S", str(tmp_path / "m.npz"))
    else:
        fe, net = kws_graph(hip_lib, "low_latency_conv", mfccs=40)
        path = frozen_kws(net, fe, "low_latency_conv", str(tmp_path / "m.npz"))
    model = deploy.FrozenModel.load(path, lib=hip_lib, device="cuda")
    assert model.meta["family"] == family and model.frontend.cfg.n_coef == fe.cfg.n_coef
    S, k = 4, 2
    x = Cm.to_dev(hip_lib, segment_audio(S, 40 * k * fe.cfg.hop, 19))
    fe_m = model.frontend
    want = pushed(St.StreamingDetector(net, fe_m, S, frames_per_step=k, **DET), x)
    assert_bitwise(pushed(model.streaming(S, frames_per_step=k, **DET), x), want)
    sc = model.scanner(frames_per_step=k, **DET)
    out = sc.scan(x)
    assert_bitwise(out, want)
    thr = [0.0, 0.3, 0.6, 0.9]
    res = sc.sweep(out, thr, return_fired=True)
    direct = scanner(net, fe_m, k, **DET).sweep(out, thr, return_fired=True)
    for a, b in zip(res[:4], direct[:4]):
        assert torch.equal(a, b)
    for t, th in enumerate(thr):
        one = model.scanner(frames_per_step=k, **dict(DET, detection_threshold=th)).scan(x)
        assert torch.equal(res.fired[t].to(torch.int32), one.is_new)


@pytest.mark.gpu
def test_gpu_scan_audio_cli_dscnn_chunked(hip_lib, tmp_path):
    fe, net = dscnn(hip_lib, "S")
    path = frozen_dscnn(net, fe, "S", str(tmp_path / "ds.npz"))
    audio = segment_audio(2, 20 * 16000, 29)
    pcm = [np.clip(audio[0] * 32767, -32768, 32767).astype(np.int16), np.clip(audio[1, :251234] * 32767, -32768, 32767).astype(np.int16)]
    wavs = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for w, a in zip(wavs, pcm):
        write_wav(w, a)
    args = ["--frozen", path, "--wav", *wavs, "--frames_per_step", "2", "--average_window_ms", "200", "--min_count", "2",
            "--detection_threshold", "0.0", "--suppression_ms", "400"]
    run = lambda *extra: subprocess.run([sys.executable, os.path.join(ROOT, "tc-resnet_amd", "scan_audio.py"), *args, *extra],
                                        capture_output=True, text=True, timeout=600)
    whole, chunked = run(), run("--chunk_seconds", "3.3")
    assert whole.returncode == 0, whole.stderr
    assert chunked.returncode == 0, chunked.stderr
    assert whole.stdout == chunked.stdout
    assert len(whole.stdout.strip().splitlines()) >= 2
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text(f"file,start_ms,end_ms,label\n{wavs[0]},2000,2600,3\n{wavs[1]},5000,5400,7\n")
    sw = subprocess.run([sys.executable, os.path.join(ROOT, "tc-resnet_amd", "sweep_audio.py"), "--frozen", path, "--wav", *wavs,
                         "--events", str(ev_csv), "--thresholds", "0:0.9:0.1", "--frames_per_step", "2", "--average_window_ms", "200",
                         "--min_count", "2", "--suppression_ms", "400"], capture_output=True, text=True, timeout=600)
    assert sw.returncode == 0, sw.stderr
    assert len(sw.stdout.strip().splitlines()) >= 10


@pytest.mark.gpu
def test_gpu_dscnn_prepared_is_push_and_refuses_rebound_params(hip_lib):
    St = streaming()
    fe, net = dscnn(hip_lib, "L")
    S = 64
    a, b = St.StreamingDetector(net, fe, S, min_count=1), St.StreamingDetector(net, fe, S, min_count=1)
    buf = torch.zeros((S, fe.cfg.hop), device="cuda")
    call = b.prepared(buf)
    g = torch.Generator(device="cuda").manual_seed(4)
    for i in range(10):
        x = (torch.rand((S, fe.cfg.hop), device="cuda", generator=g) * 2 - 1) * 0.5
        if i == 5:
            a.reset([2, 7])
            b.reset([2, 7])
        if i == 7:
            with torch.no_grad():
                net.params.mul_(1.01)              # in place: both see it at their next step
        oa = [t.clone() for t in a.push(x)]
        buf.copy_(x)
        for ta, tb in zip(oa, call()):
            assert torch.equal(ta, tb)
    net.params = net.params.clone()
    with pytest.raises(T.TcrError, match="rebound"):
        call()
    ob = b.prepared(buf)()
    assert torch.equal(ob.logits, net.forward_infer(b.window().clone())[0])
