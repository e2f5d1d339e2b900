"""Offline keyword scanning (tcr_scan, tcresnet_amd.scanning): every step of a scan is bitwise what a fresh streaming detector returns
push by push, in all six outputs, whatever the chunking.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_streaming import frozen_artifact, segment_audio, setup, write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("logits", "probs", "smoothed", "top", "score", "is_new")


def scanning():
    from tcresnet_amd import scanning as Sc
    return Sc


def pushed(det, audio, prepared=False):
    """The streaming detector fed audio [S, L] (on the device) k * hop samples at a time: its outputs stacked [S, steps, ...]."""
    step = det.step_samples
    steps = audio.shape[1] // step
    outs = None
    buf = torch.zeros((audio.shape[0], step), dtype=torch.float32, device=audio.device)
    call = det.prepared(buf) if prepared else None
    for i in range(steps):
        x = audio[:, i * step:(i + 1) * step].contiguous()
        if call is not None:
            buf.copy_(x)
            o = call()
        else:
            o = det.push(x)
        if outs is None:
            outs = [torch.empty((steps,) + tuple(t.shape), dtype=t.dtype, device=t.device) for t in o]
        for dst, t in zip(outs, o):
            dst[i].copy_(t)
    return [t.transpose(0, 1).contiguous() for t in outs]


def assert_bitwise(got, want):
    for name, g, w in zip(FIELDS, got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert torch.equal(g, w), (name, int((g != w).sum()))


DET = dict(average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=200)


def check_scan_equals_stream(lib, fe, net, audio, k, det=DET, **scan_kw):
    from tcresnet_amd import streaming as St
    Sc = scanning()
    x = Cm.to_dev(lib, audio)
    want = pushed(St.StreamingDetector(net, fe, audio.shape[0], frames_per_step=k, **det), x)
    got = Sc.KeywordScanner(net, fe, frames_per_step=k, **det, **scan_kw).scan(x)
    assert_bitwise(got, want)
    return got


# ---- emulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_scan_4020_equals_streaming(emu_lib, k):
    fe, net, _, _, _ = setup(emu_lib)
    L = 20160                                             # 1.26 s: 63 steps at k = 1, 21 at k = 3
    got = check_scan_equals_stream(emu_lib, fe, net, segment_audio(2, L, 3), k)
    assert got.is_new.shape == (2, L // (k * fe.cfg.hop))
    assert int(got.is_new.sum()) >= 1
    assert int((got.top == -1).sum()) == 2                # one step below min_count = 2 per signal


def test_scan_3010_log_mel_equals_streaming(emu_lib):
    fe, net, _, _, _ = setup(emu_lib, win=480, hop=160, method="log_mel_spectrogram")
    assert fe.n_frames == 98 and fe.n_coef == 64
    got = check_scan_equals_stream(emu_lib, fe, net, segment_audio(2, 16000, 5), 2)
    assert int(got.is_new.sum()) >= 1


def test_scan_chunking_invariance(emu_lib):
    """max_windows = 1 (a network launch per window, at batch 1), 7 and the default give the same bits."""
    Sc = scanning()
    fe, net, _, _, _ = setup(emu_lib)
    x = Cm.to_dev(emu_lib, segment_audio(2, 7680, 9))     # 24 steps per signal
    outs = [Sc.KeywordScanner(net, fe, max_windows=m, **DET).scan(x) for m in (1, 7, None)]
    for o in outs[1:]:
        assert_bitwise(o, outs[0])
    assert outs[2].logits.shape == (2, 24, 12)


def test_scan_argument_errors(emu_lib):
    Sc = scanning()
    fe, net, _, _, _ = setup(emu_lib)
    sc = Sc.KeywordScanner(net, fe, frames_per_step=2)
    with pytest.raises(T.TcrError, match="multiple of k \\* hop"):
        sc.scan(torch.zeros((2, 1000)))
    with pytest.raises(T.TcrError, match="\\[N, L\\]"):
        sc.scan(torch.zeros(640))
    with pytest.raises(T.TcrError, match="outside 1..T"):
        Sc.KeywordScanner(net, fe, frames_per_step=fe.n_frames + 1)
    with pytest.raises(T.TcrError, match="max_windows"):
        Sc.KeywordScanner(net, fe, max_windows=0)
    with pytest.raises(T.TcrError, match="min_count"):
        Sc.KeywordScanner(net, fe, average_window_ms=40, min_count=3).scan(torch.zeros((1, 640)))
    dep = Cm.make_frontend(emu_lib, 640, 320, method="mfcc_deploy")
    with pytest.raises(T.TcrError, match="deploy"):
        Sc.KeywordScanner(net, dep)
    fe98 = Cm.make_frontend(emu_lib, 480, 160)
    with pytest.raises(T.TcrError, match="network expects"):
        Sc.KeywordScanner(net, fe98)
    # the C entry points refuse on their own (size 0 / status + message)
    lib = emu_lib
    assert lib.tcr_scan_workspace_bytes(C.byref(dep.cfg), net._h, 1, 16) == 0 and b"deploy" in lib.tcr_last_error()
    assert lib.tcr_scan_workspace_bytes(C.byref(fe.cfg), net._h, 1, 0) == 0 and b"max_windows" in lib.tcr_last_error()
    det = T._lib.DetectCfg(4, 2, 0, 0.5)
    buf = torch.zeros(1 << 16)
    ss = net.fold_bn()
    p = buf.data_ptr()

    def call(n, L, ws_bytes, cfg=fe.cfg, d=det):
        return lib.tcr_scan(C.byref(cfg), fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), n, L, 1, C.byref(d), p, p,
                            ws_bytes, p, p, p, p, p, p, None)
    assert call(0, 640, 1 << 18) == -1 and b"number of signals must be positive" in lib.tcr_last_error()
    assert call(1, 650, 1 << 18) == -1 and b"multiple of k * hop" in lib.tcr_last_error()
    assert call(1, 640, 1024) == -3 and b"one window" in lib.tcr_last_error()
    assert call(1, 640, 1 << 18, cfg=dep.cfg) == -1 and b"deploy" in lib.tcr_last_error()
    assert call(1, 640, 1 << 18, d=T._lib.DetectCfg(0, 1, 0, 0.5)) == -1 and b"average_steps" in lib.tcr_last_error()


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_scan_64_signals_30s(hip_lib):
    fe, net, _, _, _ = setup(hip_lib)
    audio = segment_audio(64, 30 * 16000, 21)
    got = check_scan_equals_stream(hip_lib, fe, net, audio, 1, det=dict(average_window_ms=1000, min_count=3, detection_threshold=0.3,
                                                                        suppression_ms=1500))
    assert got.logits.shape == (64, 1500, 12)
    assert int(got.is_new.sum()) >= 1


@pytest.mark.gpu
def test_gpu_scan_tcresnet14_3010(hip_lib):
    fe, net, _, _, _ = setup(hip_lib, "TCResNet14", 1.5, win=480, hop=160)
    got = check_scan_equals_stream(hip_lib, fe, net, segment_audio(16, 10 * 16000, 22), 2)
    assert int(got.is_new.sum()) >= 1


@pytest.mark.gpu
def test_gpu_scan_10_minutes_prepared_and_chunking(hip_lib):
    from tcresnet_amd import streaming as St
    Sc = scanning()
    fe, net, _, _, _ = setup(hip_lib)
    det = dict(average_window_ms=1000, min_count=3, detection_threshold=0.3, suppression_ms=1500)
    x = Cm.to_dev(hip_lib, segment_audio(1, 600 * 16000, 23))
    want = pushed(St.StreamingDetector(net, fe, 1, **det), x, prepared=True)
    outs = [Sc.KeywordScanner(net, fe, max_windows=m, **det).scan(x) for m in (None, 7, 1)]
    assert outs[0].logits.shape == (1, 30000, 12)
    for o in outs:
        assert_bitwise(o, want)
    assert int(want[5].sum()) >= 1


@pytest.mark.gpu
def test_gpu_scan_audio_cli_equals_stream_audio(hip_lib, tmp_path):
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    audio = segment_audio(2, 96000, 24)
    pcm = [np.clip(audio[0] * 32767, -32768, 32767).astype(np.int16), np.clip(audio[1, :61234] * 32767, -32768, 32767).astype(np.int16)]
    wavs = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    args = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(f"c{i}" for i in range(12)), "--frames_per_step", "2",
            "--average_window_ms", "200", "--min_count", "2", "--detection_threshold", "0.3", "--suppression_ms", "400"]
    run = lambda script, *extra: subprocess.run([sys.executable, os.path.join(ROOT, "tc-resnet_amd", script), *args, *extra],
                                                capture_output=True, text=True, timeout=600)
    st, sc = run("stream_audio.py"), run("scan_audio.py", "--summary")
    assert st.returncode == 0, st.stderr
    assert sc.returncode == 0, sc.stderr
    assert sc.stdout == st.stdout
    assert len(st.stdout.strip().splitlines()) >= 2
    assert "dropping" in sc.stderr
    import json
    summary = json.loads(sc.stderr.strip().splitlines()[-1])
    assert summary["detections"] == len(st.stdout.strip().splitlines())
    assert abs(summary["hours"] - (96000 + 61234 // 640 * 640) / 16000 / 3600) < 1e-12
