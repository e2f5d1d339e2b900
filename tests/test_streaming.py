"""Streaming detection (tcr_stream_*, tcresnet_amd.streaming): the window kept on the device is bitwise the offline front-end of
each stream's last clip, the logits / probs are bitwise the frozen forward of those windows, and the detector follows its rule
(a NumPy float32 restatement below).  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import ctypes as C
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from tests import common as Cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def streaming():
    from tcresnet_amd import streaming as St
    return St


def setup(lib, name="TCResNet8", width=1.0, win=640, hop=320, method="mfcc", seed=0):
    fe = Cm.make_frontend(lib, win, hop, method=method)
    arch = R.make_tcresnet(name, width, in_channels=fe.n_coef)
    p, s = R.init_params(arch, seed)
    R.randomize_bn(arch, p, s, seed + 1)
    net = Cm.make_net(lib, name, width, fe.n_frames, p, s, in_channels=fe.n_coef)
    return fe, net, arch, p, s


class Clips:
    """Each stream's last n_samples samples of  zeros(n_samples) ++ everything pushed since its reset (on the device)."""

    def __init__(self, lib, n_streams, n_samples):
        self.clip = torch.zeros((n_streams, n_samples), dtype=torch.float32, device=Cm.device_of(lib))

    def step(self, x, reset_idx=()):
        for i in reset_idx:
            self.clip[i] = 0.0
        self.clip = torch.cat([self.clip, x], dim=1)[:, -self.clip.shape[1]:].contiguous()     # (a step may be longer than a clip)
        return self.clip


def segment_audio(n_streams, n_samples, seed):
    """Quiet (0.01) and loud (0.5) noise in alternating segments of 0.8 - 1.6 s, a different cut per stream: the random nets' top
    class moves between two labels with them."""
    rng = np.random.RandomState(seed)
    out = np.zeros((n_streams, n_samples), np.float32)
    for s in range(n_streams):
        pos, loud = 0, s % 2
        while pos < n_samples:
            m = min(int(rng.randint(12800, 25600)), n_samples - pos)
            out[s, pos:pos + m] = rng.uniform(-1, 1, m) * (0.5 if loud else 0.01)
            pos, loud = pos + m, 1 - loud
    return out


def check_step(fe, net, ss, det, clip, out):
    """Window bitwise the offline front-end, logits / probs bitwise forward_frozen of it at batch S."""
    ref = fe(clip)
    assert torch.equal(det.window(), ref), float((det.window() - ref).abs().max())
    lo, pr = net.forward_frozen(ref, ss)
    assert torch.equal(out.logits, lo) and torch.equal(out.probs, pr)
    return ref


def run_checked(lib, fe, net, arch, p, s, n_streams, k, steps, resets, seed=0):
    St = streaming()
    det = St.StreamingDetector(net, fe, n_streams, frames_per_step=k, min_count=1)
    ss = net.fold_bn()
    clips = Clips(lib, n_streams, fe.n_samples)
    rng = np.random.RandomState(seed)
    for i in range(steps):
        x = Cm.to_dev(lib, rng.uniform(-1, 1, (n_streams, k * fe.cfg.hop)) * rng.uniform(0.01, 0.6, (n_streams, 1)))
        idx = resets.get(i, ())
        if idx:
            det.reset(idx)
        out = det.push(x)
        ref = check_step(fe, net, ss, det, clips.step(x, idx), out)
    want = R.forward(arch, p, s, fe.reference_view(ref)[..., 0].cpu().numpy().astype(np.float64), False)["logits"]
    err = np.abs(out.logits.cpu().numpy() - want).max()
    assert err < Cm.LOGIT_TOL, err
    return det


# ---- the detector rule, restated ------------------------------------------------------------------------------------------------
class RefDetector:
    def __init__(self, n_streams, W, min_count, suppression, threshold):
        self.W, self.min_count, self.supp, self.thr = W, min_count, suppression, np.float32(threshold)
        self.ring = [[] for _ in range(n_streams)]
        self.prev = [-1] * n_streams
        self.prev_step = [0] * n_streams
        self.n = [0] * n_streams
        self.branches = set()

    def step(self, probs, reset=()):
        S, Cn = probs.shape
        smoothed = np.zeros((S, Cn), np.float32)
        top = np.full(S, -1, np.int32)
        score = np.zeros(S, np.float32)
        is_new = np.zeros(S, np.int32)
        for s in range(S):
            if s in reset:
                self.ring[s], self.prev[s], self.prev_step[s], self.n[s] = [], -1, 0, 0
            self.ring[s] = (self.ring[s] + [probs[s].astype(np.float32)])[-self.W:]
            count = len(self.ring[s])
            acc = np.zeros(Cn, np.float32)
            for v in self.ring[s]:
                acc = acc + v
            smoothed[s] = acc * (np.float32(1.0) / np.float32(count))
            if count < self.min_count:
                self.branches.add("warming up")
            else:
                top[s] = int(np.argmax(smoothed[s]))
                score[s] = smoothed[s, top[s]]
                if not score[s] > self.thr:
                    self.branches.add("below threshold")
                elif top[s] == self.prev[s]:
                    self.branches.add("same label")
                elif self.prev[s] != -1 and self.n[s] - self.prev_step[s] <= self.supp:
                    self.branches.add("suppressed")
                else:
                    self.branches.add("first" if self.prev[s] == -1 else "new label")
                    is_new[s] = 1
                    self.prev[s], self.prev_step[s] = int(top[s]), self.n[s]
            self.n[s] += 1
        return smoothed, top, score, is_new


def compare_detector(out, ref):
    smoothed, top, score, is_new = ref
    assert np.array_equal(out.smoothed.cpu().numpy(), smoothed)
    assert np.array_equal(out.top.cpu().numpy(), top)
    assert np.array_equal(out.score.cpu().numpy(), score)
    assert np.array_equal(out.is_new.cpu().numpy(), is_new)


# ---- emulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_stream_4020_bitwise_offline(emu_lib, k):
    fe, net, arch, p, s = setup(emu_lib)
    run_checked(emu_lib, fe, net, arch, p, s, 3, k, 8, {4: [1]})


def test_stream_3010_and_log_mel(emu_lib):
    fe, net, arch, p, s = setup(emu_lib, win=480, hop=160)
    assert fe.n_frames == 98
    run_checked(emu_lib, fe, net, arch, p, s, 2, 2, 4, {2: [0]})
    fe, net, arch, p, s = setup(emu_lib, method="log_mel_spectrogram")
    assert fe.n_coef == 64
    run_checked(emu_lib, fe, net, arch, p, s, 2, 1, 4, {1: [1]}, seed=1)


def test_stream_k_equals_T(emu_lib):
    """k = T: every column is new each step (the left halo is the front-end's to write)."""
    fe, net, arch, p, s = setup(emu_lib)
    run_checked(emu_lib, fe, net, arch, p, s, 2, fe.n_frames, 2, {1: [0]})


def test_stream_detector_rule(emu_lib):
    """Device detector == the NumPy restatement on the probs the device produced, bitwise; every branch of the rule is taken."""
    St = streaming()
    fe, net, _, _, _ = setup(emu_lib)
    S, k, steps = 3, 3, 80
    step = k * fe.cfg.hop
    audio = segment_audio(S, steps * step, 7)
    resets = {30: [1], 50: [2, 0]}
    branches = set()
    # pass 1: threshold 0, collect the probs; pass 2: the threshold at the median smoothed score of pass 1
    params = [dict(average_window_ms=120, min_count=2, suppression_ms=180, detection_threshold=0.0)]
    probs_seen = []
    for pi in range(2):
        if pi == 1:
            sc = np.concatenate(probs_seen)
            params.append(dict(average_window_ms=60, min_count=1, suppression_ms=120, detection_threshold=float(np.median(sc))))
        det = St.StreamingDetector(net, fe, S, frames_per_step=k, **params[pi])
        assert det.step_ms == 60.0
        ref = RefDetector(S, det.average_steps, params[pi]["min_count"], det.suppression_steps, params[pi]["detection_threshold"])
        for i in range(steps):
            if i in resets:
                det.reset(resets[i])
            out = det.push(Cm.to_dev(emu_lib, audio[:, i * step:(i + 1) * step]))
            r = ref.step(out.probs.cpu().numpy(), resets.get(i, ()))
            compare_detector(out, r)
            probs_seen.append(r[2][r[1] >= 0])
        branches |= ref.branches
    assert branches == {"warming up", "below threshold", "same label", "suppressed", "first", "new label"}, branches


def test_stream_reset_forms(emu_lib):
    St = streaming()
    fe, net, _, _, _ = setup(emu_lib)
    det = St.StreamingDetector(net, fe, 4)
    det.reset(np.array([False, True, False, False]))
    det.reset([3])
    assert det._pending.tolist() == [False, True, False, True]
    with pytest.raises(T.TcrError):
        det.reset([4])
    with pytest.raises(T.TcrError):
        det.reset(np.zeros(3, bool))


def test_stream_argument_errors(emu_lib):
    St = streaming()
    fe, net, _, _, _ = setup(emu_lib)
    det = St.StreamingDetector(net, fe, 2, frames_per_step=2)
    with pytest.raises(T.TcrError, match="k \\* hop"):
        det.push(torch.zeros((2, 320)))
    with pytest.raises(T.TcrError, match="outside 1..T"):
        St.StreamingDetector(net, fe, 2, frames_per_step=fe.n_frames + 1)
    with pytest.raises(T.TcrError, match="outside 1..T"):
        St.StreamingDetector(net, fe, 2, frames_per_step=0)
    fe98 = Cm.make_frontend(emu_lib, 480, 160)
    with pytest.raises(T.TcrError, match="network expects"):
        St.StreamingDetector(net, fe98, 2)
    dep = Cm.make_frontend(emu_lib, 640, 320, method="mfcc_deploy")
    with pytest.raises(T.TcrError, match="deploy"):
        St.StreamingDetector(net, dep, 2)
    with pytest.raises(T.TcrError, match="min_count"):
        St.StreamingDetector(net, fe, 2, average_window_ms=40, min_count=3)
    for bad in (0, -1):
        with pytest.raises(T.TcrError, match="positive"):
            St.StreamingDetector(net, fe, bad)
    # the C entry points refuse on their own (size 0 / TCR_ERR_ARG + message)
    lib = emu_lib
    good = T._lib.DetectCfg(4, 2, 0, 0.5)
    assert lib.tcr_stream_state_bytes(C.byref(fe.cfg), net._h, 0, 1, C.byref(good)) == 0 and b"positive" in lib.tcr_last_error()
    assert lib.tcr_stream_state_bytes(C.byref(fe.cfg), net._h, 2, 1, C.byref(T._lib.DetectCfg(0, 1, 0, 0.5))) == 0
    assert lib.tcr_stream_workspace_bytes(C.byref(dep.cfg), net._h, 2, 1) == 0 and b"deploy" in lib.tcr_last_error()
    ws = torch.zeros(16)
    assert lib.tcr_stream_init(C.byref(fe.cfg), fe.plan.data_ptr(), net._h, 2, 1, C.byref(good), ws.data_ptr(), ws.data_ptr(), 64,
                               None) == -3


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_stream_4096_random_resets(hip_lib):
    St = streaming()
    fe, net, arch, p, s = setup(hip_lib)
    S, steps = 4096, 200
    det = St.StreamingDetector(net, fe, S)
    ss = net.fold_bn()
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
        if (i + 1) % 50 == 0:
            ref = check_step(fe, net, ss, det, clip, out)
            pick = rng.choice(S, 32, replace=False)
            want = R.forward(arch, p, s, fe.reference_view(ref[pick])[..., 0].cpu().numpy().astype(np.float64), False)["logits"]
            assert np.abs(out.logits[pick].cpu().numpy() - want).max() < 1e-4


@pytest.mark.gpu
def test_gpu_stream_no_drift(hip_lib):
    St = streaming()
    fe, net, _, _, _ = setup(hip_lib)
    det = St.StreamingDetector(net, fe, 1)
    steps, hop = 3000, fe.cfg.hop
    audio = torch.from_numpy((np.random.RandomState(5).uniform(-1, 1, steps * hop) * 0.4).astype(np.float32)).cuda()
    for i in range(steps):
        det.push(audio[i * hop:(i + 1) * hop].view(1, hop))
    assert torch.equal(det.window(), fe(audio[-fe.n_samples:].view(1, -1).contiguous()))


@pytest.mark.gpu
def test_gpu_stream_permutation(hip_lib):
    St = streaming()
    fe, net, _, _, _ = setup(hip_lib)
    S = 64
    a, b = St.StreamingDetector(net, fe, S, min_count=1), St.StreamingDetector(net, fe, S, min_count=1)
    perm = torch.from_numpy(np.random.RandomState(1).permutation(S)).cuda()
    g = torch.Generator(device="cuda").manual_seed(2)
    for i in range(12):
        x = ((torch.rand((S, fe.cfg.hop), device="cuda", generator=g) * 2 - 1) * 0.5).contiguous()
        oa = [t.clone() for t in a.push(x)]
        ob = b.push(x[perm].contiguous())
        for ta, tb in zip(oa, ob):
            assert torch.equal(ta[perm], tb)
    assert torch.equal(a.window()[perm], b.window())


@pytest.mark.gpu
def test_gpu_stream_tcresnet14_3010(hip_lib):
    fe, net, arch, p, s = setup(hip_lib, "TCResNet14", 1.5, win=480, hop=160)
    run_checked(hip_lib, fe, net, arch, p, s, 64, 4, 30, {10: [0, 5], 20: list(range(0, 64, 3))})


@pytest.mark.gpu
def test_gpu_prepared_is_push_and_refuses_stale_weights(hip_lib):
    St = streaming()
    fe, net, _, _, _ = setup(hip_lib)
    S = 16
    a, b = St.StreamingDetector(net, fe, S, min_count=1), St.StreamingDetector(net, fe, S, min_count=1)
    buf = torch.zeros((S, fe.cfg.hop), device="cuda")
    call = b.prepared(buf)
    g = torch.Generator(device="cuda").manual_seed(4)
    for i in range(10):
        x = (torch.rand((S, fe.cfg.hop), device="cuda", generator=g) * 2 - 1) * 0.5
        if i == 5:
            a.reset([2, 7])
            b.reset([2, 7])
        oa = [t.clone() for t in a.push(x)]
        buf.copy_(x)
        ob = call()
        for ta, tb in zip(oa, ob):
            assert torch.equal(ta, tb)
    with torch.no_grad():
        net.params[0] += 0.25
    with pytest.raises(T.TcrError, match="prepare it again"):
        call()
    out = a.push(buf)                                   # push refolds
    assert torch.equal(out.logits, net.forward_frozen(a.window().clone(), net.fold_bn())[0])
    ob = b.prepared(buf)()
    assert torch.equal(ob.logits, out.logits)


def frozen_artifact(net, fe, path, method="mfcc"):
    from tcresnet_amd import deploy
    meta = {"format": deploy.FORMAT, "model": "TCResNet8Model", "family": "tcresnet", "scope": net.scope, "channels": net.channels,
            "num_classes": net.num_classes, "include_preprocess": True, "height": net.t_in, "width": net.in_channels, "channels_in": 1,
            "bn_decay": float(net.cfg.bn_decay), "bn_eps": float(net.cfg.bn_eps),
            "inputs": [{"name": "input/audio/before_preprocessing", "shape": [1, fe.n_samples, 1]}],
            "output": {"name": "output/softmax", "shape": [1, net.num_classes]},
            "frontend": {"sample_rate": 16000, "clip_duration_ms": 1000, "window_size_samples": int(fe.cfg.win),
                         "window_stride_samples": int(fe.cfg.hop), "num_mel_bins": 64, "num_mfccs": int(fe.cfg.n_coef),
                         "lower_edge_hertz": 80.0, "upper_edge_hertz": 7600.0, "method": method}}
    consts = {k: v for k, v in net.state_dict().items() if k.endswith("/weights")}
    consts["__folded_batch_norm__"] = net.fold_bn().cpu().numpy()
    return deploy.FrozenModel(meta, consts, lib=net.lib, device=net.device).save(path)


@pytest.mark.gpu
def test_gpu_frozen_model_streaming_round_trip(hip_lib, tmp_path):
    St = streaming()
    from tcresnet_amd import deploy
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    model = deploy.FrozenModel.load(path, lib=hip_lib, device="cuda")
    S = 8
    a = St.StreamingDetector(net, fe, S, frames_per_step=2, min_count=2)
    b = model.streaming(S, frames_per_step=2, min_count=2)
    g = torch.Generator(device="cuda").manual_seed(6)
    for i in range(15):
        x = (torch.rand((S, 2 * fe.cfg.hop), device="cuda", generator=g) * 2 - 1) * 0.4
        oa = [t.clone() for t in a.push(x)]
        for ta, tb in zip(oa, b.push(x)):
            assert torch.equal(ta, tb)
    dep = frozen_artifact(net, fe, str(tmp_path / "dep.npz"), method="mfcc_deploy")
    with pytest.raises(T.TcrError, match="deploy"):
        deploy.FrozenModel.load(dep, lib=hip_lib, device="cuda").streaming(2)
    with pytest.raises(ValueError, match="TC-ResNet"):
        deploy.FrozenModel.streaming(types.SimpleNamespace(meta={"family": "dscnn"}, frontend=None), 2)


def write_wav(path, pcm):
    data = pcm.astype("<i2").tobytes()
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        fh.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16))
        fh.write(b"data" + struct.pack("<I", len(data)) + data)


@pytest.mark.gpu
def test_gpu_stream_audio_cli(hip_lib, tmp_path):
    St = streaming()
    from tcresnet_amd import deploy
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    audio = segment_audio(2, 64000, 11)
    pcm = [np.clip(audio[0] * 32767, -32768, 32767).astype(np.int16), np.clip(audio[1, :41234] * 32767, -32768, 32767).astype(np.int16)]
    wavs = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    labels = [f"c{i}" for i in range(12)]
    kw = dict(frames_per_step=2, average_window_ms=200, min_count=2, detection_threshold=0.3, suppression_ms=400)
    cmd = [sys.executable, os.path.join(ROOT, "tc-resnet_amd", "stream_audio.py"), "--frozen", path, "--wav", *wavs, "--labels", ",".join(labels)]
    for k, v in kw.items():
        cmd += [f"--{k}", str(v)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = r.stdout.strip().splitlines()
    assert "dropping" in r.stderr
    # the Python API on the same audio
    model = deploy.FrozenModel.load(path, lib=hip_lib, device="cuda")
    det = model.streaming(2, **kw)
    step = det.step_samples
    lens = [len(x) // step * step for x in pcm]
    want = []
    from tcresnet_amd.stream_audio import format_time_ms
    for i in range(max(lens) // step):
        x = np.zeros((2, step), np.float32)
        for sidx in range(2):
            if (i + 1) * step <= lens[sidx]:
                x[sidx] = pcm[sidx][i * step:(i + 1) * step].astype(np.float32) * (1.0 / 32768.0)
        out = det.push(torch.from_numpy(x).cuda())
        for sidx in np.nonzero(out.is_new.cpu().numpy())[0]:
            want.append(f"{wavs[sidx]},{format_time_ms(1000.0 * (i + 1) * step / 16000)},{labels[int(out.top[sidx])]},"
                        f"{float(out.score[sidx]):.6f}")
    assert got == want
    assert len(want) >= 2
