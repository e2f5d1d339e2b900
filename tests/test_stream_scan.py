"""Many-step pushes on streaming state (tcr_stream_scan, StreamingDetector.push_many): m steps in one call are bitwise m `push` calls,
outputs and the state they leave, so a recording scanned in pieces is bitwise one scan of the whole.  Emulator (`-m "not gpu"`) and
MI355X (`-m gpu`)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import assert_bitwise, pushed, scanning
from tests.test_streaming import frozen_artifact, segment_audio, setup, write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def streaming():
    from tcresnet_amd import streaming as St
    return St


def align64(v):
    return (v + 63) // 64 * 64


def state_parts(det):
    """The state's regions (stream.hip, StreamGeom): window [S, n_coef, Tp], tail [S, tail_len], ring [W, S, C], integers [5, S]."""
    cfg, S, W, ncls = det.frontend.cfg, det.n_streams, det.average_steps, det.net.num_classes
    tp = T._lib.padded_len(cfg.n_frames)
    tail_len = max(cfg.win - cfg.hop + (cfg.n_samples - cfg.win) % cfg.hop, 0)     # (hop > win: no tail is kept when it is negative)
    o = align64(S * cfg.n_coef * tp)
    o = align64(o + cfg.n_coef * tp)
    tail_off = o
    o = align64(o + S * tail_len)
    ring_off = o
    o = align64(o + W * S * ncls)
    st = det.state
    return (st[:S * cfg.n_coef * tp].view(S, cfg.n_coef, tp), st[tail_off:tail_off + S * tail_len].view(S, tail_len),
            st[ring_off:ring_off + W * S * ncls].view(W, S, ncls), st[o:o + 5 * S].view(torch.int32).view(5, S))


def assert_same_state(a, b):
    """Window, tail, the five integers and the ring slots of the last min(count, W) vectors bitwise (other slots are never read)."""
    wa, ta, ra, ia = state_parts(a)
    wb, tb, rb, ib = state_parts(b)
    assert torch.equal(wa, wb), int((wa != wb).sum())
    assert torch.equal(ta, tb), int((ta != tb).sum())
    assert torch.equal(ia, ib), (ia.cpu().numpy(), ib.cpu().numpy())
    ints = ia.cpu().numpy()
    W = a.average_steps
    for s in range(a.n_streams):
        head, count = int(ints[0, s]), int(ints[1, s])
        for d in range(1, count + 1):
            slot = (head - d) % W
            assert torch.equal(ra[slot, s], rb[slot, s]), (s, slot)


def push_chunks(det, x, chunks):
    """push_many over consecutive chunks of x [S, L] (steps per chunk), outputs concatenated over steps."""
    step, pos, outs = det.step_samples, 0, []
    for m in chunks:
        outs.append(det.push_many(x[:, pos:pos + m * step].contiguous()))
        pos += m * step
    assert pos == x.shape[1]
    return [torch.cat([o[f] for o in outs], dim=1) for f in range(6)]


def check_chunks_equal_scan(lib, fe, net, audio, k, chunks, det, **kw):
    Sc = scanning()
    x = Cm.to_dev(lib, audio)
    want = Sc.KeywordScanner(net, fe, frames_per_step=k, **det).scan(x)
    d = streaming().StreamingDetector(net, fe, audio.shape[0], frames_per_step=k, **det, **kw)
    got = push_chunks(d, x, chunks)
    assert_bitwise(got, want)
    return got, d


# ---- emulator -------------------------------------------------------------------------------------------------------------------
DET = dict(average_window_ms=200, min_count=2, detection_threshold=0.0, suppression_ms=200)


@pytest.mark.parametrize("k,chunks", [(1, [1, 3, 20, 2, 30, 7]),      # W = 10, T / k = 49, G <= 16 (max_windows = 16)
                                      (2, [1, 5, 17, 8]),
                                      (3, [1, 2, 12, 6]),
                                      (49, [1, 2, 1, 3])])
def test_push_many_4020_equals_scan(emu_lib, k, chunks):
    fe, net, _, _, _ = setup(emu_lib)
    assert fe.n_frames == 49
    det = DET if k < 49 else dict(DET, average_window_ms=2000, suppression_ms=1000)
    L = sum(chunks) * k * fe.cfg.hop
    got, _ = check_chunks_equal_scan(emu_lib, fe, net, segment_audio(2, L, 40 + k), k, chunks, det, max_windows=16)
    assert int(got[5].sum()) >= 1


def test_push_many_3010_log_mel_equals_scan(emu_lib):
    fe, net, _, _, _ = setup(emu_lib, win=480, hop=160, method="log_mel_spectrogram")
    assert fe.n_frames == 98 and fe.n_coef == 64
    got, _ = check_chunks_equal_scan(emu_lib, fe, net, segment_audio(2, 50 * 320, 45), 2, [1, 4, 30, 15], DET, max_windows=16)
    assert int(got[5].sum()) >= 1


def test_push_many_interleaved_with_push_and_resets(emu_lib):
    """push, push_many and push in any order, resets pending before push_many on some streams: outputs and state bitwise the
    pure-push detector's after every call."""
    St = streaming()
    fe, net, _, _, _ = setup(emu_lib)
    k, S = 2, 3
    det = dict(average_window_ms=120, min_count=2, detection_threshold=0.0, suppression_ms=120)      # W = 3, suppression 3 steps
    ref = St.StreamingDetector(net, fe, S, frames_per_step=k, **det)
    dut = St.StreamingDetector(net, fe, S, frames_per_step=k, max_windows=8, **det)
    step = ref.step_samples
    plan = [("push", 1, None), ("many", 4, [1]), ("push", 1, None), ("many", 1, None), ("many", 7, [0, 2]), ("push", 1, [1]),
            ("many", 2, None), ("many", 23, [2]), ("push", 1, None)]
    audio = Cm.to_dev(emu_lib, segment_audio(S, sum(m for _, m, _ in plan) * step, 46))
    pos = 0
    for kind, m, rst in plan:
        x = audio[:, pos:pos + m * step].contiguous()
        pos += m * step
        if rst:
            ref.reset(rst)
            dut.reset(rst)
        want = pushed(ref, x)
        if kind == "push":
            got = [t.unsqueeze(1) for t in dut.push(x)]
        else:
            got = dut.push_many(x)
        assert_bitwise(got, want)
        assert_same_state(dut, ref)
    assert pos == audio.shape[1]


def test_push_many_chunking_invariance(emu_lib):
    """max_windows = 1 (G = 1: every group past the first T / k reads carried columns), 7 and the default give the same bits."""
    St = streaming()
    fe, net, _, _, _ = setup(emu_lib)
    x = Cm.to_dev(emu_lib, segment_audio(2, 30 * 320, 47))
    chunks = [1, 3, 26]
    outs, dets = [], []
    for mw in (1, 7, None):
        d = St.StreamingDetector(net, fe, 2, max_windows=mw, **DET)
        outs.append(push_chunks(d, x, chunks))
        dets.append(d)
    want = scanning().KeywordScanner(net, fe, **DET).scan(x)
    for o, d in zip(outs, dets):
        assert_bitwise(o, want)
        assert_same_state(d, dets[0])


def test_push_many_refusals(emu_lib):
    St = streaming()
    fe, net, _, _, _ = setup(emu_lib)
    det = St.StreamingDetector(net, fe, 2, frames_per_step=2)
    with pytest.raises(T.TcrError, match="multiple of k \\* hop"):
        det.push_many(torch.zeros((2, 1000)))
    with pytest.raises(T.TcrError, match="push_many expects samples \\[2, m \\* 640\\]"):
        det.push_many(torch.zeros((3, 640)))
    with pytest.raises(T.TcrError, match="push_many expects"):
        det.push_many(torch.zeros(1280))
    with pytest.raises(T.TcrError, match="max_windows"):
        St.StreamingDetector(net, fe, 2, max_windows=0).push_many(torch.zeros((2, 320)))
    # the C entry point refuses on its own, with tcr_stream_step's messages (its own name in front)
    lib = emu_lib
    dep = Cm.make_frontend(emu_lib, 640, 320, method="mfcc_deploy")
    d = T._lib.DetectCfg(4, 2, 0, 0.5)
    buf = torch.zeros(1 << 16)
    ss = net.fold_bn()
    p = buf.data_ptr()

    def scan(n, L, ws_bytes, cfg=fe.cfg, dc=d, k=1):
        return lib.tcr_stream_scan(C.byref(cfg), fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), n, L, k, C.byref(dc),
                                   p, None, p, p, ws_bytes, p, p, p, p, p, p, None)

    def step(n, cfg=fe.cfg, dc=d, k=1):
        return lib.tcr_stream_step(C.byref(cfg), fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), n, k, C.byref(dc),
                                   p, None, p, p, 1 << 18, p, p, p, p, p, p, None)

    assert scan(1, 650, 1 << 18) == -1 and b"tcr_stream_scan: the signal length 650 is not a positive multiple of k * hop = 320" \
        == lib.tcr_last_error()
    assert scan(1, 640, 1024) == -3 and b"one window" in lib.tcr_last_error()
    for kw in (dict(cfg=dep.cfg), dict(dc=T._lib.DetectCfg(0, 1, 0, 0.5)), dict(dc=T._lib.DetectCfg(4, 5, 0, 0.5)), dict(k=50)):
        assert scan(1, 16000, 1 << 18, **kw) == -1
        got = lib.tcr_last_error()
        assert step(1, **kw) == -1
        assert got == lib.tcr_last_error().replace(b"tcr_stream_step", b"tcr_stream_scan"), got
    assert scan(0, 640, 1 << 18) == -1 and b"number of streams must be positive" in lib.tcr_last_error()


def test_wav_chunks_read_what_the_one_call_path_pads(tmp_path, capsys):
    """The tools' chunked reader (audio_input.Recordings): whole steps of every file, zeros once a file has ended, chunks rounded down
    to whole steps; concatenated they are the one-call path's zero-padded array, and the dropped samples are noted the same way."""
    from types import SimpleNamespace
    from tcresnet_amd.audio_input import Recordings
    from tcresnet_amd.datasets.augmentation_factory import read_wav_pcm16
    rng = np.random.RandomState(60)
    pcm = [rng.randint(-32768, 32767, n).astype(np.int16) for n in (33333, 1000, 12800, 0)]
    wavs = [str(tmp_path / f"{i}.wav") for i in range(len(pcm))]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    step = 640
    audio = [read_wav_pcm16(w).astype(np.float32) * (1.0 / 32768.0) for w in wavs]
    audio = [a[:len(a) // step * step] for a in audio]
    want = np.zeros((len(wavs), max(len(a) for a in audio)), np.float32)
    for s, a in enumerate(audio):
        want[s, :len(a)] = a
    # a detector's side of the reader: its step, rate and device (16 kHz files: no resampler, so no library)
    det = SimpleNamespace(step_samples=step, frontend=SimpleNamespace(cfg=SimpleNamespace(sample_rate=16000)), device=torch.device("cpu"), lib=None)
    rec = Recordings(wavs, det)
    assert rec.lengths == [len(a) for a in audio] and rec.n_steps == want.shape[1] // step
    assert capsys.readouterr().err.splitlines() == [f"{w}: dropping the last {len(x) % step} samples (not a whole step of {step})"
                                                    for w, x in zip(wavs, pcm) if len(x) % step]
    whole = list(rec.chunks())                                               # the one-call path: one chunk of every step
    assert len(whole) == 1 and whole[0][0] == 0 and np.array_equal(whole[0][1].numpy(), want)
    for sec in (0.1, 0.5, 1.0, 100.0):
        parts = list(rec.chunks(sec))
        assert [i0 for i0, _ in parts] == [i * max(1, int(sec * 16000) // step) for i in range(len(parts))]
        assert all(h.shape[1] % step == 0 and h.dtype == torch.float32 for _, h in parts)
        assert np.array_equal(np.concatenate([h.numpy() for _, h in parts], axis=1), want)
    with pytest.raises(SystemExit, match="shorter than one step"):
        list(rec.chunks(0.01))


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
GPU_DET = dict(average_window_ms=1000, min_count=3, detection_threshold=0.3, suppression_ms=1500)


def random_chunks(rng, steps, lo=1, hi=400):
    out = []
    while sum(out) < steps:
        out.append(min(int(rng.randint(lo, hi)), steps - sum(out)))
    return out


@pytest.mark.gpu
def test_gpu_push_many_64_streams_30s_random_chunks(hip_lib):
    fe, net, _, _, _ = setup(hip_lib)
    chunks = [1, 2, 40, 1] + random_chunks(np.random.RandomState(50), 1500 - 44)
    got, _ = check_chunks_equal_scan(hip_lib, fe, net, segment_audio(64, 30 * 16000, 51), 1, chunks, GPU_DET)
    assert got[0].shape == (64, 1500, 12)
    assert int(got[5].sum()) >= 1


@pytest.mark.gpu
def test_gpu_push_many_4096_streams_against_prepared_pushes(hip_lib):
    """One push_many of 1 s against 50 prepared pushes, after a second of pushes and with resets pending on some streams."""
    St = streaming()
    fe, net, _, _, _ = setup(hip_lib)
    S = 4096
    det = dict(GPU_DET, detection_threshold=0.05)
    ref = St.StreamingDetector(net, fe, S, **det)
    dut = St.StreamingDetector(net, fe, S, **det)
    warm = Cm.to_dev(hip_lib, segment_audio(S, 8 * 320, 52))
    for d in (ref, dut):
        pushed(d, warm)
    assert_same_state(dut, ref)
    rst = np.arange(0, S, 7)
    ref.reset(rst)
    dut.reset(rst)
    x = Cm.to_dev(hip_lib, segment_audio(S, 16000, 53))
    want = pushed(ref, x, prepared=True)
    got = dut.push_many(x)
    assert got.logits.shape == (S, 50, 12)
    assert_bitwise(got, want)
    assert_same_state(dut, ref)


@pytest.mark.gpu
def test_gpu_push_many_tcresnet14_3010(hip_lib):
    fe, net, _, _, _ = setup(hip_lib, "TCResNet14", 1.5, win=480, hop=160)
    chunks = [1, 10, 60, 3] + random_chunks(np.random.RandomState(54), 500 - 74, 1, 120)
    got, _ = check_chunks_equal_scan(hip_lib, fe, net, segment_audio(16, 10 * 16000, 55), 2, chunks, GPU_DET)
    assert int(got[5].sum()) >= 1


def _cli(script, args, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tc-resnet_amd", script), *args, *extra], capture_output=True, text=True,
                          timeout=600)


@pytest.mark.gpu
def test_gpu_scan_and_sweep_audio_chunked_equal_one_call(hip_lib, tmp_path):
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    audio = segment_audio(3, 40 * 16000, 56)
    pcm = [np.clip(audio[0] * 32767, -32768, 32767).astype(np.int16),
           np.clip(audio[1, :331234] * 32767, -32768, 32767).astype(np.int16),
           np.clip(audio[2, :12345] * 32767, -32768, 32767).astype(np.int16)]
    wavs = [str(tmp_path / f"{c}.wav") for c in "abc"]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    labels = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(10)]
    common = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), "--frames_per_step", "2", "--average_window_ms", "400",
              "--min_count", "2", "--suppression_ms", "600"]
    one = _cli("scan_audio.py", common + ["--detection_threshold", "0.2"], "--summary")
    assert one.returncode == 0, one.stderr
    assert len(one.stdout.strip().splitlines()) >= 2
    for sec in ("7.3", "0.5", "100"):
        ch = _cli("scan_audio.py", common + ["--detection_threshold", "0.2"], "--summary", "--chunk_seconds", sec)
        assert ch.returncode == 0, ch.stderr
        assert ch.stdout == one.stdout
        assert ch.stderr == one.stderr
    rows = [(wavs[0], 1000, 2000, "w0"), (wavs[0], 15000, 16500, "w3"), (wavs[1], 2000, 3000, "w7")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{a},{b},{c}\n" for f, a, b, c in rows))
    sw = common + ["--events", str(ev_csv), "--thresholds", "0:0.9:0.05", "--tolerance_ms", "500", "--target_fa_per_hour", "1000"]
    one = _cli("sweep_audio.py", sw, "--per_label")
    assert one.returncode == 0, one.stderr
    for sec in ("6.1", "100"):
        ch = _cli("sweep_audio.py", sw, "--per_label", "--chunk_seconds", sec)
        assert ch.returncode == 0, ch.stderr
        assert ch.stdout == one.stdout
        assert ch.stderr == one.stderr
