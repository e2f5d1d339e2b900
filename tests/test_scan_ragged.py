"""Ragged scanning (tcr_scan_ragged, KeywordScanner.scan_ragged) and the ragged sweep (tcr_detect_sweep_ragged): signals of different
lengths packed into one call.  The reference of every bitwise check is the dense path: each signal's rows are `scan` of that signal
alone, and the sweep's counts are the dense sweep of the zero-padded scan with lengths=.  Emulator (`-m "not gpu"`) and MI355X
(`-m gpu`)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import DET, assert_bitwise
from tests.test_streaming import frozen_artifact, segment_audio, setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("logits", "probs", "smoothed", "top", "score", "is_new")
_CACHE = {}


def scanning():
    from tcresnet_amd import scanning as Sc
    return Sc


def cut_signals(lib, audio, steps, step_samples):
    """Row n of audio [N, L] cut to steps[n] steps, on the device."""
    return [Cm.to_dev(lib, audio[n, :int(s) * step_samples]) for n, s in enumerate(steps)]


def solo_scans(sc, signals):
    """The reference: the dense scan of every signal that has steps, alone (None for the others)."""
    return [sc.scan(x[None, :]) if x.numel() else None for x in signals]


def check_ragged_equals_solo(out, want, steps):
    assert len(out) == len(steps)
    assert out.offsets.tolist() == np.concatenate([[0], np.cumsum(steps)]).tolist()
    assert out.logits.shape[0] == int(np.sum(steps)) and out.top.shape == (int(np.sum(steps)),)
    for n, w in enumerate(want):
        got = out.signal(n)
        if w is None:
            assert got.top.shape == (1, 0) and got.logits.shape[:2] == (1, 0)
        else:
            assert_bitwise(got, w)


def check_family_case(lib, fe, net, steps, k, seed, det=DET, max_windows=(None,)):
    Sc = scanning()
    step = k * fe.cfg.hop
    signals = cut_signals(lib, segment_audio(len(steps), max(steps) * step, seed), steps, step)
    want = solo_scans(Sc.KeywordScanner(net, fe, frames_per_step=k, **det), signals)
    outs = [Sc.KeywordScanner(net, fe, frames_per_step=k, max_windows=m, **det).scan_ragged(signals) for m in max_windows]
    for o in outs:
        check_ragged_equals_solo(o, want, steps)
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o.tensors(), outs[0].tensors()))
    return outs[0]


def events_at_detections(out, n, step_ms, length_ms, gap_ms, limit):
    """Events (start_ms, end_ms, label) of signal n that start half a step before a detection of the scan `out` and last length_ms, a
    later one at least gap_ms after the earlier one's end, `limit` at the most: events that the sweep can hit."""
    a, b = int(out.offsets[n]), int(out.offsets[n + 1])
    fired = np.flatnonzero(out.is_new[a:b].cpu().numpy())
    top = out.top[a:b].cpu().numpy()
    events, free = [], 0.0
    for i in fired:
        t = step_ms * (i + 1)
        if t - step_ms / 2 > free and len(events) < limit:
            events.append((t - step_ms / 2, t - step_ms / 2 + length_ms, int(top[i])))
            free = events[-1][1] + gap_ms
    return events


# ---- emulator -------------------------------------------------------------------------------------------------------------------
STEPS_1 = [1, 24, 0, 63, 7, 8]


def case_1(lib):
    """The 4020, k = 1 corpus of six signals, its solo dense scans and its ragged scans at max_windows 1, 7 and the default
    (computed once per process)."""
    if "case_1" not in _CACHE:
        Sc = scanning()
        fe, net, _, _, _ = setup(lib)
        audio = segment_audio(len(STEPS_1), max(STEPS_1) * 320, 3)
        signals = cut_signals(lib, audio, STEPS_1, 320)
        want = solo_scans(Sc.KeywordScanner(net, fe, **DET), signals)
        outs = [Sc.KeywordScanner(net, fe, max_windows=m, **DET).scan_ragged(signals) for m in (1, 7, None)]
        _CACHE["case_1"] = dict(fe=fe, net=net, audio=audio, signals=signals, want=want, outs=outs)
    return _CACHE["case_1"]


def test_ragged_scan_equals_solo_scans(emu_lib):
    """max_windows = 7 forces several groups per signal and chunks that span signals; W = 5 steps straddles every boundary."""
    c = case_1(emu_lib)
    for o in c["outs"]:
        check_ragged_equals_solo(o, c["want"], STEPS_1)
        assert o.offsets.tolist() == [0, 1, 25, 25, 88, 95, 103]
    for o in c["outs"][1:]:
        assert all(torch.equal(a, b) for a, b in zip(o.tensors(), c["outs"][0].tensors()))
    out = c["outs"][2]
    assert int(out.is_new.sum()) >= 3
    assert int((out.top == -1).sum()) == 5                # one step below min_count = 2 per signal that has steps
    assert out.steps.tolist() == STEPS_1


def test_ragged_scan_packed_form_equals_list_form(emu_lib):
    Sc = scanning()
    c = case_1(emu_lib)
    sc = Sc.KeywordScanner(c["net"], c["fe"], max_signals=2, **DET)       # fewer than the call brings: the tables are reallocated
    out = sc.scan_ragged((torch.cat(c["signals"]), [s * 320 for s in STEPS_1]))
    assert sc.max_signals == 6
    assert all(torch.equal(a, b) for a, b in zip(out.tensors(), c["outs"][2].tensors()))


def test_ragged_scan_k3(emu_lib):
    fe, net, _, _, _ = setup(emu_lib)
    out = check_family_case(emu_lib, fe, net, [21, 5], 3, 4, max_windows=(4, None))
    assert out.offsets.tolist() == [0, 21, 26]


def test_ragged_scan_3010_log_mel_k2(emu_lib):
    fe, net, _, _, _ = setup(emu_lib, win=480, hop=160, method="log_mel_spectrogram")
    check_family_case(emu_lib, fe, net, [17, 0, 30], 2, 5, max_windows=(8,))


@pytest.mark.parametrize("model", ["dscnn_s", "tiny_conv"])
def test_ragged_scan_families(emu_lib, model):
    """DS-CNN, and a 2-D graph (the planes gather)."""
    from tests.test_detect_families import MODELS
    fe, net = MODELS[model](emu_lib)
    check_family_case(emu_lib, fe, net, [9, 2, 14], 1, 6, max_windows=(5,))


THRESHOLDS = [float("-inf"), 0.0, 0.25, 0.5, float("inf")]


def test_ragged_sweep_equals_padded_dense_sweep(emu_lib):
    Sc = scanning()
    c = case_1(emu_lib)
    fe, net, out = c["fe"], c["net"], c["outs"][2]
    sc = Sc.KeywordScanner(net, fe, **DET)                # 20 ms steps
    off = out.offsets
    events = [events_at_detections(out, n, 20.0, 60.0, 45.0, 2) if n in (1, 3) else [] for n in range(len(STEPS_1))]
    assert len(events[1]) >= 1 and len(events[3]) >= 1
    res = sc.sweep(out, THRESHOLDS, events=events, tolerance_ms=40.0, return_fired=True)
    padded = np.zeros((len(STEPS_1), max(STEPS_1) * 320), np.float32)
    for n, s in enumerate(STEPS_1):
        padded[n, :s * 320] = c["audio"][n, :s * 320]
    dense = sc.scan(Cm.to_dev(emu_lib, padded))
    ref = sc.sweep(dense, THRESHOLDS, events=events, lengths=[s * 320 for s in STEPS_1], tolerance_ms=40.0, return_fired=True)
    for name in ("detections", "hits", "duplicates"):
        assert torch.equal(getattr(res, name), getattr(ref, name)), name
    assert int(res.hits.sum()) >= 1 and int(res.detections[:, 0].sum()) >= 3
    assert int(res.detections[:, 4].sum()) == 0           # nothing exceeds +inf
    assert res.fired.shape == (len(THRESHOLDS), 103)
    for t in range(len(THRESHOLDS)):
        for n, s in enumerate(STEPS_1):
            assert torch.equal(res.fired[t, off[n]:off[n + 1]], ref.fired[t, n, :s]), (t, n)
    assert np.array_equal(res.events, ref.events) and np.allclose(res.hours, np.array(STEPS_1) * 0.02 / 3600, rtol=0, atol=1e-15)
    assert np.array_equal(res.hours, ref.hours)
    for t, th in enumerate(THRESHOLDS):
        want = Sc.KeywordScanner(net, fe, **dict(DET, detection_threshold=th)).scan_ragged(c["signals"]).is_new
        assert torch.equal(res.fired[t].to(torch.int32), want), th
    # the raw form
    raw = Sc.detection_sweep(out.top, out.score, THRESHOLDS, sc.suppression_steps, 12, step_offsets=off, lib=emu_lib)
    assert torch.equal(raw.detections, res.detections) and raw.fired is None and int(raw.hits.sum()) == 0


def test_ragged_argument_errors(emu_lib):
    Sc = scanning()
    lib = emu_lib
    fe, net, _, _, _ = setup(lib)
    sc = Sc.KeywordScanner(net, fe, frames_per_step=2)    # k * hop = 640
    z = lambda n: torch.zeros(n)
    with pytest.raises(T.TcrError, match="not a multiple of k \\* hop"):
        sc.scan_ragged([z(640), z(1000)])
    with pytest.raises(T.TcrError, match="not a multiple of k \\* hop"):
        sc.scan_ragged((z(1640), [640, 1000]))
    with pytest.raises(T.TcrError, match="sample_offsets decrease at signal 1"):
        sc.scan_ragged((z(640), [1280, -640]))
    with pytest.raises(T.TcrError, match="total_steps == 0"):
        sc.scan_ragged([z(0), z(0)])
    with pytest.raises(T.TcrError, match="lengths sum to"):
        sc.scan_ragged((z(640), [640, 640]))
    with pytest.raises(T.TcrError, match="1-D"):
        sc.scan_ragged([torch.zeros((1, 640))])
    with pytest.raises(T.TcrError, match="max_signals"):
        Sc.KeywordScanner(net, fe, max_signals=0)
    out = Sc.KeywordScanner(net, fe, **DET).scan_ragged([z(640), z(0), z(320)])
    assert out.offsets.tolist() == [0, 2, 2, 3]
    with pytest.raises(T.TcrError, match="lengths given with a ragged scan"):
        sc.sweep(out, [0.5], lengths=[640, 0, 320])
    with pytest.raises(T.TcrError, match="events for 2 signals, the scan has 3"):
        sc.sweep(out, [0.5], events=[[], []])
    with pytest.raises(T.TcrError, match="valid_steps with step_offsets"):
        Sc.detection_sweep(out.top, out.score, [0.5], 0, 12, valid_steps=[2, 0, 1], step_offsets=out.offsets, lib=lib)
    with pytest.raises(T.TcrError, match="step_offsets must run from 0"):
        Sc.detection_sweep(out.top, out.score, [0.5], 0, 12, step_offsets=[1, 2, 3], lib=lib)
    with pytest.raises(T.TcrError, match="step_offsets must run from 0"):
        Sc.detection_sweep(out.top, out.score, [0.5], 0, 12, step_offsets=[0, 3, 2, 3], lib=lib)
    # the C entries refuse on their own (status + message), before anything is launched: the buffers below are never touched
    det = T._lib.DetectCfg(4, 2, 0, 0.5)
    ref = T._lib.ModelRef(T._lib.FAMILY_TCRESNET, net._h.value, net.params.data_ptr(), net.fold_bn().data_ptr())
    buf = torch.full((1 << 16,), 7.0)
    p = buf.data_ptr()
    ws_bytes = lib.tcr_scan_ragged_workspace_bytes(C.byref(fe.cfg), C.byref(ref), 1, 16, 4)
    assert ws_bytes == 256 + lib.tcr_scan_workspace_bytes_m(C.byref(fe.cfg), C.byref(ref), 1, 16)
    assert lib.tcr_scan_ragged_workspace_bytes(C.byref(fe.cfg), C.byref(ref), 1, 16, 0) == 0 and b"max_signals" in lib.tcr_last_error()
    assert lib.tcr_scan_ragged_workspace_bytes(C.byref(fe.cfg), C.byref(ref), 1, 0, 4) == 0 and b"max_windows" in lib.tcr_last_error()

    def call(offsets, n=None, ws=1 << 18, d=det, samples=p, k=1):
        off = np.asarray(offsets, np.int64)
        return lib.tcr_scan_ragged(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), len(off) - 1 if n is None else n,
                                   off.ctypes.data if len(off) else None, k, C.byref(d), samples, p, ws, p, p, p, p, p, p, None)
    for args, kw, status, msg in [(([320, 640],), {}, -1, b"sample_offsets must start at 0"),
                                  (([0, 650],), {}, -1, b"length 650 of signal 0 is not a multiple of k * hop = 320"),
                                  (([0, 640, 320],), {}, -1, b"sample_offsets decrease at signal 1"),
                                  (([0, 0, 0],), {}, -1, b"total_steps == 0"),
                                  (([0, 320],), dict(n=0), -1, b"number of signals must be positive"),
                                  (([0] * 40,), dict(ws=512), -1, b"more than the max_signals"),
                                  (([],), dict(n=1), -1, b"null argument"),
                                  (([0, 320],), dict(samples=None), -1, b"null argument"),
                                  (([0, 320],), dict(ws=1024), -3, b"one window"),
                                  (([0, 320],), dict(k=0), -1, b"frames per step"),
                                  (([0, 320],), dict(d=T._lib.DetectCfg(0, 1, 0, 0.5)), -1, b"average_steps")]:
        assert call(*args, **kw) == status, (args, kw, lib.tcr_last_error())
        assert msg in lib.tcr_last_error(), (args, kw, lib.tcr_last_error())
    assert bool((buf == 7.0).all())

    def sweep(n=1, off=p, ncls=4, top=p, supp=0, nthr=1, dets=p, ev=None, hits=p):
        return lib.tcr_detect_sweep_ragged(n, off, ncls, top, p, supp, nthr, p, ev, p, p, p, dets, hits, p, None, None)
    for kw, msg in [(dict(off=None), b"null argument"), (dict(top=None), b"null argument"), (dict(dets=None), b"null argument"),
                    (dict(n=0), b"number of signals must be positive"), (dict(nthr=0), b"number of thresholds must be positive"),
                    (dict(ncls=257), b"num_classes 257 outside"), (dict(supp=-1), b"suppression_steps must be >= 0"),
                    (dict(ev=p, hits=None), b"events need"), (dict(n=1 << 12, nthr=1 << 12, ncls=200), b"too large")]:
        assert sweep(**kw) == -1, kw
        assert msg in lib.tcr_last_error(), (kw, lib.tcr_last_error())
    assert bool((buf == 7.0).all())


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
GPU_DET = dict(average_window_ms=1000, min_count=3, detection_threshold=0.3, suppression_ms=1500)


def gpu_corpus(lib):
    """64 signals of seeded 1..400 steps, one of them without steps, one of 1 step and one of 8200 (more than one 8192-step pass of
    scan_suppress_kernel), with their solo dense scans and the ragged scan at the default max_windows (once per process)."""
    if "gpu" not in _CACHE:
        Sc = scanning()
        fe, net, _, _, _ = setup(lib)
        steps = np.random.RandomState(41).randint(1, 401, 64)
        steps[5], steps[17], steps[40] = 0, 1, 8200
        audio = segment_audio(64, 400 * 320, 42)
        long = segment_audio(1, 8200 * 320, 43)[0]
        host = [long if n == 40 else audio[n, :s * 320] for n, s in enumerate(steps)]
        signals = [Cm.to_dev(lib, x) for x in host]
        sc = Sc.KeywordScanner(net, fe, **GPU_DET)
        want = solo_scans(sc, signals)
        out = sc.scan_ragged(signals)
        _CACHE["gpu"] = dict(fe=fe, net=net, steps=steps, signals=signals, sc=sc, want=want, out=out)
    return _CACHE["gpu"]


@pytest.mark.gpu
def test_gpu_ragged_scan_64_signals(hip_lib):
    Sc = scanning()
    c = gpu_corpus(hip_lib)
    check_ragged_equals_solo(c["out"], c["want"], c["steps"])
    other = Sc.KeywordScanner(c["net"], c["fe"], max_windows=1000, **GPU_DET).scan_ragged(c["signals"])
    assert all(torch.equal(a, b) for a, b in zip(other.tensors(), c["out"].tensors()))
    assert int(c["out"].is_new.sum()) >= 10


@pytest.mark.gpu
def test_gpu_ragged_sweep_64_thresholds(hip_lib):
    c = gpu_corpus(hip_lib)
    sc, out, steps = c["sc"], c["out"], c["steps"]
    off = out.offsets
    warm = out.score[out.top >= 0].cpu().numpy()
    thr = np.quantile(warm, np.linspace(0.0, 1.0, 64)).astype(np.float32)
    events = [[] for _ in steps]
    with_events = [40]                                   # the long one, and seven more that have detections
    for n in range(64):
        if len(with_events) < 8 and n != 40 and int(out.is_new[off[n]:off[n + 1]].sum()) >= 1:
            with_events.append(n)
    assert len(with_events) == 8
    for n in with_events:
        events[n] = events_at_detections(out, n, 20.0, 1000.0, 600.0, 50)
    assert sum(len(e) for e in events) >= 12
    res = sc.sweep(out, thr, events=events, tolerance_ms=500.0, return_fired=True)
    L = int(steps.max()) * 320
    padded = torch.zeros((64, L), dtype=torch.float32, device="cuda")
    for n, x in enumerate(c["signals"]):
        padded[n, :x.numel()] = x
    dense = sc.scan(padded)
    ref = sc.sweep(dense, thr, events=events, lengths=(steps * 320).tolist(), tolerance_ms=500.0, return_fired=True)
    for name in ("detections", "hits", "duplicates"):
        assert torch.equal(getattr(res, name), getattr(ref, name)), name
    assert int(res.hits.sum()) >= 1 and int(res.detections.sum()) > int(res.hits.sum())
    for n, s in enumerate(steps):
        assert torch.equal(res.fired[:, off[n]:off[n + 1]], ref.fired[:, n, :s]), n
    assert np.array_equal(res.hours, ref.hours)


@pytest.mark.gpu
def test_gpu_ragged_scan_tcresnet14_3010_k2(hip_lib):
    fe, net, _, _, _ = setup(hip_lib, "TCResNet14", 1.5, win=480, hop=160)
    steps = [int(s) for s in np.random.RandomState(45).randint(1, 300, 8)]
    out = check_family_case(hip_lib, fe, net, steps, 2, 46, det=dict(GPU_DET, average_window_ms=500, suppression_ms=600),
                            max_windows=(None, 333))
    assert int(out.is_new.sum()) >= 1


def write_wav(path, pcm, rate=16000):
    data = pcm.astype("<i2").tobytes()
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        fh.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16))
        fh.write(b"data" + struct.pack("<I", len(data)) + data)


def run_all(commands):
    """The commands as concurrent child processes (each opens the GPU once): [(returncode, stdout, stderr)]."""
    procs = [subprocess.Popen([sys.executable, *cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for cmd in commands]
    out = []
    for p in procs:
        so, se = p.communicate(timeout=600)
        out.append((p.returncode, so, se))
    return out


def cli_files(tmp_path, lengths, rates, seed):
    audio = segment_audio(len(lengths), max(lengths), seed)
    wavs = []
    for n, (m, rate) in enumerate(zip(lengths, rates)):
        x = audio[n, :m]
        if rate != 16000:                                 # (any 48 kHz signal will do: hold every sample three times)
            x = np.repeat(x, rate // 16000)
        wavs.append(str(tmp_path / f"f{seed}_{n}.wav"))
        write_wav(wavs[-1], np.clip(x * 32767, -32768, 32767).astype(np.int16), rate)
    return wavs


@pytest.mark.gpu
def test_gpu_scan_audio_cli_ragged(hip_lib, tmp_path):
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    lengths = [96000, 61234, 20000]                      # the second is written at 48 kHz
    mixed = cli_files(tmp_path, lengths, [16000, 48000, 16000], 51)
    equal = cli_files(tmp_path, [48000, 48000, 48000], [16000, 16000, 16000], 52)
    script = os.path.join(ROOT, "tc-resnet_amd", "scan_audio.py")
    common = ["--labels", ",".join(f"c{i}" for i in range(12)), "--frames_per_step", "2", "--average_window_ms", "200", "--min_count", "2",
              "--detection_threshold", "0.3", "--suppression_ms", "400"]
    cmd = lambda wavs, *extra: [script, "--frozen", path, "--wav", *wavs, *common, *extra]
    plain, ragged, plain_eq, ragged_eq, refused = run_all([cmd(mixed), cmd(mixed, "--ragged"), cmd(equal), cmd(equal, "--ragged"),
                                                           cmd(equal, "--ragged", "--chunk_seconds", "1")])
    for r in (plain, ragged, plain_eq, ragged_eq):
        assert r[0] == 0, r[2]
    assert refused[0] != 0 and "--chunk_seconds" in refused[2] and refused[1] == ""
    end_ms = {w: 1000.0 * (m // 640 * 640) / 16000 for w, m in zip(mixed, lengths)}
    kept = [line for line in plain[1].splitlines(keepends=True) if float(line.split(",")[1]) <= end_ms[line.split(",")[0]]]
    assert ragged[1] == "".join(kept)
    assert len(kept) >= 3 and len(kept) < len(plain[1].splitlines())       # the padded run fires after a file's end, the ragged does not
    assert "48000 Hz -> 16000 Hz" in ragged[2]
    assert ragged_eq[1] == plain_eq[1] and len(plain_eq[1].splitlines()) >= 3


@pytest.mark.gpu
def test_gpu_sweep_audio_cli_ragged(hip_lib, tmp_path):
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    lengths = [20 * 16000, 11 * 16000 + 77, 3 * 16000]
    wavs = cli_files(tmp_path, lengths, [16000, 48000, 16000], 53)
    labels = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(10)]
    rows = [(wavs[0], 1000, 2000, "w0"), (wavs[0], 5000, 6500, "w3"), (wavs[1], 2000, 3000, "w7"), (wavs[2], 500, 900, "w1")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{a},{b},{c}\n" for f, a, b, c in rows))
    cmd = lambda *extra: [os.path.join(ROOT, "tc-resnet_amd", "sweep_audio.py"), "--frozen", path, "--wav", *wavs, "--labels", ",".join(labels),
                          "--events", str(ev_csv), "--thresholds", "0:0.9:0.1", "--tolerance_ms", "500", "--target_fa_per_hour", "1000", *extra]
    plain, ragged = run_all([cmd(), cmd("--ragged")])
    assert plain[0] == 0, plain[2]
    assert ragged[0] == 0, ragged[2]
    assert ragged[1] == plain[1] and len(plain[1].splitlines()) == 11
    assert ragged[2].strip().splitlines()[-1] == plain[2].strip().splitlines()[-1]      # the hours and the operating point
