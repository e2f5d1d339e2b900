"""Cascade scans (scanning.CascadeScanner): a first scanner over every step, a second one over the steps around the first one's flags,
the second's detector over the merged posteriors.  The reference of every bitwise check is the existing code: `scan_ragged` of either
model, `redetect` and `sweep` of a merge the test builds itself with index_copy_.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import os

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import DET
from tests.test_scan_ragged import FIELDS, cli_files, cut_signals, run_all, scanning
from tests.test_scan_steps import select_reference
from tests.test_streaming import frozen_artifact, segment_audio, setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
THRESHOLDS = [float("-inf"), 0.0, 0.2, 0.4, float("inf")]


def pair_models(lib, pair):
    """(first fe, net, k), (second fe, net, k): both steps are 320 samples."""
    if pair == "tc8_tc14":
        fe1, net1, _, _, _ = setup(lib)
        fe2, net2, _, _, _ = setup(lib, "TCResNet14", 1.5, seed=2)
        return (fe1, net1, 1), (fe2, net2, 1)
    if pair == "tc8_tc8":
        fe1, net1, _, _, _ = setup(lib)
        fe2, net2, _, _, _ = setup(lib, seed=4)
        return (fe1, net1, 1), (fe2, net2, 1)
    from tests.test_detect_families import MODELS
    fe1, net1, _, _, _ = setup(lib, win=480, hop=160)               # 30 / 10 ms at k = 2
    fe2, net2 = MODELS["dscnn_s"](lib)                              # 40 / 20 ms at k = 1
    return (fe1, net1, 2), (fe2, net2, 1)


def case(lib, pair, steps, seed, **kw):
    """The two scanners of a pairing, the signals and both models' full ragged scans (computed once per process)."""
    key = (lib.kind, pair, tuple(steps), seed, tuple(sorted(kw.items())))
    if key not in _CACHE:
        Sc = scanning()
        (fe1, net1, k1), (fe2, net2, k2) = pair_models(lib, pair)
        first = Sc.KeywordScanner(net1, fe1, frames_per_step=k1, **DET, **kw)
        second = Sc.KeywordScanner(net2, fe2, frames_per_step=k2, **DET, **kw)
        assert first.step_samples == second.step_samples == 320
        signals = cut_signals(lib, segment_audio(len(steps), max(steps) * 320, seed), steps, 320)
        _CACHE[key] = dict(first=first, second=second, signals=signals, out1=first.scan_ragged(signals), out2=second.scan_ragged(signals))
    return _CACHE[key]


def assert_fields(got, want):
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), (f, int((getattr(got, f) != getattr(want, f)).sum()))


def keyword_peak(out):
    """Every step's largest first-stage probability over the keyword classes (2 on)."""
    return out.probs[:, 2:].max(dim=1).values.cpu().numpy()


def check_everything_selected(c):
    Sc = scanning()
    out = Sc.CascadeScanner(c["first"], c["second"], float("-inf")).scan_ragged(c["signals"])
    assert isinstance(out, Sc.CascadeOutput) and isinstance(out, Sc.RaggedScanOutput)
    assert_fields(out, c["out2"])
    assert out.selected.tolist() == list(range(out.top.shape[0])) and out.offsets.tolist() == c["out2"].offsets.tolist()
    assert_fields(out.first, c["out1"])


def check_nothing_selected(lib, c):
    from tests.test_net_configs import Log, kernel_of
    Sc = scanning()
    cascade = Sc.CascadeScanner(c["first"], c["second"], float("inf"))
    with Log(lib) as alone:
        c["first"].scan_ragged(c["signals"])
    with Log(lib) as g:
        out = cascade.scan_ragged(c["signals"])
    assert_fields(out, c["second"].redetect(c["out1"]))
    assert out.selected.numel() == 0 and out.selected.dtype == torch.int64
    if lib.kind == "emu":       # after the first stage's launches: the selection and the detector tail, no front-end and no network
        assert g.entries[:len(alone.entries)] == alone.entries and len(alone.entries) >= 4
        rest = {kernel_of(e) for e in g.entries[len(alone.entries):]}
        assert rest == {"select_flag_kernel", "select_count_kernel", "select_scan_kernel", "select_prefix_kernel", "select_dilate_kernel",
                        "select_compact_kernel", "scan_smooth_kernel", "scan_suppress_kernel"}, rest


def check_median(c, on="probs", **pads):
    """enter = the median of the first stage's keyword peak: some steps are the second model's, the others the first's."""
    Sc = scanning()
    first, second, out1, out2 = c["first"], c["second"], c["out1"], c["out2"]
    values = getattr(out1, on)
    enter = float(np.median(values[:, 2:].max(dim=1).values.cpu().numpy()))
    cascade = Sc.CascadeScanner(first, second, enter, on=on, **pads)
    total = int(out1.top.shape[0])
    want_sel, _ = select_reference(values.cpu().numpy(), out1.offsets, enter, list(range(2, 12)), cascade.pad_before, cascade.pad_after)
    assert 0 < want_sel.size < total, (want_sel.size, total)        # (the first-stage scan alone determines it)
    out = cascade.scan_ragged(c["signals"])
    assert out.selected.cpu().numpy().tolist() == want_sel.tolist()
    sel = out.selected
    rest = torch.ones(total, dtype=torch.bool, device=sel.device)
    rest[sel] = False
    for f in ("logits", "probs"):
        assert torch.equal(getattr(out, f)[sel], getattr(out2, f)[sel]), f
        assert torch.equal(getattr(out, f)[rest], getattr(out1, f)[rest]), f
    logits, probs = out1.logits.clone(), out1.probs.clone()
    logits.index_copy_(0, sel, out2.logits[sel])
    probs.index_copy_(0, sel, out2.probs[sel])
    ref = second.redetect(Sc.RaggedScanOutput(logits, probs, None, None, None, None, out1.offsets))
    assert_fields(out, ref)
    got, want = second.sweep(out, THRESHOLDS, return_fired=True), second.sweep(ref, THRESHOLDS, return_fired=True)
    for name in ("detections", "hits", "duplicates", "fired"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert int(got.detections[:, 0].sum()) >= 1
    return out


# ---- emulator -------------------------------------------------------------------------------------------------------------------
STEPS = [1, 30, 0, 50, 7]
EMU_PAIRS = ["tc8_tc14", "tc8_3010_k2_dscnn_s"]


@pytest.mark.parametrize("pair", EMU_PAIRS)
def test_cascade_everything_and_nothing_selected(emu_lib, pair):
    c = case(emu_lib, pair, STEPS, 21)
    check_everything_selected(c)
    check_nothing_selected(emu_lib, c)


@pytest.mark.parametrize("pair", EMU_PAIRS)
def test_cascade_median_threshold(emu_lib, pair):
    c = case(emu_lib, pair, STEPS, 21)
    out = check_median(c)                                           # the default pads: W - 1 = 4 steps on both sides
    assert isinstance(out.first, scanning().RaggedScanOutput)
    if pair == "tc8_tc14":
        check_median(c, on="smoothed", pad_before_ms=40, pad_after_ms=0)


def test_cascade_dense_scan_equals_ragged_rows(emu_lib):
    Sc = scanning()
    c = case(emu_lib, "tc8_tc8", [40, 40], 22)
    enter = float(np.median(keyword_peak(c["out1"])))
    cascade = Sc.CascadeScanner(c["first"], c["second"], enter, pad_before_ms=20, pad_after_ms=40)
    assert (cascade.pad_before, cascade.pad_after) == (1, 2)
    x = torch.stack(c["signals"])
    dense, ragged = cascade.scan(x), cascade.scan_ragged(c["signals"])
    assert isinstance(dense, Sc.ScanOutput) and 0 < ragged.selected.numel() < 80
    for f in FIELDS:
        got, want = getattr(dense, f), getattr(ragged, f)
        assert got.shape[:2] == (2, 40) and torch.equal(got.reshape(want.shape), want), f


def test_cascade_refusals(emu_lib):
    Sc = scanning()
    lib = emu_lib
    fe, net, _, _, _ = setup(lib)
    a = Sc.KeywordScanner(net, fe, **DET)
    with pytest.raises(T.TcrError, match="steps differ \\(320 and 640 samples\\)"):
        Sc.CascadeScanner(a, Sc.KeywordScanner(net, fe, frames_per_step=2, **DET), 0.5)
    fe10 = Cm.make_frontend(lib, 640, 320, num_mfccs=10)
    few = T.DSCNN("S", fe10.n_frames, fe10.n_coef, 10, lib=lib, device=Cm.device_of(lib))
    with pytest.raises(T.TcrError, match="12 and 10 classes"):
        Sc.CascadeScanner(a, Sc.KeywordScanner(few, fe10, **DET), 0.5)
    fe8 = Cm.make_frontend(lib, 320, 160, sample_rate=8000, upper_hz=3800.0)
    fe8b, net8, _, _, _ = setup(lib, win=640, hop=320)
    slow = Sc.KeywordScanner(net8, fe8b, **DET)
    slow.frontend = fe8                                             # (only the rate is read)
    with pytest.raises(T.TcrError, match="different sample rates \\(16000 and 8000 Hz\\)"):
        Sc.CascadeScanner(a, slow, 0.5)
    with pytest.raises(T.TcrError, match="on must be"):
        Sc.CascadeScanner(a, a, 0.5, on="logits")
    with pytest.raises(T.TcrError, match="enter_threshold is NaN"):
        Sc.CascadeScanner(a, a, float("nan"))
    with pytest.raises(T.TcrError, match="keyword_classes outside 0..11"):
        Sc.CascadeScanner(a, a, 0.5, keyword_classes=[12])
    with pytest.raises(T.TcrError, match="negative pads"):
        Sc.CascadeScanner(a, a, 0.5, pad_before_ms=-40)
    ok = Sc.CascadeScanner(a, a, 0.5)
    assert ok.keyword_classes == list(range(2, 12)) and (ok.pad_before, ok.pad_after) == (4, 4)
    with pytest.raises(T.TcrError, match="samples \\[N, L\\]"):
        ok.scan(torch.zeros(640))


def test_cli_cascade_flags_are_refused_without_ragged():
    """The argument checks come before any model is opened."""
    from tcresnet_amd import audio_input, scan_audio
    base = ["--frozen", "a.npz", "--wav", "a.wav"]
    for extra, msg in [(["--enter_threshold", "0.5"], "give --second_frozen"), (["--cascade_pad_ms", "100"], "give --second_frozen"),
                       (["--second_frozen", "b.npz"], "needs --enter_threshold"),
                       (["--second_frozen", "b.npz", "--enter_threshold", "0.5"], "--ragged only"),
                       (["--second_frozen", "b.npz", "--enter_threshold", "0.5", "--chunk_seconds", "1"], "--ragged only"),
                       (["--second_frozen", "b.npz", "--enter_threshold", "-inf", "--ragged_chunk_seconds", "1"], "--ragged only")]:
        with pytest.raises(SystemExit, match=msg):
            audio_input.open_cascade(scan_audio.parse_arguments(base + extra))
    args = scan_audio.parse_arguments(base + ["--second_frozen", "b.npz", "--enter_threshold", "-inf", "--ragged"])
    assert args.enter_threshold == float("-inf") and args.second_frames_per_step == 1 and args.cascade_pad_ms is None
    assert audio_input.open_cascade(scan_audio.parse_arguments(base + ["--ragged"])) is None


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
GPU_STEPS = np.random.RandomState(71).randint(1, 301, 64).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("max_windows", [16, None])
def test_gpu_cascade_64_signals(hip_lib, max_windows):
    """64 signals of 1 .. 300 steps, TCResNet8 (30 / 10 ms, k = 2) then DS-CNN-S."""
    c = case(hip_lib, "tc8_3010_k2_dscnn_s", GPU_STEPS, 72, max_windows=max_windows)
    check_everything_selected(c)
    check_nothing_selected(hip_lib, c)
    out = check_median(c)
    assert 0 < out.selected.numel() < sum(GPU_STEPS)


@pytest.mark.gpu
def test_gpu_cascade_tcresnet14(hip_lib):
    c = case(hip_lib, "tc8_tc14", GPU_STEPS[:16], 73)
    check_everything_selected(c)
    check_median(c, on="smoothed", pad_before_ms=100, pad_after_ms=20)


def cli_models(lib, tmp_path):
    fe, net, _, _, _ = setup(lib)
    fe2, net2, _, _, _ = setup(lib, seed=4)
    return frozen_artifact(net, fe, str(tmp_path / "first.npz")), frozen_artifact(net2, fe2, str(tmp_path / "second.npz"))


@pytest.mark.gpu
def test_gpu_scan_audio_cli_cascade(hip_lib, tmp_path):
    first, second = cli_models(hip_lib, tmp_path)
    wavs = cli_files(tmp_path, [64000, 41234, 20000], [16000, 16000, 16000], 74)
    script = os.path.join(ROOT, "tc-resnet_amd", "scan_audio.py")
    common = ["--wav", *wavs, "--labels", ",".join(f"c{i}" for i in range(12)), "--average_window_ms", "200", "--min_count", "2",
              "--detection_threshold", "0.3", "--suppression_ms", "400", "--ragged", "--summary"]
    own, everything, some, refused = run_all([
        [script, "--frozen", second, "--frames_per_step", "2", *common],
        [script, "--frozen", first, "--frames_per_step", "2", "--second_frozen", second, "--second_frames_per_step", "2", "--enter_threshold",
         "-inf", *common],
        [script, "--frozen", first, "--frames_per_step", "2", "--second_frozen", second, "--second_frames_per_step", "2", "--enter_threshold",
         "0.3", "--cascade_pad_ms", "80", *common],
        [script, "--frozen", first, "--second_frozen", second, "--second_frames_per_step", "2", "--enter_threshold", "0.3", *common]])
    for r in (own, everything, some):
        assert r[0] == 0, r[2]
    assert everything[1] == own[1] and len(own[1].splitlines()) >= 3
    import json
    total = sum(m // 640 for m in (64000, 41234, 20000))
    summary = json.loads(everything[2].strip().splitlines()[-1])
    assert summary["selected_steps"] == summary["total_steps"] == total
    assert "selected_steps" not in json.loads(own[2].strip().splitlines()[-1])
    assert 0 <= json.loads(some[2].strip().splitlines()[-1])["selected_steps"] <= total
    assert refused[0] != 0 and "steps differ" in refused[2] and refused[1] == ""


@pytest.mark.gpu
def test_gpu_sweep_audio_cli_cascade(hip_lib, tmp_path):
    first, second = cli_models(hip_lib, tmp_path)
    wavs = cli_files(tmp_path, [8 * 16000, 5 * 16000 + 77, 3 * 16000], [16000, 16000, 16000], 75)
    labels = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(10)]
    rows = [(wavs[0], 1000, 2000, "w0"), (wavs[0], 5000, 6500, "w3"), (wavs[1], 2000, 3000, "w7"), (wavs[2], 500, 900, "w1")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{a},{b},{c}\n" for f, a, b, c in rows))
    script = os.path.join(ROOT, "tc-resnet_amd", "sweep_audio.py")
    common = ["--wav", *wavs, "--labels", ",".join(labels), "--events", str(ev_csv), "--thresholds", "0:0.9:0.1", "--tolerance_ms", "500",
              "--target_fa_per_hour", "1000", "--ragged"]
    own, everything = run_all([[script, "--frozen", second, *common],
                               [script, "--frozen", first, "--second_frozen", second, "--enter_threshold", "-inf", *common]])
    assert own[0] == 0, own[2]
    assert everything[0] == 0, everything[2]
    assert everything[1] == own[1] and len(own[1].splitlines()) == 11
    assert '"selected_steps": 800' in everything[2] and "selected_steps" not in own[2]
