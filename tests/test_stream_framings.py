"""Streaming detection and the scans across front-end framings (tests/stream_framings.py): hop == window, hop > window with a
positive, zero and negative tail, hop % 4 == 2, remainders, every window of both FFT sizes, k in {1, T - 1, T}, 64 log-mel coefficients
and one MFCC.  Every accepted row: pushes, scans, many-step and ragged pushes against the offline front-end + frozen forward and
against each other, bitwise (the final logits within Cm.LOGIT_TOL of the float64 oracle); the state's zero window untouched by a
ring that wraps; the size queries.  Odd clip lengths are refused with their cause.
Emulator (`-m "not gpu"`, 3 streams) and MI355X (`-m gpu`, 96 streams)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from tests import common as Cm
from tests import stream_framings as F
from tests import test_scan as TSc
from tests import test_scan_ragged as TSR
from tests import test_scan_steps as TSteps
from tests import test_stream_scan as TSS
from tests import test_stream_scan_ragged as TSSR
from tests import test_streaming as TSt

NFFT = {320: 512, 480: 512, 512: 512, 640: 1024, 960: 1024, 1024: 1024}
CHUNKS = [1, 4, 7, 2]                   # push_many's chunks: 14 steps
RING = 3                                # the detector's averaging ring, in steps


def build(lib, row, seed=0):
    """Front-end and TCResNet8-1.0 of a row; the row's (T, remainder, tail) are what the front-end's numbers give."""
    fe = Cm.make_frontend(lib, row.win, row.hop, num_mfccs=row.num_mfccs, method=row.method, sample_rate=row.sample_rate,
                          clip_ms=row.clip_ms, lower_hz=row.lower_hz, upper_hz=row.upper_hz)
    cfg = fe.cfg
    assert (cfg.win, cfg.hop, cfg.nfft) == (row.win, row.hop, NFFT[row.win]), row.name
    assert fe.n_samples == int(row.sample_rate * row.clip_ms / 1000) and fe.n_samples % 2 == 0, row.name
    assert F.geometry(fe.n_samples, row.win, row.hop) == (row.T, row.remainder, row.tail), (row.name, F.geometry(fe.n_samples, row.win, row.hop))
    assert fe.n_frames == row.T and 1 <= row.k <= row.T, row.name
    assert fe.n_coef == (64 if row.method == F.LOG_MEL else row.num_mfccs), row.name
    arch = R.make_tcresnet("TCResNet8", 1.0, in_channels=fe.n_coef)
    p, s = R.init_params(arch, seed)
    R.randomize_bn(arch, p, s, seed + 1)
    return fe, Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef), arch, p, s


def det_for(row):
    """Detector settings in the row's steps: a ring of RING vectors, suppression over four steps, every warm step a candidate."""
    step_ms = 1000.0 * row.k * row.hop / row.sample_rate
    return dict(average_window_ms=RING * step_ms, min_count=2, detection_threshold=0.0, suppression_ms=4 * step_ms)


def state_layout(fe, net, S, W, tail):
    """stream.hip's StreamGeom restated, in floats: {region: (offset, floats)} and the total.  A negative tail keeps no samples."""
    tp = T._lib.padded_len(fe.n_frames)
    out, o = {}, 0
    for key, n in (("window", S * fe.n_coef * tp), ("zero_window", fe.n_coef * tp), ("tail", S * max(tail, 0)),
                   ("ring", W * S * net.num_classes), ("integers", 5 * S)):
        out[key] = (o, n)
        o = TSS.align64(o + n)
    return out, o


def check_sizes(lib, fe, net, row):
    """The C size queries: the state is the restated layout's bytes, and state and workspace never shrink as streams are added (a
    region of negative size would make them); the scan workspace, which has no stream count, over its max_windows."""
    det = T._lib.DetectCfg(RING, 2, 4, 0.0)
    counts = (1, 2, 3, 4, 96)                             # (4 x 20 samples: the smallest negative tail passes an alignment unit of 64)
    state = [lib.tcr_stream_state_bytes(C.byref(fe.cfg), net._h, S, row.k, C.byref(det)) for S in counts]
    assert state == [4 * state_layout(fe, net, S, RING, row.tail)[1] for S in counts], (row.name, state, lib.tcr_last_error())
    ws = [lib.tcr_stream_workspace_bytes(C.byref(fe.cfg), net._h, S, row.k) for S in counts]
    scan = [lib.tcr_scan_workspace_bytes(C.byref(fe.cfg), net._h, row.k, m) for m in counts]
    for sizes in (state, ws, scan):
        assert sizes[0] > 0 and sizes == sorted(sizes), (row.name, state, ws, scan, lib.tcr_last_error())
    need = 4 * ((row.k - 1) * row.hop + row.win)          # a staging row holds the k new frames
    assert ws[0] >= need and scan[0] >= 4 * ((row.T - 1) * row.hop + row.win), (row.name, ws, scan)


def check_scan_is_offline(lib, fe, net, x, k, out):
    """Steps 0, the middle one and the last of a scan against their definition, not against the pushes (both derive their geometry
    from stream.hip's): step j's window is the offline front-end of the last n_samples of  zeros(n_samples) ++ signal[: (j + 1) k hop]."""
    n, khop, steps = fe.n_samples, k * fe.cfg.hop, out.logits.shape[1]
    assert steps == x.shape[1] // khop and steps >= 3
    ss = net.fold_bn()
    zeros = torch.zeros((x.shape[0], n), dtype=torch.float32, device=x.device)
    for j in (0, steps // 2, steps - 1):
        clip = torch.cat([zeros, x[:, :(j + 1) * khop]], dim=1)[:, -n:].contiguous()
        lo, pr = net.forward_frozen(fe(clip), ss)
        assert torch.equal(out.logits[:, j], lo), (j, int((out.logits[:, j] != lo).sum()))
        assert torch.equal(out.probs[:, j], pr), j


def bits(t):
    return t.view(torch.int32)


def check_state_guard(lib, fe, net, row, S):
    """The state's zero window -- the region in front of the tail -- is the offline features of a silent clip and keeps every byte
    while the detector's ring wraps; a reset after that gives the window of  zeros ++ new samples."""
    from tcresnet_amd import streaming as St
    det = St.StreamingDetector(net, fe, S, frames_per_step=row.k, **det_for(row))
    assert det.average_steps == RING
    layout, total = state_layout(fe, net, S, RING, row.tail)
    assert det.state.numel() == total, (row.name, det.state.numel(), total)
    o, n = layout["zero_window"]
    before = det.state[o:o + n].clone()
    silent = fe(torch.zeros((1, fe.n_samples), dtype=torch.float32, device=det.state.device))
    assert torch.equal(bits(before), bits(silent.reshape(-1))), row.name
    ss = net.fold_bn()
    clips = TSt.Clips(lib, S, fe.n_samples)
    rng = np.random.RandomState(17)
    for i in range(RING + 3):                             # the ring wraps, and a reset on the last step
        x = Cm.to_dev(lib, rng.uniform(-0.5, 0.5, (S, row.k * row.hop)))
        idx = list(range(0, S, 2)) if i == RING + 2 else ()
        if idx:
            det.reset(idx)
        out = det.push(x)
        TSt.check_step(fe, net, ss, det, clips.step(x, idx), out)
        assert torch.equal(bits(det.state[o:o + n]), bits(before)), (row.name, i)
    n_steps = TSS.state_parts(det)[3][4]                  # the streams' step counters: restarted / RING + 3 steps
    assert S > 1 and int(n_steps.min()) == 1 and int(n_steps.max()) == RING + 3


def check_row_streams(lib, row, S):
    """Sizes; pushes == offline (resets mid-run and on the last step); scan == pushes == offline; push_many == scan; the state guard."""
    fe, net, arch, p, s = build(lib, row)
    check_sizes(lib, fe, net, row)
    TSt.run_checked(lib, fe, net, arch, p, s, S, row.k, 6, {3: [1], 5: [0, S - 1]})
    det = det_for(row)
    audio = TSt.segment_audio(S, sum(CHUNKS) * row.k * row.hop, 11)
    got = TSc.check_scan_equals_stream(lib, fe, net, audio, row.k, det=det)
    check_scan_is_offline(lib, fe, net, Cm.to_dev(lib, audio), row.k, got)
    TSS.check_chunks_equal_scan(lib, fe, net, audio, row.k, CHUNKS, det, max_windows=5)
    check_state_guard(lib, fe, net, row, S)


def cycle(pattern, n):
    return [pattern[i % len(pattern)] for i in range(n)]


def check_row_ragged(lib, row, S):
    """scan_ragged == each signal's own scan (one signal of a single step, one shorter than a clip where a step is, one without
    steps); scan_steps on subsets == the ragged rows; push_ragged with streams that do not advance == one-stream oracles, their state
    byte for byte what it was."""
    fe, net, _, _, _ = build(lib, row)
    det, k, khop = det_for(row), row.k, row.k * row.hop
    short = max(1, min(5, (fe.n_samples - 1) // khop))
    steps = cycle([1, short, 7, 0, 12], max(S, 5))
    assert short * khop < fe.n_samples or khop >= fe.n_samples
    out = TSR.check_family_case(lib, fe, net, steps, k, 31, det=det, max_windows=(5,))
    # scan_steps: the selections of test_scan_steps.py at group boundaries of 5, against the default scan_ragged of the same signals
    Sc = TSR.scanning()
    signals = TSR.cut_signals(lib, TSt.segment_audio(len(steps), max(steps) * khop, 31), steps, khop)
    want = Sc.KeywordScanner(net, fe, frames_per_step=k, **det).scan_ragged(signals)
    assert all(torch.equal(a, b) for a, b in zip(want.tensors(), out.tensors()))
    sc = Sc.KeywordScanner(net, fe, frames_per_step=k, max_windows=5, **det)
    sels = TSteps.selections(steps, 5, 31)
    for name in ("ends", "bounds", "random"):
        assert len(sels[name]) > 0, name
        idx = torch.tensor(sels[name], dtype=torch.int64)
        logits, probs = sc.scan_steps(signals, idx)
        at = idx.to(want.logits.device)
        assert torch.equal(logits, want.logits[at]) and torch.equal(probs, want.probs[at]), (row.name, name)
    # push_ragged: every call leaves some streams where they are; a reset waits for its stream's next step
    rig = TSSR.Rig(lib, fe, net, S, 9, 32, k=k, det=det, many=lib.kind == "hip", max_windows=5)
    rig.ragged(cycle([3, 0, 1], S))
    rig.ragged(cycle([0, 2, 2], S), packed=True)
    rig.reset([i for i in range(S) if i % 3 != 2])
    rig.ragged(cycle([1, 0, 6], S))
    assert rig.dut._pending.tolist() == [i % 3 == 1 for i in range(S)]


def check_refusals(lib):
    """An odd clip length: the detector, the scanner and the size queries refuse, naming the clip length; init writes nothing."""
    from tcresnet_amd import scanning as Sc
    from tcresnet_amd import streaming as St
    for name, sr, clip_ms, win, hop, lo, hi, n in F.REFUSED:
        fe = Cm.make_frontend(lib, win, hop, sample_rate=sr, clip_ms=clip_ms, lower_hz=lo, upper_hz=hi)
        assert fe.n_samples == n and n % 2 == 1, name
        arch = R.make_tcresnet("TCResNet8", 1.0, in_channels=fe.n_coef)
        p, s = R.init_params(arch, 0)
        net = Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef)

        def named(msg):
            return "frontend_pk3_kernel" in msg and f"clip of {n} samples" in msg and "odd" in msg and "bitwise" in msg

        for make in (lambda: St.StreamingDetector(net, fe, 2), lambda: Sc.KeywordScanner(net, fe)):
            with pytest.raises(T.TcrError) as e:
                make()
            assert named(str(e.value)), str(e.value)
        det = T._lib.DetectCfg(RING, 2, 4, 0.5)
        for query in (lambda: lib.tcr_stream_state_bytes(C.byref(fe.cfg), net._h, 2, 1, C.byref(det)),
                      lambda: lib.tcr_stream_workspace_bytes(C.byref(fe.cfg), net._h, 2, 1),
                      lambda: lib.tcr_scan_workspace_bytes(C.byref(fe.cfg), net._h, 1, 16)):
            assert query() == 0 and named(lib.tcr_last_error().decode()), (name, lib.tcr_last_error())
        buf = torch.full((1 << 16,), 7.0, dtype=torch.float32, device=Cm.device_of(lib))
        assert lib.tcr_stream_init(C.byref(fe.cfg), fe.plan.data_ptr(), net._h, 2, 1, C.byref(det), buf.data_ptr(), buf.data_ptr(),
                                   buf.numel() * 4, None) == -1 and named(lib.tcr_last_error().decode()), (name, lib.tcr_last_error())
        assert bool((buf == 7.0).all()), name


def test_rows_take_every_listed_case():
    """The table covers the cases by its own numbers (a row that leaves would take its case with it)."""
    rows = F.ROWS
    assert len(set(F.ROW_IDS)) == len(rows)
    for r in rows:
        n = int(r.sample_rate * r.clip_ms / 1000)
        assert F.geometry(n, r.win, r.hop) == (r.T, r.remainder, r.tail), r.name
        assert 9 <= r.T <= 33 and r.hop % 2 == 0 and n % 2 == 0 and r.win <= n, r.name
    khop = {r.name: r.k * r.hop for r in rows}
    assert sum(r.tail < 0 for r in rows) >= 3 and any(-64 < r.tail < 0 for r in rows)
    assert any(r.tail == 0 and r.hop == r.win for r in rows)
    assert any(r.tail == 0 and r.hop > r.win and r.remainder == r.hop - r.win for r in rows)
    assert any(r.tail > 0 and r.hop > r.win for r in rows)
    assert any(0 < r.tail < khop[r.name] for r in rows) and any(r.tail > khop[r.name] for r in rows)
    assert any(r.tail == khop[r.name] for r in rows) and max(r.tail for r in rows) > 1024 - 64
    assert any(r.hop % 4 == 2 for r in rows) and any(r.remainder == 0 for r in rows) and any(r.remainder for r in rows)
    assert {r.win for r in rows} == set(NFFT) and {NFFT[r.win] for r in rows} == {512, 1024}
    assert any(r.k == 1 for r in rows) and any(r.k == r.T - 1 for r in rows)
    assert any(r.k == r.T and r.hop > r.win for r in rows) and any(r.k == r.T and r.tail < 0 for r in rows)
    assert any(r.method == F.LOG_MEL and r.win in (960, 1024) for r in rows) and any(r.num_mfccs == 1 for r in rows)
    assert {r.sample_rate for r in rows} >= {16000, 32000}
    assert all(n % 2 == 1 for *_, n in F.REFUSED) and len({r[1] for r in F.REFUSED}) == 2


# ---- emulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.ROW_IDS)
def test_framing_row_streams(emu_lib, name):
    check_row_streams(emu_lib, F.ROW[name], 3)


@pytest.mark.parametrize("name", F.ROW_IDS)
def test_framing_row_ragged(emu_lib, name):
    check_row_ragged(emu_lib, F.ROW[name], 3)


def test_stream_refuses_odd_clips(emu_lib):
    check_refusals(emu_lib)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", F.ROW_IDS)
def test_gpu_framing_row_streams(hip_lib, name):
    check_row_streams(hip_lib, F.ROW[name], 96)


@pytest.mark.gpu
@pytest.mark.parametrize("name", F.ROW_IDS)
def test_gpu_framing_row_ragged(hip_lib, name):
    check_row_ragged(hip_lib, F.ROW[name], 96)


@pytest.mark.gpu
def test_gpu_stream_refuses_odd_clips(hip_lib):
    check_refusals(hip_lib)
