"""Detection sweeps (tcr_detect_sweep, scanning.KeywordScanner.sweep / detection_sweep, sweep_audio.py): for every threshold the steps
that fire are the scan's is_new at that threshold, bitwise, and the hit / duplicate / false-accept counts follow the documented
scoring (a NumPy restatement below).  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import csv
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import DET, scanning
from tests.test_streaming import frozen_artifact, segment_audio, setup, write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS = 2048                     # sweep.hip's kSweepPass


# ---- the rule and the scoring, restated -----------------------------------------------------------------------------------------
def naive_sweep(top, score, thr, supp, ncls, valid=None, events=None):
    """Step by step, as include/tcresnet_hip.h states it."""
    N, steps = top.shape
    thr = np.asarray(thr, np.float32)
    T_ = len(thr)
    det, hits, dups = (np.zeros((N, T_, ncls), np.int64) for _ in range(3))
    fired = np.zeros((T_, N, steps), np.uint8)
    for n in range(N):
        vs = steps if valid is None else int(valid[n])
        evs = [] if events is None else events[n]
        for t in range(T_):
            prev, pstep, last_hit = -1, 0, -1
            for i in range(vs):
                c = int(top[n, i])
                if not (0 <= c < ncls and score[n, i] > thr[t] and c != prev and (prev == -1 or i - pstep > supp)):
                    continue
                prev, pstep = c, i
                fired[t, n, i] = 1
                det[n, t, c] += 1
                for j, (f, l, lab) in enumerate(evs):
                    if f <= i <= l and lab == c:
                        if j == last_hit:
                            dups[n, t, c] += 1
                        else:
                            hits[n, t, c] += 1
                            last_hit = j
    return det, hits, dups, fired


def fast_sweep(top, score, thr, supp, ncls, valid=None, events=None, want_fired=True):
    """The same walk over the candidate steps only, jumping past suppressed steps and runs of one label (for long signals)."""
    N, steps = top.shape
    thr = np.asarray(thr, np.float32)
    T_ = len(thr)
    det, hits, dups = (np.zeros((N, T_, ncls), np.int64) for _ in range(3))
    fired = np.zeros((T_, N, steps), np.uint8) if want_fired else None
    for n in range(N):
        vs = steps if valid is None else int(valid[n])
        tp, sc = top[n, :vs].astype(np.int64), score[n, :vs]
        ok = (tp >= 0) & (tp < ncls)
        evs = [] if events is None else events[n]
        ef = np.array([e[0] for e in evs], np.int64)
        el = np.array([e[1] for e in evs], np.int64)
        ec = np.array([e[2] for e in evs], np.int64)
        for t in range(T_):
            idx = np.flatnonzero(ok & (sc > thr[t]))
            if idx.size == 0:
                continue
            lab = tp[idx]
            change = np.flatnonzero(np.diff(lab) != 0) + 1                   # run starts after the first
            run_end = np.append(change, idx.size)[np.searchsorted(change, np.arange(idx.size), side="right")]
            prev, pstep, last_hit, pos = -1, 0, -1, 0
            while pos < idx.size:
                if prev != -1:
                    lo = np.searchsorted(idx, pstep + supp + 1)
                    if lo > pos:
                        pos = lo
                    if pos >= idx.size:
                        break
                    if lab[pos] == prev:
                        pos = run_end[pos]
                        continue
                i, c = int(idx[pos]), int(lab[pos])
                prev, pstep = c, i
                if fired is not None:
                    fired[t, n, i] = 1
                det[n, t, c] += 1
                j = int(np.searchsorted(ef, i, side="right")) - 1
                if j >= 0 and el[j] >= i and ec[j] == c:
                    if j == last_hit:
                        dups[n, t, c] += 1
                    else:
                        hits[n, t, c] += 1
                        last_hit = j
                pos += 1
    return det, hits, dups, fired


def check_result(res, ref, fired=True):
    det, hits, dups, rf = ref
    assert np.array_equal(res.detections.cpu().numpy(), det)
    assert np.array_equal(res.hits.cpu().numpy(), hits)
    assert np.array_equal(res.duplicates.cpu().numpy(), dups)
    assert np.array_equal(res.false_accepts().cpu().numpy(), det - hits - dups)
    if fired:
        assert np.array_equal(res.fired.cpu().numpy(), rf)


def synthetic(N, steps, ncls, seed):
    """top / score with runs of one label, alternating labels and top = -1 stretches; scores on a coarse grid (many ties)."""
    rng = np.random.RandomState(seed)
    top = np.empty((N, steps), np.int32)
    for n in range(N):
        pos = 0
        while pos < steps:
            m = min(int(rng.randint(1, 400)), steps - pos)
            kind = rng.randint(4)
            if kind == 0:
                top[n, pos:pos + m] = -1
            elif kind == 1:
                top[n, pos:pos + m] = rng.randint(ncls)
            elif kind == 2:
                a, b = rng.randint(ncls, size=2)
                top[n, pos:pos + m] = np.where(np.arange(m) % 2 == 0, a, b)
            else:
                top[n, pos:pos + m] = rng.randint(ncls, size=m)
            pos += m
    score = (rng.randint(0, 64, size=(N, steps)) / 64.0).astype(np.float32)
    score[top == -1] = 0.0
    return top, score


def random_events(steps, ncls, rng, n_events):
    """Disjoint sorted inclusive step ranges with mixed labels (some past the valid steps)."""
    cuts = np.sort(rng.choice(np.arange(1, steps), size=2 * n_events, replace=False))
    return [(int(cuts[2 * j]), int(cuts[2 * j + 1]) - (j % 3 == 0), int(rng.randint(ncls))) for j in range(n_events)]


def sweep_lib(lib, top, score, thr, supp, ncls, **kw):
    Sc = scanning()
    dev = Cm.device_of(lib)
    return Sc.detection_sweep(torch.from_numpy(top).to(dev), torch.from_numpy(score).to(dev), thr, supp, ncls, lib=lib, **kw)


# ---- emulator -------------------------------------------------------------------------------------------------------------------
def test_reference_walks_agree():
    top, score = synthetic(2, 3000, 5, 7)
    rng = np.random.RandomState(8)
    ev = [random_events(3000, 5, rng, 40) for _ in range(2)]
    thr = [-np.inf, 0.0, 0.25, 0.5, 0.984375, np.inf]
    for supp in (0, 7, 500):
        a = naive_sweep(top, score, thr, supp, 5, [3000, 1234], ev)
        b = fast_sweep(top, score, thr, supp, 5, [3000, 1234], ev)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("supp", [0, 7, 500])
def test_sweep_direct_equals_reference(emu_lib, supp):
    N, steps, ncls = 3, 20000, 5
    top, score = synthetic(N, steps, ncls, 11 + supp)
    rng = np.random.RandomState(supp)
    events = [random_events(steps, ncls, rng, 60) for _ in range(N)]
    present = np.unique(score[top >= 0])
    thr = [-np.inf, float(present[0]), 0.25, float(present[len(present) // 2]), float(present[-2]), float(present[-1]), np.inf, 0.3]
    valid = [steps, PASS, 8191]
    res = sweep_lib(emu_lib, top, score, thr, supp, ncls, events=events, valid_steps=valid, step_seconds=0.02, return_fired=True)
    ref = fast_sweep(top, score, thr, supp, ncls, valid, events)
    check_result(res, ref)
    assert res.detections.shape == (N, len(thr), ncls) and res.fired.shape == (len(thr), N, steps)
    det = ref[0].sum(axis=(0, 2))
    assert det[0] > 0 and det[5] == 0 and det[6] == 0           # -inf fires, the largest score present and +inf never do
    assert ref[1].sum() > 0 and (ref[2].sum() > 0 or supp == 500) and (ref[0] - ref[1] - ref[2]).sum() > 0
    assert np.allclose(res.hours, np.array(valid) * 0.02 / 3600)
    assert np.array_equal(res.events, np.stack([np.bincount([e[2] for e in evs], minlength=ncls) for evs in events]))


def test_sweep_valid_steps_edges(emu_lib):
    N, steps, ncls = 8, 2 * PASS + 300, 4
    top, score = synthetic(N, steps, ncls, 3)
    valid = [0, 1, PASS - 1, PASS, PASS + 1, 2 * PASS, steps - 1, steps]
    thr = [0.0, 0.5]
    rng = np.random.RandomState(4)
    events = [random_events(steps, ncls, rng, 30) for _ in range(N)]
    res = sweep_lib(emu_lib, top, score, thr, 3, ncls, events=events, valid_steps=valid, return_fired=True)
    check_result(res, naive_sweep(top, score, thr, 3, ncls, valid, events))
    assert int(res.detections[0].sum()) == 0
    # no events: hits / duplicates zero, the detections the same; past-T rows of the last block untouched
    res2 = sweep_lib(emu_lib, top, score, thr, 3, ncls, valid_steps=valid)
    assert torch.equal(res2.detections, res.detections) and int(res2.hits.sum()) == 0 and res2.fired is None
    assert np.isnan(res2.hours).all()


def test_sweep_many_thresholds_and_classes(emu_lib):
    """T = 37 (three workgroups of thresholds, the last one partial), 200 classes (counters past 64 KB of LDS with the staging)."""
    top, score = synthetic(1, 5000, 200, 5)
    thr = np.linspace(-0.1, 1.0, 37)
    rng = np.random.RandomState(6)
    events = [random_events(5000, 200, rng, 50)]
    res = sweep_lib(emu_lib, top, score, thr, 2, 200, events=events, return_fired=True)
    check_result(res, fast_sweep(top, score, thr, 2, 200, None, events))


def check_scan_sweep(lib, fe, net, audio, k, det, thresholds):
    """fired[t] of a sweep over one scan == is_new of a scanner built with detection_threshold = thresholds[t], bitwise."""
    Sc = scanning()
    x = Cm.to_dev(lib, audio)
    sc = Sc.KeywordScanner(net, fe, frames_per_step=k, **det)
    out = sc.scan(x)
    res = sc.sweep(out, thresholds, return_fired=True)
    for t, th in enumerate(thresholds):
        want = Sc.KeywordScanner(net, fe, frames_per_step=k, **dict(det, detection_threshold=th)).scan(x).is_new
        assert torch.equal(res.fired[t].to(torch.int32), want), (th, int((res.fired[t].to(torch.int32) != want).sum()))
        assert torch.equal(res.detections[:, t].sum(dim=1), want.sum(dim=1).to(torch.int32))
    return out, res


@pytest.mark.parametrize("k", [1, 3])
def test_sweep_equals_scans_4020(emu_lib, k):
    fe, net, _, _, _ = setup(emu_lib)
    out, res = check_scan_sweep(emu_lib, fe, net, segment_audio(2, 20160, 3), k, DET, [0.0, 0.3, 0.6])
    assert int(res.fired[0].sum()) >= 1


def test_scanner_sweep_events_in_ms(emu_lib):
    """ms -> inclusive step ranges (t_i = 1000 (i + 1) step / sr, start <= t_i <= end + tolerance), lengths in samples."""
    Sc = scanning()
    fe, net, _, _, _ = setup(emu_lib)
    sc = Sc.KeywordScanner(net, fe, **DET)                          # 20 ms steps
    N, steps, ncls = 2, 3000, 12
    top, score = synthetic(N, steps, ncls, 9)
    out = Sc.ScanOutput(None, None, None, torch.from_numpy(top), torch.from_numpy(score), None)
    labels = [f"c{i}" for i in range(ncls)]
    events = [[(100.0, 140.0, "c1"), (1000.0, 1999.0, 3), (5010.5, 5010.5, "c2")], [(40.0, 59.9, 4)]]
    res = sc.sweep(out, [0.0, 0.5], events=events, lengths=[steps * 320, 2000 * 320 + 319], tolerance_ms=20.0, labels=labels,
                   return_fired=True)
    steps_ev = [[(4, 7, 1), (49, 99, 3), (250, 250, 2)], [(1, 2, 4)]]      # step i ends at 20 (i + 1) ms
    check_result(res, naive_sweep(top, score, [0.0, 0.5], sc.suppression_steps, ncls, [steps, 2000], steps_ev))
    assert np.allclose(res.hours, np.array([steps, 2000]) * 0.02 / 3600)
    assert res.events[0, 1] == 1 and res.events[0, 3] == 1 and res.events.sum() == 4
    cv = res.curve()
    assert cv["events"][0] == 4 and np.array_equal(cv["hits"], res.hits.numpy().sum(axis=(0, 2)))
    assert np.allclose(cv["fa_per_hour"], res.false_accepts().numpy().sum(axis=(0, 2)) / res.hours.sum())
    op = res.operating_point(1e9)
    assert op is not None and op["fa_per_hour"] <= 1e9
    assert res.operating_point(-1.0) is None
    with pytest.raises(T.TcrError, match="signal 0: events .* overlap"):
        sc.sweep(out, [0.5], events=[[(0.0, 100.0, 1), (110.0, 200.0, 2)], []], tolerance_ms=10.0)
    with pytest.raises(T.TcrError, match="signal 1: event .* starts past"):
        sc.sweep(out, [0.5], events=[[], [(50000.0, 50100.0, 1)]], lengths=[steps * 320, 1000 * 320])
    with pytest.raises(T.TcrError, match="signal 0: event .* unknown label"):
        sc.sweep(out, [0.5], events=[[(0.0, 100.0, "nope")], []], labels=labels)
    with pytest.raises(T.TcrError, match="unknown label"):
        sc.sweep(out, [0.5], events=[[(0.0, 100.0, 12)], []])
    with pytest.raises(T.TcrError, match="NaN thresholds"):
        sc.sweep(out, [0.5, float("nan")])


def test_sweep_c_refusals(emu_lib):
    lib = emu_lib
    buf = torch.zeros(1 << 12)
    p = buf.data_ptr()

    def call(n=1, steps=16, ncls=4, top=p, supp=0, nthr=1, det=p, ev=None, hits=p):
        return lib.tcr_detect_sweep(n, steps, ncls, top, p, None, supp, nthr, p, ev, p, p, p, det, hits, p, None, None)
    assert call() == 0
    for kw, msg in [(dict(top=None), b"null argument"), (dict(det=None), b"null argument"),
                    (dict(n=0), b"number of signals must be positive"), (dict(steps=0), b"number of steps must be positive"),
                    (dict(nthr=0), b"number of thresholds must be positive"), (dict(ncls=0), b"num_classes 0 outside"),
                    (dict(ncls=257), b"num_classes 257 outside"), (dict(supp=-1), b"suppression_steps must be >= 0"),
                    (dict(ev=p, hits=None), b"events need"), (dict(n=1 << 16, steps=1 << 15), b"too large"),
                    (dict(n=1 << 12, nthr=1 << 12, ncls=200), b"too large")]:
        assert call(**kw) == -1, kw
        assert msg in lib.tcr_last_error(), (kw, lib.tcr_last_error())
    Sc = scanning()
    with pytest.raises(T.TcrError, match="tcr_detect_sweep failed .*suppression_steps"):
        Sc.detection_sweep(torch.zeros((1, 8), dtype=torch.int32), torch.zeros((1, 8)), [0.5], -1, 4, lib=lib)
    with pytest.raises(T.TcrError, match="overlap"):
        Sc.detection_sweep(torch.zeros((1, 8), dtype=torch.int32), torch.zeros((1, 8)), [0.5], 0, 4, events=[[(0, 3, 1), (3, 4, 1)]],
                           lib=lib)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
DEFAULT_DET = dict(average_window_ms=1000, min_count=3, detection_threshold=0.5, suppression_ms=1500)


def warm_quantiles(out, n):
    sc = out.score[out.top >= 0].cpu().numpy()
    return np.quantile(sc, np.linspace(0.0, 1.0, n)).astype(np.float32)


@pytest.mark.gpu
def test_gpu_sweep_8x10min_64_thresholds(hip_lib):
    Sc = scanning()
    fe, net, _, _, _ = setup(hip_lib)
    x = Cm.to_dev(hip_lib, segment_audio(8, 600 * 16000, 31))
    sc = Sc.KeywordScanner(net, fe, **DEFAULT_DET)
    out = sc.scan(x)
    thr = warm_quantiles(out, 64)
    top, score = out.top.cpu().numpy(), out.score.cpu().numpy()
    rng = np.random.RandomState(32)
    steps = top.shape[1]
    events = [random_events(steps, 12, rng, 200) for _ in range(8)]
    res = Sc.detection_sweep(out.top, out.score, thr, sc.suppression_steps, 12, events=events, step_seconds=0.02, return_fired=True,
                             lib=hip_lib)
    ref = fast_sweep(top, score, thr, sc.suppression_steps, 12, None, events)
    check_result(res, ref)
    assert ref[0].sum() > 0 and ref[1].sum() > 0
    for t in (0, 21, 42, 63):
        want = Sc.KeywordScanner(net, fe, **dict(DEFAULT_DET, detection_threshold=float(thr[t]))).scan(x).is_new
        assert torch.equal(res.fired[t].to(torch.int32), want), t


@pytest.mark.gpu
def test_gpu_sweep_1h_256_thresholds(hip_lib):
    Sc = scanning()
    fe, net, _, _, _ = setup(hip_lib)
    sc = Sc.KeywordScanner(net, fe, **DEFAULT_DET)
    out = sc.scan(Cm.to_dev(hip_lib, segment_audio(1, 3600 * 16000, 33)))
    thr = warm_quantiles(out, 256)
    top, score = out.top.cpu().numpy(), out.score.cpu().numpy()
    rng = np.random.RandomState(34)
    events = [random_events(top.shape[1], 12, rng, 1500)]
    res = Sc.detection_sweep(out.top, out.score, thr, sc.suppression_steps, 12, events=events, lib=hip_lib)
    check_result(res, fast_sweep(top, score, thr, sc.suppression_steps, 12, None, events, want_fired=False), fired=False)
    assert int(res.detections.sum()) > 0


@pytest.mark.gpu
def test_gpu_sweep_lengths_equal_truncated_scans(hip_lib):
    Sc = scanning()
    fe, net, _, _, _ = setup(hip_lib)
    audio = segment_audio(3, 120 * 16000, 35)
    lengths = [120 * 16000, 77 * 16000 + 123, 3 * 16000 + 5]
    for n, L in enumerate(lengths):
        audio[n, L:] = 0.0
    sc = Sc.KeywordScanner(net, fe, **DEFAULT_DET)
    out = sc.scan(Cm.to_dev(hip_lib, audio))
    thr = [0.0, 0.2, 0.4, 0.6]
    res = sc.sweep(out, thr, lengths=lengths, return_fired=True)
    for n, L in enumerate(lengths):
        vs = L // sc.step_samples
        cut = Cm.to_dev(hip_lib, audio[n:n + 1, :vs * sc.step_samples])
        for t, th in enumerate(thr):
            want = Sc.KeywordScanner(net, fe, **dict(DEFAULT_DET, detection_threshold=th)).scan(cut).is_new[0]
            assert torch.equal(res.fired[t, n, :vs].to(torch.int32), want), (n, th)
            assert int(res.fired[t, n, vs:].sum()) == 0
        assert abs(res.hours[n] - vs * 0.02 / 3600) < 1e-15


@pytest.mark.gpu
def test_gpu_sweep_tcresnet14_3010_log_mel(hip_lib):
    fe, net, _, _, _ = setup(hip_lib, "TCResNet14", 1.5, win=480, hop=160, method="log_mel_spectrogram")
    det = dict(average_window_ms=500, min_count=2, detection_threshold=0.3, suppression_ms=600)
    check_scan_sweep(hip_lib, fe, net, segment_audio(4, 20 * 16000, 36), 2, det, [0.0, 0.15, 0.3])


@pytest.mark.gpu
def test_gpu_sweep_audio_cli(hip_lib, tmp_path):
    Sc = scanning()
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    audio = segment_audio(2, 60 * 16000, 37)
    pcm = [np.clip(audio[0] * 32767, -32768, 32767).astype(np.int16), np.clip(audio[1, :41234 * 16] * 32767, -32768, 32767).astype(np.int16)]
    wavs = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    labels = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(10)]
    rows = [(wavs[0], 1000, 2000, "w0"), (wavs[0], 5000, 6500, "w3"), (wavs[0], 30000, 31000, "w0"), (wavs[1], 2000, 3000, "w7")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{a},{b},{c}\n" for f, a, b, c in rows))
    args = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), "--events", str(ev_csv), "--thresholds", "0:0.9:0.1",
            "--tolerance_ms", "500", "--target_fa_per_hour", "1000"]
    run = lambda *extra: subprocess.run([sys.executable, os.path.join(ROOT, "tc-resnet_amd", "sweep_audio.py"), *args, *extra],
                                        capture_output=True, text=True, timeout=600)
    r, rl = run(), run("--per_label")
    assert r.returncode == 0, r.stderr
    assert rl.returncode == 0, rl.stderr
    got = list(csv.DictReader(io.StringIO(r.stdout)))
    assert r.stdout.splitlines()[0] == "threshold,hits,events,false_accepts,duplicates,frr,fa_per_hour"
    assert rl.stdout.splitlines()[0] == "label,threshold,hits,events,false_accepts,duplicates,frr,fa_per_hour"
    # the same through the Python API
    from tcresnet_amd.deploy import FrozenModel
    sc = FrozenModel.load(path).scanner()
    host = np.zeros((2, 60 * 16000), np.float32)
    lens = []
    for n, x in enumerate(pcm):
        x = x.astype(np.float32) * (1.0 / 32768.0)
        x = x[:len(x) // sc.step_samples * sc.step_samples]
        host[n, :len(x)] = x
        lens.append(len(x))
    out = sc.scan(torch.from_numpy(host).cuda())
    ev = [[(a, b, c) for f, a, b, c in rows if f == w] for w in wavs]
    res = sc.sweep(out, np.arange(0, 0.9 + 1e-9, 0.1), events=ev, lengths=lens, tolerance_ms=500, labels=labels)
    cv = res.curve(list(range(2, 12)))
    assert len(got) == len(cv["threshold"]) == 10
    for t, row in enumerate(got):
        assert float(row["threshold"]) == pytest.approx(float(cv["threshold"][t]), abs=1e-6)
        for k in ("hits", "events", "false_accepts", "duplicates"):
            assert int(row[k]) == int(cv[k][t]), (t, k)
        assert float(row["fa_per_hour"]) == pytest.approx(float(cv["fa_per_hour"][t]), rel=1e-6)
    per = list(csv.DictReader(io.StringIO(rl.stdout)))
    assert len(per) == 10 * 10 and {p["label"] for p in per} == set(labels[2:])
    info = json.loads(r.stderr.strip().splitlines()[-1])
    assert info["hours"] == pytest.approx(sum(lens) / 16000 / 3600)
    assert "operating_point" in info and info["operating_point"] == res.operating_point(1000, list(range(2, 12)))
