"""Streaming cascades (tcr_stream_select, tcr_stream_step_selected_m, streaming.StreamingCascade, stream_audio.py's cascade flags).  The
reference of every bitwise check is the existing code: the causal cascade scan `CascadeScanner(..., pad_before_ms=0)` of the whole signals,
a plain `StreamingDetector`'s pushes, `redetect` of the first scan; the `since` rule is restated in NumPy below.  Emulator (`-m "not
gpu"`) and MI355X (`-m gpu`)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_cascade import assert_fields, case, cli_models
from tests.test_net_configs import Log, kernel_of
from tests.test_scan import DET
from tests.test_scan_ragged import FIELDS, cli_files, run_all, scanning
from tests.test_scan_steps import select_reference
from tests.test_stream_scan import assert_same_state, state_parts
from tests.test_streaming import segment_audio, setup, streaming

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = np.iinfo(np.int32).max
KEYWORDS = list(range(2, 12))


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def detectors(c, S):
    """Two fresh StreamingDetectors over the models and settings of a case's scanners."""
    St = streaming()
    return tuple(St.StreamingDetector(sc.net, sc.frontend, S, frames_per_step=sc.k, **DET) for sc in (c["first"], c["second"]))


def run_cascade(cascade, x, resets=None, each=None):
    """The cascade fed x [S, L] a step at a time: its outputs stacked [S, steps, ...] and its masks [S, steps]; `selected` and
    `n_selected` are checked against the mask at every step.  resets: {step: streams}; each(i): called after push i."""
    step = cascade.step_samples
    steps = x.shape[1] // step
    fields, masks = [[] for _ in FIELDS], []
    for i in range(steps):
        if resets and i in resets:
            cascade.reset(resets[i])
        out = cascade.push(x[:, i * step:(i + 1) * step].contiguous())
        for dst, t in zip(fields, out):
            dst.append(t.clone())
        m = cascade.mask.cpu().numpy().copy()
        assert cascade.selected.dtype == torch.int64 and cascade.selected.cpu().numpy().tolist() == np.flatnonzero(m).tolist(), i
        assert cascade.n_selected == int(m.sum()) and cascade.first_out is cascade.first.out
        masks.append(m)
        if each is not None:
            each(i, out)
    return SimpleNamespace(mask=np.stack(masks, axis=1), **{f: torch.stack(v, dim=1) for f, v in zip(FIELDS, fields)})


def first_values(out1, on, S):
    """The first stage's `on` rows [S x steps, C] (NumPy), their keyword peak and a ragged scan's offsets as a dense one's."""
    v = getattr(out1, on).reshape(-1, getattr(out1, on).shape[-1]).cpu().numpy()
    return v, v[:, 2:].max(axis=1), np.arange(S + 1, dtype=np.int64) * (v.shape[0] // S)


def reference(first, second, out1, x, enter, pad_after_ms, on="probs"):
    """The causal cascade scan of x [S, L], the selection mask [S, steps] and the flags [S, steps] from the first stage's scan."""
    Sc = scanning()
    S = int(x.shape[0])
    cas = Sc.CascadeScanner(first, second, enter, pad_before_ms=0, pad_after_ms=pad_after_ms, on=on)
    v, _, offsets = first_values(out1, on, S)
    _, mask = select_reference(v, offsets, enter, KEYWORDS, 0, cas.pad_after)
    with np.errstate(invalid="ignore"):
        flag = (v[:, 2:] >= np.float32(enter)).any(axis=1)
    return cas.scan(x), mask.reshape(S, -1).astype(bool), flag.reshape(S, -1), cas.pad_after


def assert_four_conditions(mask, flag):
    """Steps with no stream, some streams and all streams selected, and a stream selected while not flagged (held)."""
    S, per_step = mask.shape[0], mask.sum(axis=0)
    stats = dict(selected=int(mask.sum()), held=int((mask & ~flag).sum()), partial=int(((per_step > 0) & (per_step < S)).sum()),
                 empty=int((per_step == 0).sum()), full=int((per_step == S).sum()))
    print("selection:", stats)
    assert stats["held"] > 0 and stats["partial"] > 0 and stats["empty"] > 0 and stats["full"] > 0, stats
    return stats


def check_equals_causal_scan(lib, c, quantile, pad_after_ms, on="probs"):
    S = len(c["signals"])
    x = torch.stack(c["signals"])
    _, peak, _ = first_values(c["out1"], on, S)
    enter = float(np.quantile(peak, quantile))
    ref, mask, flag, pad_after = reference(c["first"], c["second"], c["out1"], x, enter, pad_after_ms, on)
    stats = assert_four_conditions(mask, flag)
    St = streaming()
    cascade = St.StreamingCascade(*detectors(c, S), enter, pad_after_ms=pad_after_ms, on=on)
    assert (cascade.pad_before, cascade.pad_after) == (0, pad_after)
    got = run_cascade(cascade, x)
    assert np.array_equal(got.mask, mask), int((got.mask != mask).sum())
    assert_fields(got, ref)
    return stats


def graph_case(lib, S, steps, seed):
    """A TCResNet8 first stage and a 2-D graph (tiny_conv) second stage, both 40 / 20 ms at k = 1, as a `case` dictionary."""
    from tests.test_detect_families import MODELS
    Sc = scanning()
    fe1, net1, _, _, _ = setup(lib)
    fe2, net2 = MODELS["tiny_conv"](lib)
    first, second = Sc.KeywordScanner(net1, fe1, **DET), Sc.KeywordScanner(net2, fe2, **DET)
    assert first.step_samples == second.step_samples == 320
    signals = [Cm.to_dev(lib, a) for a in segment_audio(S, steps * 320, seed)]
    return dict(first=first, second=second, signals=signals, out1=first.scan_ragged(signals))


def bytes_dev(lib, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(Cm.device_of(lib))


# ---- 1. the selection alone -----------------------------------------------------------------------------------------------------
def since_reference(values, cmask, enter, pad_after, resets):
    """The rule, stated directly: values [steps, S, C]; per step the mask [S] and `since` [S]."""
    steps, S, _ = values.shape
    since = np.full(S, NEVER, np.int64)
    masks, sinces = [], []
    for i in range(steps):
        if i in resets:
            since[resets[i]] = NEVER
        with np.errstate(invalid="ignore"):
            flag = (values[i][:, cmask.astype(bool)] >= np.float32(enter)).any(axis=1)
        since = np.where(flag, 0, np.where(since == NEVER, NEVER, np.minimum(since + 1, NEVER)))
        masks.append(((since != NEVER) & (since <= pad_after)).astype(np.uint8))
        sinces.append(since.astype(np.int32))
    return masks, sinces


def check_select(lib, S, ncls, enter, pad_after, seed):
    rng = np.random.RandomState(seed)
    steps = 12
    values = rng.uniform(0, 1, (steps, S, ncls)).astype(np.float32)
    values[rng.uniform(size=values.shape) < 0.05] = np.nan
    cmask = (rng.uniform(size=ncls) < 0.5).astype(np.uint8)
    cmask[[0, ncls - 1]] = (0, 1)
    dead = rng.choice(S, S // 10, replace=False)                 # streams whose masked values are all NaN at every step
    values[:, dead[:, None], np.flatnonzero(cmask)[None, :]] = np.nan
    values[3:8, S // 2:, :] = np.where(np.isnan(values[3:8, S // 2:, :]), np.nan, 0.0)      # a run without flags at finite thresholds
    resets = {6: np.sort(rng.choice(S, S // 3, replace=False))}
    want_masks, want_since = since_reference(values, cmask, enter, pad_after, resets)
    dev = Cm.device_of(lib)
    since = torch.empty(S, dtype=torch.int32, device=dev)
    selected = torch.full((S,), -7, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    mask = torch.empty(S, dtype=torch.uint8, device=dev)
    cm = bytes_dev(lib, cmask)
    nws = lib.tcr_stream_select_workspace_bytes(S)
    assert nws > 0
    ws = torch.empty(nws // 4, dtype=torch.int32, device=dev)
    lib.check(lib.tcr_stream_select_init(S, since.data_ptr(), None))
    assert (since.cpu().numpy() == NEVER).all()
    total = 0
    for i in range(steps):
        v = Cm.to_dev(lib, values[i])
        rst = None
        if i in resets:
            r = np.zeros(S, np.uint8)
            r[resets[i]] = 1
            rst = bytes_dev(lib, r)
        lib.check(lib.tcr_stream_select(S, ncls, v.data_ptr(), cm.data_ptr(), enter, pad_after, None if rst is None else rst.data_ptr(),
                                        since.data_ptr(), ws.data_ptr(), nws, selected.data_ptr(), count.data_ptr(), mask.data_ptr(), None),
                  "tcr_stream_select")
        n = int(count.item())
        assert np.array_equal(mask.cpu().numpy(), want_masks[i]), (i, enter, pad_after)
        assert n == int(want_masks[i].sum()) and selected[:n].cpu().numpy().tolist() == np.flatnonzero(want_masks[i]).tolist(), i
        assert np.array_equal(since.cpu().numpy(), want_since[i]), i
        total += n
    return total, want_masks, dead


@pytest.mark.parametrize("ncls", [12, 200])
def test_stream_select_equals_the_since_rule(emu_lib, ncls):
    S = 2500                                                    # crosses the 1024-stream compaction tile twice
    for pad_after in (0, 3):
        total, masks, _ = check_select(emu_lib, S, ncls, 0.93 if ncls == 12 else 0.995, pad_after, 5 + ncls)
        assert 0 < total < 12 * S
        assert any(0 < int(m[S // 2:].sum()) < S - S // 2 for m in masks[3:8]) or pad_after == 0
    total, masks, dead = check_select(emu_lib, S, ncls, float("-inf"), 0, 7)
    alive = np.ones(S, bool)
    alive[dead] = False
    assert all(np.array_equal(m.astype(bool), alive) for m in masks) and total == 12 * (S - len(dead))
    total, _, _ = check_select(emu_lib, S, ncls, float("inf"), 3, 8)
    assert total == 0


# ---- 2. bitwise the causal cascade scan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,on,pad_after_ms,counts", [("tc8_tc14", "probs", 40, (45, 13, 17, 20, 3)), ("tc8_tc14", "smoothed", 80, (40, 8, 15, 22, 3)),
                                                          ("tc8_3010_k2_dscnn_s", "probs", 40, (35, 3, 4, 29, 7))])
def test_stream_cascade_equals_causal_scan(emu_lib, pair, on, pad_after_ms, counts):
    """enter = the 80th percentile of the first stage's keyword peak.  counts: what the existing scanners select on these inputs
    (selected of 160, held, partial / empty / full steps), so that a change of the inputs shows here and not as a weaker check."""
    stats = check_equals_causal_scan(emu_lib, case(emu_lib, pair, [40] * 4, 31), 0.8, pad_after_ms, on)
    assert tuple(stats[k] for k in ("selected", "held", "partial", "empty", "full")) == counts, stats


# ---- 3. everything and nothing --------------------------------------------------------------------------------------------------
def full_state(det):
    """Every region of the state the library defines, whole (the ring with all its slots)."""
    return [t.clone() for t in state_parts(det)]


def check_everything_selected(lib, c):
    St = streaming()
    S = len(c["signals"])
    x = torch.stack(c["signals"])
    cascade = St.StreamingCascade(*detectors(c, S), float("-inf"))
    plain = detectors(c, S)[1]

    def each(i, out):
        want = plain.push(x[:, i * 320:(i + 1) * 320].contiguous())
        for f, g, w in zip(FIELDS, out, want):
            assert torch.equal(g, w), (i, f)
        for g, w in zip(full_state(cascade.second), full_state(plain)):
            assert torch.equal(g, w), i
        assert cascade.n_selected == S

    run_cascade(cascade, x, each=each)


def check_nothing_selected(lib, c):
    St = streaming()
    S = len(c["signals"])
    x = torch.stack(c["signals"])
    cascade = St.StreamingCascade(*detectors(c, S), float("inf"))
    plain = detectors(c, S)[1]
    logs = []

    def each(i, out):
        xi = x[:, i * 320:(i + 1) * 320].contiguous()
        if i == 3:
            with Log(lib) as g:
                plain.push(xi)
            logs.append(g)
        else:
            plain.push(xi)
        assert torch.equal(cascade.second.window(), plain.window()), i
        assert cascade.n_selected == 0

    got = run_cascade(cascade, x, each=each)
    want = c["second"].redetect(c["out1"])
    for f in FIELDS:
        assert torch.equal(getattr(got, f).reshape(getattr(want, f).shape), getattr(want, f)), f
    if lib.kind == "emu":       # a cascade push launches none of the kernels a plain push launches only because of its network
        shared = {"stream_stage_kernel", "frontend_pk3_kernel", "stream_detect_kernel"}
        network = {kernel_of(e) for e in logs[0].entries} - shared
        assert network and shared <= {kernel_of(e) for e in logs[0].entries}, logs[0].entries
        with Log(lib) as g:
            cascade.push(x[:, :320].contiguous())
        names = {kernel_of(e) for e in g.entries}
        assert not names & network and "stream_gather_kernel" not in names, names
        assert {"stream_flag_kernel", "select_compact_kernel", "stream_merge_kernel", "stream_detect_kernel"} <= names, names


@pytest.mark.parametrize("pair", ["tc8_tc14", "tc8_3010_k2_dscnn_s"])
def test_stream_cascade_everything_and_nothing_selected(emu_lib, pair):
    c = case(emu_lib, pair, [40] * 4, 31)
    check_everything_selected(emu_lib, c)
    check_nothing_selected(emu_lib, c)


# ---- 4. mixing ------------------------------------------------------------------------------------------------------------------
def test_push_selected_mixes_with_push_and_push_many(emu_lib):
    c = case(emu_lib, "tc8_tc14", [40] * 4, 31)
    S = 4
    x = torch.stack(c["signals"])
    dut, plain = detectors(c, S)[1], detectors(c, S)[1]
    everyone = torch.arange(S, dtype=torch.int64, device=x.device)
    i = 0
    for kind, m in [("selected", 1), ("push", 1), ("selected", 1), ("many", 7), ("selected", 1), ("selected", 1), ("many", 3), ("push", 1),
                    ("selected", 1)]:
        xs = x[:, i * 320:(i + m) * 320].contiguous()
        want = [[t.clone() for t in plain.push(xs[:, j * 320:(j + 1) * 320].contiguous())] for j in range(m)]
        if kind == "many":
            got = dut.push_many(xs)
            for j in range(m):
                for f, g, w in zip(FIELDS, got, want[j]):
                    assert torch.equal(g[:, j], w), (i, j, f)
        else:
            got = dut.push_selected(xs, everyone, S, None, None) if kind == "selected" else dut.push(xs)
            for f, g, w in zip(FIELDS, got, want[0]):
                assert torch.equal(g, w), (i, kind, f)
        assert_same_state(dut, plain)
        i += m


# ---- 5. reset -------------------------------------------------------------------------------------------------------------------
def test_stream_cascade_reset(emu_lib):
    c = case(emu_lib, "tc8_tc14", [40] * 4, 31)
    S = 4
    x = torch.stack(c["signals"])
    _, peak, _ = first_values(c["out1"], "probs", S)
    enter = float(np.quantile(peak, 0.8))
    ref, mask, flag, _ = reference(c["first"], c["second"], c["out1"], x, enter, 40)
    held = np.argwhere((mask & ~flag).T)                        # [step, stream], by step
    assert len(held)
    i0, s0 = int(held[0][0]), int(held[0][1])
    assert i0 > 0
    Sc, St = scanning(), streaming()
    rest = x[s0:s0 + 1, i0 * 320:].contiguous()
    first_rest = c["first"].scan_ragged([rest[0]])
    ref_rest, mask_rest, _, _ = reference(c["first"], c["second"], first_rest, rest, enter, 40)
    assert not mask_rest[0, 0]                                  # (held, so not flagged: a fresh stream is not selected there)
    cascade = St.StreamingCascade(*detectors(c, S), enter, pad_after_ms=40)
    got = run_cascade(cascade, x, resets={i0: [s0]})
    others = [s for s in range(S) if s != s0]
    assert not got.mask[s0, i0]
    assert np.array_equal(got.mask[s0, i0:], mask_rest[0]) and np.array_equal(got.mask[s0, :i0], mask[s0, :i0])
    assert np.array_equal(got.mask[others], mask[others])
    for f in FIELDS:
        g, w = getattr(got, f), getattr(ref, f)
        assert torch.equal(g[others], w[others]), f
        assert torch.equal(g[s0, :i0], w[s0, :i0]), f
        assert torch.equal(g[s0, i0:], getattr(ref_rest, f)[0]), f


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_stream_cascade_refusals(emu_lib):
    St = streaming()
    lib = emu_lib
    fe, net, _, _, _ = setup(lib)
    a = St.StreamingDetector(net, fe, 3, **DET)
    with pytest.raises(T.TcrError, match="steps differ \\(320 and 640 samples\\)"):
        St.StreamingCascade(a, St.StreamingDetector(net, fe, 3, frames_per_step=2, **DET), 0.5)
    fe10 = Cm.make_frontend(lib, 640, 320, num_mfccs=10)
    few = T.DSCNN("S", fe10.n_frames, fe10.n_coef, 10, lib=lib, device=Cm.device_of(lib))
    with pytest.raises(T.TcrError, match="12 and 10 classes"):
        St.StreamingCascade(a, St.StreamingDetector(few, fe10, 3, **DET), 0.5)
    fe8 = Cm.make_frontend(lib, 320, 160, sample_rate=8000, upper_hz=3800.0)
    fe8b, net8, _, _, _ = setup(lib, win=640, hop=320)
    slow = St.StreamingDetector(net8, fe8b, 3, **DET)
    slow.frontend = fe8                                             # (only the rate is read)
    with pytest.raises(T.TcrError, match="different sample rates \\(16000 and 8000 Hz\\)"):
        St.StreamingCascade(a, slow, 0.5)
    with pytest.raises(T.TcrError, match="hold 3 and 2 streams"):
        St.StreamingCascade(a, St.StreamingDetector(net, fe, 2, **DET), 0.5)
    with pytest.raises(T.TcrError, match="on must be"):
        St.StreamingCascade(a, a, 0.5, on="logits")
    with pytest.raises(T.TcrError, match="enter_threshold is NaN"):
        St.StreamingCascade(a, a, float("nan"))
    with pytest.raises(T.TcrError, match="keyword_classes outside 0..11"):
        St.StreamingCascade(a, a, 0.5, keyword_classes=[12])
    with pytest.raises(T.TcrError, match="negative pads"):
        St.StreamingCascade(a, a, 0.5, pad_after_ms=-40)
    ok = St.StreamingCascade(a, St.StreamingDetector(net, fe, 3, **DET), 0.5)
    assert ok.keyword_classes == KEYWORDS and (ok.pad_before, ok.pad_after) == (0, 4)

    # tcr_stream_select
    dev = Cm.device_of(lib)
    S, ncls = 5, 12
    values = torch.zeros((S, ncls), dtype=torch.float32, device=dev)
    cm = torch.ones(ncls, dtype=torch.uint8, device=dev)
    since = torch.empty(S, dtype=torch.int32, device=dev)
    sel, count = torch.zeros(S, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    nws = lib.tcr_stream_select_workspace_bytes(S)
    ws = torch.empty(nws // 4, dtype=torch.int32, device=dev)
    assert lib.tcr_stream_select_workspace_bytes(0) == 0 and nws > 0
    assert lib.tcr_stream_select_init(0, since.data_ptr(), None) == -1 and lib.tcr_stream_select_init(S, None, None) == -1

    def select(S=S, ncls=ncls, values=values.data_ptr(), cm=cm.data_ptr(), enter=0.5, pad=1, since=since.data_ptr(), ws=ws.data_ptr(),
               ws_bytes=nws, sel=sel.data_ptr(), count=count.data_ptr()):
        return lib.tcr_stream_select(S, ncls, values, cm, enter, pad, None, since, ws, ws_bytes, sel, count, None, None)

    with Log(lib) as g:
        for kw, msg in [(dict(values=None), "null argument"), (dict(cm=None), "null argument"), (dict(since=None), "null argument"),
                        (dict(ws=None), "null argument"), (dict(sel=None), "null argument"), (dict(count=None), "null argument"),
                        (dict(S=0), "number of streams must be positive"), (dict(ncls=0), "num_classes 0 outside 1..256"),
                        (dict(ncls=257), "num_classes 257 outside 1..256"), (dict(enter=float("nan")), "enter is NaN"),
                        (dict(pad=-1), "pad_after must be >= 0")]:
            assert select(**kw) == -1, kw
            assert msg in lib.tcr_last_error().decode(), (kw, lib.tcr_last_error())
        assert select(ws_bytes=nws - 1) == -3 and "workspace" in lib.tcr_last_error().decode()
    assert not g.entries

    # tcr_stream_step_selected_m / push_selected
    b = ok.second
    x = torch.zeros((3, 320), dtype=torch.float32, device=dev)
    idx = torch.arange(3, dtype=torch.int64, device=dev)
    fill = torch.zeros((3, 12), dtype=torch.float32, device=dev)
    with pytest.raises(T.TcrError, match="n_selected 4 outside 0..3"):
        b.push_selected(x, idx, 4, fill, fill)
    with pytest.raises(T.TcrError, match="n_selected -1 outside 0..3"):
        b.push_selected(x, idx, -1, fill, fill)
    with pytest.raises(T.TcrError, match="fill_logits is None with 2 of 3"):
        b.push_selected(x, idx, 2, None, fill)
    with pytest.raises(T.TcrError, match="expects selected"):
        b.push_selected(x, idx.to(torch.int32), 2, fill, fill)
    b.push_selected(x, idx, 3, None, None)                       # (allocates the workspace)
    ref, o, wsb = b._call_ref(), b.out, b._sel_ws

    def step(n=2, selected=idx.data_ptr(), fl=fill.data_ptr(), fp=fill.data_ptr(), ws_bytes=wsb.numel() * 4, samples=x.data_ptr(), k=1):
        return lib.tcr_stream_step_selected_m(C.byref(b.frontend.cfg), b.frontend.plan.data_ptr(), C.byref(ref), 3, k, C.byref(b.det), samples,
                                              None, b.state.data_ptr(), wsb.data_ptr(), ws_bytes, selected, n, fl, fp, o.logits.data_ptr(),
                                              o.probs.data_ptr(), o.smoothed.data_ptr(), o.top.data_ptr(), o.score.data_ptr(),
                                              o.is_new.data_ptr(), None)

    before = b.state.clone()
    with Log(lib) as g:
        for kw, msg in [(dict(n=-1), "n_selected -1 outside 0..3"), (dict(n=4), "n_selected 4 outside 0..3"),
                        (dict(selected=None), "null selected with n_selected = 2"), (dict(fl=None), "null fill rows with 2 of 3"),
                        (dict(fp=None, n=0), "null fill rows with 0 of 3"), (dict(samples=None), "null argument"),
                        (dict(k=0), "frames per step k = 0 outside")]:
            assert step(**kw) == -1, kw
            assert msg in lib.tcr_last_error().decode(), (kw, lib.tcr_last_error())
        assert step(ws_bytes=wsb.numel() * 4 - 4) == -3 and "workspace" in lib.tcr_last_error().decode()
        assert lib.tcr_stream_selected_workspace_bytes_m(C.byref(b.frontend.cfg), C.byref(ref), 0, 1) == 0
    assert not g.entries and torch.equal(b.state.view(torch.int32), before.view(torch.int32))
    assert step(n=3, fl=None, fp=None) == 0 and step(n=0, selected=None) == 0


def test_cli_stream_cascade_flags():
    """The argument checks come before any model is opened."""
    from tcresnet_amd import audio_input, scan_audio, stream_audio, sweep_audio
    base = ["--frozen", "a.npz", "--wav", "a.wav"]
    for extra, msg in [(["--enter_threshold", "0.5"], "give --second_frozen"), (["--cascade_pad_ms", "100"], "give --second_frozen"),
                       (["--second_frozen", "b.npz"], "needs --enter_threshold")]:
        with pytest.raises(SystemExit, match=msg):
            audio_input.open_streaming_cascade(stream_audio.parse_arguments(base + extra), 1)
    args = stream_audio.parse_arguments(base + ["--second_frozen", "b.npz", "--enter_threshold", "-inf"])
    assert args.enter_threshold == float("-inf") and args.second_frames_per_step == 1 and args.cascade_pad_ms is None
    assert audio_input.open_streaming_cascade(stream_audio.parse_arguments(base), 1) is None
    for tool in (scan_audio, sweep_audio):
        more = [] if tool is scan_audio else ["--events", "e.csv", "--thresholds", "0.5"]
        with pytest.raises(SystemExit, match="give --second_frozen"):
            audio_input.open_cascade(tool.parse_arguments(base + more + ["--ragged", "--cascade_pad_before_ms", "0"]))
        args = tool.parse_arguments(base + more + ["--ragged", "--second_frozen", "b.npz", "--enter_threshold", "0.5"])
        assert args.cascade_pad_before_ms is None


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pair,S,on,seed", [("tc8_3010_k2_dscnn_s", 64, "probs", 81), ("tc8_tc14", 16, "smoothed", 82)])
def test_gpu_stream_cascade_equals_causal_scan(hip_lib, pair, S, on, seed):
    check_equals_causal_scan(hip_lib, case(hip_lib, pair, [60] * S, seed), 0.5, 40, on)


@pytest.mark.gpu
def test_gpu_stream_cascade_1100_streams(hip_lib):
    """Crosses the compaction tile and runs several gather workgroups."""
    c = case(hip_lib, "tc8_tc8", [6] * 1100, 83)
    S = 1100
    x = torch.stack(c["signals"])
    _, peak, _ = first_values(c["out1"], "probs", S)
    enter = float(np.median(peak))
    ref, mask, _, _ = reference(c["first"], c["second"], c["out1"], x, enter, 40)
    assert 0 < mask.sum() < mask.size and mask[1030:].any()
    got = run_cascade(streaming().StreamingCascade(*detectors(c, S), enter, pad_after_ms=40), x)
    assert np.array_equal(got.mask, mask)
    assert_fields(got, ref)


@pytest.mark.gpu
def test_gpu_stream_cascade_2d_graph_second_stage(hip_lib):
    """The plane-layout gather."""
    c = graph_case(hip_lib, 8, 20, 84)
    x = torch.stack(c["signals"])
    _, peak, _ = first_values(c["out1"], "probs", 8)
    enter = float(np.median(peak))
    ref, mask, _, _ = reference(c["first"], c["second"], c["out1"], x, enter, 40)
    per_step = mask.sum(axis=0)
    assert ((per_step > 0) & (per_step < 8)).any(), per_step
    got = run_cascade(streaming().StreamingCascade(*detectors(c, 8), enter, pad_after_ms=40), x)
    assert np.array_equal(got.mask, mask)
    assert_fields(got, ref)


@pytest.mark.gpu
def test_gpu_stream_cascade_everything_and_nothing_selected(hip_lib):
    c = case(hip_lib, "tc8_3010_k2_dscnn_s", [60] * 64, 81)
    check_everything_selected(hip_lib, c)
    check_nothing_selected(hip_lib, c)


@pytest.mark.gpu
def test_gpu_stream_audio_cli_cascade(hip_lib, tmp_path):
    """stream_audio.py feeds a file that has ended zeros, in lockstep with the longest, and prints what fires there (with or without a
    cascade); scan_audio.py --ragged has no steps past a file's end.  So the byte-for-byte runs use three files whose lengths differ
    by less than a step (the samples that do not fill one are dropped), and one more pair of runs, on files of 200, 128 and 62 steps,
    compares the lines up to each file's own end."""
    first, second = cli_models(hip_lib, tmp_path)
    lengths, ragged = [64000, 64100, 64250], [64000, 41234, 20000]
    wavs, wavs2 = cli_files(tmp_path, lengths, [16000] * 3, 85), cli_files(tmp_path, ragged, [16000] * 3, 86)
    stream, scan = (os.path.join(ROOT, "tc-resnet_amd", n) for n in ("stream_audio.py", "scan_audio.py"))
    det = ["--labels", ",".join(f"c{i}" for i in range(12)), "--average_window_ms", "200", "--min_count", "2", "--detection_threshold", "0.3",
           "--suppression_ms", "400"]
    cas = ["--frozen", first, "--second_frozen", second, "--enter_threshold", "0.3", "--cascade_pad_ms", "80"]
    offline = ["--cascade_pad_before_ms", "0", "--ragged"]
    phr = ["--phrases", "c2 c3;c3 c2;c4 c5", "--phrase_window_ms", "1000"]
    w, w2 = ["--wav", *wavs], ["--wav", *wavs2]
    runs = run_all([[stream, *cas, *w, *det], [scan, *cas, *offline, *w, *det],
                    [stream, "--frozen", first, "--second_frozen", second, "--enter_threshold", "-inf", *w2, *det], [stream, "--frozen", second, *w2, *det],
                    [stream, *cas, *w, *det, *phr], [scan, *cas, *offline, *w, *det, *phr],
                    [stream, *cas, *w2, *det], [scan, *cas, *offline, *w2, *det]])
    for r in runs:
        assert r[0] == 0, r[2]
    assert runs[0][1] == runs[1][1] and len(runs[0][1].splitlines()) >= 3
    assert all(f"dropping the last {n % 320} samples" in runs[0][2] for n in lengths[1:])
    assert runs[2][1] == runs[3][1] and len(runs[3][1].splitlines()) >= 3
    assert runs[4][1] == runs[5][1]
    end_ms = {path: n // 320 * 20 for path, n in zip(wavs2, ragged)}
    inside = [line for line in runs[6][1].splitlines() if float(line.split(",")[1]) <= end_ms[line.split(",")[0]]]
    assert inside == runs[7][1].splitlines() and len(inside) >= 3
