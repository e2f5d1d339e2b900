"""Sparse scans (tcr_scan_steps, KeywordScanner.scan_steps) and step selection (tcr_scan_select, scanning.select_steps).  The reference
of every bitwise check of scan_steps is the existing ragged scan: row b is row selected[b] of `scan_ragged`.  select_steps is checked
against a NumPy statement of its rule; it has no floating-point arithmetic, so that comparison is exact too.  Emulator
(`-m "not gpu"`) and MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import DET
from tests.test_scan_ragged import STEPS_1, cut_signals, scanning
from tests.test_streaming import segment_audio, setup

_CACHE = {}


def offsets_of(steps):
    return np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)


def selections(steps, g, seed):
    """{name: packed steps} over signals of `steps` steps: the cases of the module's scan_steps tests.  g: the group size whose
    boundaries get both neighbours selected."""
    off = offsets_of(steps)
    total = int(off[-1])
    live = [n for n, s in enumerate(steps) if s > 0]
    ends = sorted({int(off[n]) for n in live} | {int(off[n + 1]) - 1 for n in live})
    bounds = sorted({int(off[n]) + i for n in live for m in range(g, steps[n], g) for i in (m - 1, m)})
    longest = int(np.argmax(steps))
    skip = [p for n in live if n != longest for p in range(int(off[n]), int(off[n + 1]))]
    rng = np.random.RandomState(seed)
    return {"all": list(range(total)), "one": [total // 2], "ends": ends, "bounds": bounds, "skip_longest": skip,
            "random": np.flatnonzero(rng.rand(total) < 0.3).tolist()}


def check_steps_equal_ragged_rows(lib, fe, net, steps, k, seed, max_windows, g):
    """scan_steps at every max_windows and every selection against the rows of one scan_ragged (default max_windows)."""
    Sc = scanning()
    step = k * fe.cfg.hop
    signals = cut_signals(lib, segment_audio(len(steps), max(steps) * step, seed), steps, step)
    want = Sc.KeywordScanner(net, fe, frames_per_step=k, **DET).scan_ragged(signals)
    scanners = [Sc.KeywordScanner(net, fe, frames_per_step=k, max_windows=m, **DET) for m in max_windows]
    sels = selections(steps, g, seed)
    assert all(len(s) > 0 for s in sels.values()), {n: len(s) for n, s in sels.items()}
    for name, sel in sels.items():
        idx = torch.tensor(sel, dtype=torch.int64)
        got = [sc.scan_steps(signals, idx) for sc in scanners]
        at = idx.to(want.logits.device)
        for m, (logits, probs) in zip(max_windows, got):
            assert logits.shape == probs.shape == (len(sel), net.num_classes), (name, m)
            assert torch.equal(logits, want.logits[at]), (name, m, int((logits != want.logits[at]).sum()))
            assert torch.equal(probs, want.probs[at]), (name, m)
        for logits, probs in got[1:]:
            assert torch.equal(logits, got[0][0]) and torch.equal(probs, got[0][1]), name
    return scanners, signals, sels, want


# ---- emulator: scan_steps -------------------------------------------------------------------------------------------------------
def test_scan_steps_equals_ragged_rows(emu_lib):
    """TCResNet8, 4020, k = 1, the six signals of the ragged tests at max_windows 1, 7 and the default."""
    fe, net, _, _, _ = setup(emu_lib)
    scanners, signals, sels, _ = check_steps_equal_ragged_rows(emu_lib, fe, net, STEPS_1, 1, 3, (1, 7, None), 7)
    # the plans: max_windows = 7 cuts into groups of at most 7 steps and runs one row at a time; one step is one row of T frames
    plan = scanners[1].steps_plan(signals, sels["all"])
    assert 1 <= plan["group_steps"] <= 7 and plan["chunk_rows"] * plan["group_steps"] <= 7 and plan["windows"] == 103
    assert plan["rows"] == sum(-(-s // plan["group_steps"]) for s in STEPS_1)
    one = scanners[2].steps_plan(signals, sels["one"])
    assert (one["group_steps"], one["rows"], one["row_frames"]) == (1, 1, fe.n_frames)
    # the longest signal has no live group when none of its steps is selected
    skip = scanners[1].steps_plan(signals, sels["skip_longest"])
    assert skip["rows"] == sum(-(-s // skip["group_steps"]) for s in STEPS_1 if s != 63) and skip["windows"] == 40
    # forms of `selected`: a device tensor, an array, a list
    want = scanners[2].scan_steps(signals, sels["ends"])
    for form in (torch.tensor(sels["ends"], dtype=torch.int64, device=Cm.device_of(emu_lib)), np.array(sels["ends"], np.int32)):
        got = scanners[2].scan_steps(signals, form)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    empty = scanners[2].scan_steps(signals, [])
    assert empty[0].shape == (0, 12) and empty[1].shape == (0, 12)


def test_scan_steps_k3(emu_lib):
    fe, net, _, _, _ = setup(emu_lib)
    check_steps_equal_ragged_rows(emu_lib, fe, net, [21, 5, 0, 9], 3, 4, (1, 4, None), 4)


def test_scan_steps_3010_log_mel_k2(emu_lib):
    fe, net, _, _, _ = setup(emu_lib, win=480, hop=160, method="log_mel_spectrogram")
    check_steps_equal_ragged_rows(emu_lib, fe, net, [17, 0, 30], 2, 5, (1, 8, None), 8)


@pytest.mark.parametrize("model", ["dscnn_s", "tiny_conv"])
def test_scan_steps_families(emu_lib, model):
    """DS-CNN, and a 2-D graph (the planes gather)."""
    from tests.test_detect_families import MODELS
    fe, net = MODELS[model](emu_lib)
    check_steps_equal_ragged_rows(emu_lib, fe, net, [9, 2, 0, 14], 1, 6, (1, 5, None), 5)


def test_scan_steps_launch_log(emu_lib):
    """A scan_steps call reaches the new kernels and none of the scan's own instances; one selected step is one front-end launch and
    one network call."""
    from tests.test_detect_families import MODELS
    from tests.test_net_configs import Log, kernel_of
    Sc = scanning()
    fe, net, _, _, _ = setup(emu_lib)
    x = Cm.to_dev(emu_lib, segment_audio(2, 30 * 320, 79))
    signals = [x[0], x[1, :9 * 320]]
    sc = Sc.KeywordScanner(net, fe, max_windows=16, **DET)
    sc.scan_ragged([x[0, :320]])                                    # (the first call folds the BN table)
    with Log(emu_lib) as full:
        sc.scan_ragged([x[0, :320]])
    network = [kernel_of(e) for e in full.entries if "scan_" not in e and "frontend" not in e]
    assert len(network) >= 1
    with Log(emu_lib) as g:
        sc.scan_steps(signals, [33])
    names = [kernel_of(e) for e in g.entries]
    assert names[:3] == ["steps_stage_kernel", "frontend_pk3_kernel", "steps_gather_kernel"], g.entries
    assert names[3:] == network, (names, network)                  # the network at batch 1, once
    assert g.has("steps_gather_kernel<false>") and not g.has("scan_") and not g.has("select_"), g.entries
    with Log(emu_lib) as g:
        sc.scan_steps(signals, list(range(39)))
    assert sum("steps_stage_kernel" in e for e in g.entries) >= 2 and not g.has("scan_"), g.entries
    fe2, net2 = MODELS["tiny_conv"](emu_lib)
    with Log(emu_lib) as g:
        Sc.KeywordScanner(net2, fe2, max_windows=4, **DET).scan_steps([torch.zeros(3 * fe2.cfg.hop, device=x.device)], [0, 2])
    assert g.has("steps_gather_kernel<true>") and not g.has("steps_gather_kernel<false>") and not g.has("scan_"), g.entries


def test_scan_steps_refusals(emu_lib):
    Sc = scanning()
    lib = emu_lib
    fe, net, _, _, _ = setup(lib)
    sc = Sc.KeywordScanner(net, fe, frames_per_step=2)            # k * hop = 640
    z = lambda n: torch.zeros(n)
    with pytest.raises(T.TcrError, match="not a multiple of k \\* hop"):
        sc.scan_steps([z(640), z(1000)], [0])
    with pytest.raises(T.TcrError, match="outside 0..2"):
        sc.scan_steps([z(640), z(1280)], [0, 3])
    with pytest.raises(T.TcrError, match="outside 0..2"):
        sc.scan_steps([z(640), z(1280)], [-1, 2])
    with pytest.raises(T.TcrError, match="not strictly increasing at 2"):
        sc.scan_steps([z(640), z(1280)], [0, 2, 2])
    with pytest.raises(T.TcrError, match="not strictly increasing at 1"):
        sc.scan_steps([z(640), z(1280)], [2, 1])
    with pytest.raises(T.TcrError, match="1-D"):
        sc.scan_steps([z(640)], [[0]])
    with pytest.raises(T.TcrError, match="int64"):
        sc.scan_steps([z(640)], torch.zeros(1, dtype=torch.int32))
    with pytest.raises(T.TcrError, match="total_steps == 0"):
        sc.scan_steps([z(0), z(0)], [])
    # the C entry refuses on its own (status + message), before anything is launched: the buffers below are never touched
    ref = T._lib.ModelRef(T._lib.FAMILY_TCRESNET, net._h.value, net.params.data_ptr(), net.fold_bn().data_ptr())
    buf = torch.full((1 << 16,), 7.0)
    p = buf.data_ptr()
    chunk = lib.tcr_scan_workspace_bytes_m(C.byref(fe.cfg), C.byref(ref), 1, 16)
    assert lib.tcr_scan_steps_workspace_bytes(C.byref(fe.cfg), C.byref(ref), 1, 16, 4, 9) == 256 + chunk      # (5 + 27) x 8 bytes
    assert lib.tcr_scan_steps_workspace_bytes(C.byref(fe.cfg), C.byref(ref), 1, 16, 4, 10) == 512 + chunk
    for args, msg in [((1, 16, 0, 9), b"max_signals"), ((1, 0, 4, 9), b"max_windows"), ((1, 16, 4, 0), b"max_selected"),
                      ((0, 16, 4, 9), b"frames per step")]:
        assert lib.tcr_scan_steps_workspace_bytes(C.byref(fe.cfg), C.byref(ref), *args) == 0 and msg in lib.tcr_last_error(), args

    def call(offsets, sel, n=None, nsel=None, ws=1 << 18, samples=p, k=1, out=p, sel_ptr=True):
        off, s = np.asarray(offsets, np.int64), np.asarray(sel, np.int64)
        return lib.tcr_scan_steps(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), len(off) - 1 if n is None else n,
                                  off.ctypes.data if len(off) else None, k, s.ctypes.data if sel_ptr else None,
                                  len(s) if nsel is None else nsel, samples, p, ws, out, out, None)
    for args, kw, status, msg in [(([320, 640], [0]), {}, -1, b"sample_offsets must start at 0"),
                                  (([0, 650], [0]), {}, -1, b"length 650 of signal 0 is not a multiple of k * hop = 320"),
                                  (([0, 640, 320], [0]), {}, -1, b"sample_offsets decrease at signal 1"),
                                  (([0, 0, 0], []), {}, -1, b"total_steps == 0"),
                                  (([0, 320], [0]), dict(n=0), -1, b"number of signals must be positive"),
                                  (([], [0]), dict(n=1), -1, b"null argument"),
                                  (([0, 320], [0]), dict(samples=None), -1, b"null argument"),
                                  (([0, 320], [0]), dict(out=None), -1, b"null argument"),
                                  (([0, 320], [0]), dict(k=0), -1, b"frames per step"),
                                  (([0, 640], [0, 1]), dict(nsel=-1), -1, b"n_selected must be >= 0"),
                                  (([0, 640], [0, 1]), dict(sel_ptr=False), -1, b"null selected"),
                                  (([0, 640], [0, 2]), {}, -1, b"selected[1] = 2 outside 0..1"),
                                  (([0, 640], [-1, 1]), {}, -1, b"selected[0] = -1 outside 0..1"),
                                  (([0, 640], [1, 1]), {}, -1, b"not strictly increasing at 1"),
                                  (([0, 640], [1, 0]), {}, -1, b"not strictly increasing at 1"),
                                  (([0] + [320] * 40, [0]), dict(ws=256), -1, b"more than the max_signals and max_selected"),
                                  (([0, 320 * 40], list(range(40))), dict(ws=768), -1, b"more than the max_signals and max_selected"),
                                  (([0, 320], [0]), dict(ws=1024), -3, b"one window")]:
        assert call(*args, **kw) == status, (args, kw, lib.tcr_last_error())
        assert msg in lib.tcr_last_error(), (args, kw, lib.tcr_last_error())
    assert call([0, 320], [], samples=None, out=None) == 0           # nothing selected: nothing to do
    assert bool((buf == 7.0).all())


# ---- emulator: select_steps -----------------------------------------------------------------------------------------------------
def select_reference(values, offsets, enter, classes, pad_before, pad_after):
    """The rule, stated directly: flagged, then selected per signal."""
    v = values[:, list(classes)] if len(classes) else np.zeros((len(values), 0), np.float32)
    with np.errstate(invalid="ignore"):
        flag = (v >= np.float32(enter)).any(axis=1)
    sel = np.zeros(len(values), bool)
    for a, b in zip(offsets[:-1], offsets[1:]):
        for q in np.flatnonzero(flag[a:b]) + a:
            sel[max(a, q - pad_before):min(b, q + pad_after + 1)] = True   # p - pad_after <= q <= p + pad_before
    return np.flatnonzero(sel).astype(np.int64), sel.astype(np.uint8)


def check_select(lib, values, offsets, enter, classes, pads):
    Sc = scanning()
    got_sel, got_mask = Sc.select_steps(Cm.to_dev(lib, values), offsets, enter, classes, *pads, lib=lib)
    want_sel, want_mask = select_reference(values, offsets, enter, classes, *pads)
    assert got_sel.dtype == torch.int64 and got_mask.dtype == torch.uint8
    assert np.array_equal(got_sel.cpu().numpy(), want_sel), (enter, classes, pads)
    assert np.array_equal(got_mask.cpu().numpy(), want_mask), (enter, classes, pads)
    member = np.zeros(len(values), np.uint8)
    member[got_sel.cpu().numpy()] = 1
    assert np.array_equal(got_mask.cpu().numpy(), member)
    return want_sel


SEL_STEPS = [0, 1, 9, 300, 2]
PADS = [(0, 0), (3, 0), (0, 2), (40, 40), (1000, 1000)]


@pytest.mark.parametrize("ncls", [3, 12])
def test_select_steps_rule(emu_lib, ncls):
    off = offsets_of(SEL_STEPS)                                     # [0, 0, 1, 10, 310, 312]
    total = int(off[-1])
    values = np.random.RandomState(7).uniform(0.0, 0.4, (total, ncls)).astype(np.float32)
    last = ncls - 1
    # flags (0.75) at a signal's first and last step: signal 2's last (9) touches signal 3's first (10), signal 3's last (309) signal
    # 4's first (310); one in the middle; a NaN and a value just below `enter` that must not flag; a flag in class 0, which is masked
    for p in (1, 9, 150, 309):
        values[p, last] = 0.75
    values[100, last] = np.nan
    values[200, last] = np.nextafter(np.float32(0.75), np.float32(0))
    values[250, 0] = 0.9
    classes = list(range(1, ncls))
    for pads in PADS:
        sel = check_select(emu_lib, values, off, 0.75, classes, pads)              # `>=` counts the values at exactly 0.75
        assert {1, 9, 150, 309} <= set(sel.tolist())
        if pads == (0, 0):
            assert sel.tolist() == [1, 9, 150, 309]
        if pads == (0, 2):
            assert sel.tolist() == [1, 2, 3, 9, 150, 151, 152, 309]                 # 9 does not reach 10, 309 does not reach 310
        if pads == (3, 0):
            assert sel.tolist() == [1, 6, 7, 8, 9, 147, 148, 149, 150, 306, 307, 308, 309]
        if pads == (1000, 1000):
            assert sel.tolist() == list(range(1, 310))                              # whole signals 2 and 3; signals 1 and 4 have no flag
    check_select(emu_lib, values, off, float("-inf"), classes, (0, 0))
    sel, _ = scanning().select_steps(Cm.to_dev(emu_lib, values), off, float("-inf"), classes, lib=emu_lib)
    assert sel.numel() == total                                                     # (the NaN row has other classes)
    assert check_select(emu_lib, values, off, float("inf"), classes, (40, 40)).size == 0
    # the mask hides the only class above `enter`
    assert check_select(emu_lib, values, off, 0.85, classes, (3, 3)).size == 0
    assert check_select(emu_lib, values, off, 0.85, [0], (3, 3)).tolist() == list(range(247, 254))
    assert check_select(emu_lib, values, off, 0.0, [], (3, 3)).size == 0


def big_select_case(seed=11, total=300000, ncls=3):
    """More than one workgroup of every phase and a second pass of the scan of the sums: 300000 steps are 293 tiles of 1024."""
    rng = np.random.RandomState(seed)
    cuts = np.sort(rng.choice(np.arange(1, total), 40, replace=False))
    off = np.concatenate([[0], cuts[:20], cuts[19:20], cuts[20:], [total]]).astype(np.int64)        # one signal without steps
    values = rng.uniform(0.0, 0.5, (total, ncls)).astype(np.float32)
    hot = rng.choice(total, 700, replace=False)
    values[hot, rng.randint(1, ncls, hot.size)] = 0.9
    values[off[1:-1] - 1, 1] = 0.9                                  # a flag at every signal's last step
    values[rng.choice(total, 50, replace=False), 2] = np.nan
    return values, off


def test_select_steps_many_tiles(emu_lib):
    values, off = big_select_case()
    for pads in ((0, 0), (25, 60)):
        sel = check_select(emu_lib, values, off, 0.9, [1, 2], pads)
        assert 700 <= sel.size < len(values) // 2
    assert check_select(emu_lib, values, off, float("-inf"), [0], (0, 0)).size == len(values)


def test_select_steps_refusals(emu_lib):
    Sc = scanning()
    lib = emu_lib
    v = torch.zeros((10, 3))
    with pytest.raises(T.TcrError, match="offsets must run from 0"):
        Sc.select_steps(v, [0, 4, 9], 0.5, [1], lib=lib)
    with pytest.raises(T.TcrError, match="classes outside 0..2"):
        Sc.select_steps(v, [0, 10], 0.5, [3], lib=lib)
    with pytest.raises(T.TcrError, match="float32 values"):
        Sc.select_steps(v.double(), [0, 10], 0.5, [1], lib=lib)
    with pytest.raises(T.TcrError, match="enter is NaN"):
        Sc.select_steps(v, [0, 10], float("nan"), [1], lib=lib)
    with pytest.raises(T.TcrError, match="pads must be >= 0"):
        Sc.select_steps(v, [0, 10], 0.5, [1], pad_before=-1, lib=lib)
    buf = torch.full((1 << 12,), 7.0)
    p = buf.data_ptr()
    assert lib.tcr_scan_select_workspace_bytes(0) == 0 and lib.tcr_scan_select_workspace_bytes(1 << 31) == 0
    need = lib.tcr_scan_select_workspace_bytes(10)
    assert need == 256 + 256 + 256

    def call(n=1, off=p, total=10, ncls=3, values=p, cmask=p, enter=0.5, before=0, after=0, ws=p, ws_bytes=need, sel=p, count=p):
        return lib.tcr_scan_select(n, off, total, ncls, values, cmask, enter, before, after, ws, ws_bytes, sel, count, None, None)
    for kw, status, msg in [(dict(off=None), -1, b"null argument"), (dict(values=None), -1, b"null argument"),
                            (dict(cmask=None), -1, b"null argument"), (dict(ws=None), -1, b"null argument"),
                            (dict(sel=None), -1, b"null argument"), (dict(count=None), -1, b"null argument"),
                            (dict(n=0), -1, b"number of signals must be positive"), (dict(total=0), -1, b"number of steps must be positive"),
                            (dict(ncls=0), -1, b"num_classes 0 outside"), (dict(ncls=257), -1, b"num_classes 257 outside"),
                            (dict(enter=float("nan")), -1, b"enter is NaN"), (dict(before=-1), -1, b"pads must be >= 0"),
                            (dict(after=-2), -1, b"pads must be >= 0"), (dict(ws_bytes=need - 1), -3, b"workspace")]:
        assert call(**kw) == status, (kw, lib.tcr_last_error())
        assert msg in lib.tcr_last_error(), (kw, lib.tcr_last_error())
    assert bool((buf == 7.0).all())


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
def gpu_steps_corpus(lib, model):
    """64 signals of seeded 1 .. 300 steps (one without steps), a model's ragged scan of them and the scan's signals."""
    if model not in _CACHE:
        Sc = scanning()
        if model == "tcresnet8":
            fe, net, _, _, _ = setup(lib)
        else:
            from tests.test_detect_families import MODELS
            fe, net = MODELS[model](lib)
        steps = np.random.RandomState(61).randint(1, 301, 64)
        steps[9] = 0
        step = fe.cfg.hop
        signals = cut_signals(lib, segment_audio(64, 300 * step, 62), steps, step)
        want = Sc.KeywordScanner(net, fe, **DET).scan_ragged(signals)
        _CACHE[model] = dict(fe=fe, net=net, steps=steps.tolist(), signals=signals, want=want)
    return _CACHE[model]


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["tcresnet8", "dscnn_s"])
def test_gpu_scan_steps_64_signals(hip_lib, model):
    Sc = scanning()
    c = gpu_steps_corpus(hip_lib, model)
    want = c["want"]
    scanners = [Sc.KeywordScanner(c["net"], c["fe"], max_windows=m, **DET) for m in (16, None)]
    for name, sel in selections(c["steps"], 16, 63).items():
        idx = torch.tensor(sel, dtype=torch.int64, device="cuda")
        got = [sc.scan_steps(c["signals"], idx) for sc in scanners]
        for logits, probs in got:
            assert torch.equal(logits, want.logits[idx]), (name, int((logits != want.logits[idx]).sum()))
            assert torch.equal(probs, want.probs[idx]), name


@pytest.mark.gpu
def test_gpu_select_steps(hip_lib):
    values, off = big_select_case()
    for pads in ((0, 0), (25, 60), (100000, 100000)):
        check_select(hip_lib, values, off, 0.9, [1, 2], pads)
    assert check_select(hip_lib, values, off, float("-inf"), [0], (0, 0)).size == len(values)
    assert check_select(hip_lib, values, off, float("inf"), [0, 1, 2], (5, 5)).size == 0
    v12 = np.random.RandomState(12).uniform(0, 1, (5000, 12)).astype(np.float32)
    check_select(hip_lib, v12, np.array([0, 1, 1, 4000, 5000], np.int64), 0.97, list(range(2, 12)), (7, 3))
