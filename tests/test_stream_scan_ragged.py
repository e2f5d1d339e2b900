"""Ragged many-step pushes (tcr_stream_scan_ragged, StreamingDetector.push_ragged): every stream advances by its own number of
steps in one call, none included.  The oracle of stream s is a one-stream StreamingDetector with the same settings fed the same
samples; outputs and the stream's slices of the state (window, tail, the five integers, the live ring slots) are compared bitwise,
and a stream without steps is byte for byte what it was.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan import assert_bitwise, pushed, scanning
from tests.test_scan_ragged import cli_files, run_all
from tests.test_stream_scan import assert_same_state, state_parts, streaming
from tests.test_streaming import frozen_artifact, segment_audio, setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET = dict(average_window_ms=200, min_count=2, detection_threshold=0.0, suppression_ms=200)       # 4020, k = 1: W = 10


def parts_of(det, state):
    """state_parts of another tensor laid out as det's state (a clone taken earlier)."""
    return state_parts(SimpleNamespace(frontend=det.frontend, n_streams=det.n_streams, average_steps=det.average_steps, net=det.net,
                                       state=state))


def assert_streams_match(dut, oracles):
    """assert_same_state's rule, taken per stream: stream s's window, tail and five integers are the one-stream oracle's, and so are
    the ring slots of its last min(count, W) vectors (the other slots are never read)."""
    w, t, r, i = state_parts(dut)
    po = [state_parts(o) for o in oracles]
    assert torch.equal(w, torch.cat([p[0] for p in po])), [s for s, p in enumerate(po) if not torch.equal(w[s], p[0][0])]
    assert torch.equal(t, torch.cat([p[1] for p in po])), [s for s, p in enumerate(po) if not torch.equal(t[s], p[1][0])]
    ints = torch.cat([p[3] for p in po], dim=1)
    assert torch.equal(i, ints), (i.cpu().numpy(), ints.cpu().numpy())
    W = dut.average_steps
    head, count = i[0].cpu().numpy().astype(np.int64), i[1].cpu().numpy().astype(np.int64)
    live = np.zeros((W, dut.n_streams), bool)
    for s in range(dut.n_streams):
        live[(head[s] - 1 - np.arange(count[s])) % W, s] = True
    same = (r == torch.cat([p[2] for p in po], dim=1)).all(dim=2).cpu().numpy()
    assert (same | ~live).all(), np.argwhere(~same & live).tolist()


def assert_untouched(dut, before, streams):
    """Every byte of the streams' state regions -- the whole ring column included -- is what the clone `before` holds."""
    now, was = state_parts(dut), parts_of(dut, before)
    for s in streams:
        assert torch.equal(now[0][s], was[0][s]) and torch.equal(now[1][s], was[1][s]), s
        assert torch.equal(now[2][:, s], was[2][:, s]) and torch.equal(now[3][:, s], was[3][:, s]), s


class Rig:
    """An S-stream detector under test next to S one-stream oracles, fed from one seeded audio array with a cursor per stream.
    The oracles advance by `push` (many=False) or by one-stream `push_many` calls (many=True)."""

    def __init__(self, lib, fe, net, S, total_steps, seed, k=1, det=DET, many=False, **dut_kw):
        St = streaming()
        self.lib, self.S, self.many = lib, S, many
        self.dut = St.StreamingDetector(net, fe, S, frames_per_step=k, **det, **dut_kw)
        self.oracles = [St.StreamingDetector(net, fe, 1, frames_per_step=k, max_windows=256, **det) for _ in range(S)]
        self.step = self.dut.step_samples
        self.audio = Cm.to_dev(lib, segment_audio(S, total_steps * self.step, seed))
        self.at = [0] * S
        self.fired = 0

    def take(self, counts):
        xs = [self.audio[s, self.at[s]:self.at[s] + m * self.step].contiguous() for s, m in enumerate(counts)]
        self.at = [a + m * self.step for a, m in zip(self.at, counts)]
        assert max(self.at) <= self.audio.shape[1]
        return xs

    def reset(self, streams):
        self.dut.reset(streams)
        for s in streams:
            self.oracles[s].reset([0])

    def want(self, xs):
        """The oracles' outputs for xs, [1, m, ...] per stream (None without steps)."""
        out = []
        for o, x in zip(self.oracles, xs):
            if not x.numel():
                out.append(None)
            else:
                out.append(list(o.push_many(x[None, :])) if self.many else pushed(o, x[None, :]))
        return out

    def check(self, got, want):
        counts = [0 if w is None else int(w[3].shape[1]) for w in want]
        assert got.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
        assert got.top.shape == (sum(counts),) and got.logits.shape[0] == sum(counts)
        for s, w in enumerate(want):
            g = got.signal(s)
            if w is None:
                assert g.top.shape == (1, 0)
            else:
                assert_bitwise(g, w)
        assert_streams_match(self.dut, self.oracles)
        self.fired += int(got.is_new.sum())

    def ragged(self, counts, packed=False):
        xs = self.take(counts)
        want = self.want(xs)
        before = self.dut.state.clone()
        got = self.dut.push_ragged((torch.cat(xs), [int(x.numel()) for x in xs]) if packed else xs)
        self.check(got, want)
        assert_untouched(self.dut, before, [s for s, m in enumerate(counts) if m == 0])
        return got

    def lockstep(self, m, many):
        """push (m = 1) or push_many on the detector under test, against the same oracles."""
        xs = self.take([m] * self.S)
        want = self.want(xs)
        x = torch.stack(xs)
        got = self.dut.push_many(x) if many else [t.unsqueeze(1) for t in self.dut.push(x)]
        for s, w in enumerate(want):
            assert_bitwise([t[s:s + 1] for t in got], w)
        assert_streams_match(self.dut, self.oracles)


# ---- emulator -------------------------------------------------------------------------------------------------------------------
PLAN_1 = [[3, 0, 7, 1], [0, 0, 2, 30], [20, 1, 0, 5], [1, 1, 1, 1], [0, 52, 0, 0]]


def test_push_ragged_plan_4020(emu_lib):
    """Streams that advance by different amounts, call after call: outputs and state are the one-stream oracles' after every call,
    a stream without steps keeps every byte, and stream 1's 52 steps in one call (past T / k = 49) end on windows without a carried
    column."""
    fe, net, _, _, _ = setup(emu_lib)
    assert fe.n_frames == 49
    rig = Rig(emu_lib, fe, net, 4, 54, 70, max_windows=16)
    assert rig.dut.average_steps == 10
    for n, counts in enumerate(PLAN_1):
        rig.ragged(counts, packed=n % 2 == 1)
    assert rig.fired >= 1


def test_push_ragged_resets(emu_lib):
    fe, net, _, _, _ = setup(emu_lib)
    rig = Rig(emu_lib, fe, net, 3, 30, 71, max_windows=16)
    rig.ragged([12, 12, 12])
    rig.reset([0, 1])                                     # stream 0 has steps in the next call, stream 1 has none
    rig.ragged([4, 0, 2])
    assert rig.dut._pending is not None and rig.dut._pending.tolist() == [False, True, False]
    ints = state_parts(rig.dut)[3].cpu().numpy()
    assert ints[4].tolist() == [4, 12, 14]                # the step counters: stream 0 restarted, stream 1 is where it was
    rig.ragged([0, 0, 3])                                 # still pending
    assert rig.dut._pending.tolist() == [False, True, False]
    rig.ragged([1, 5, 0])                                 # ... and applied at stream 1's first step
    assert rig.dut._pending is None
    assert state_parts(rig.dut)[3].cpu().numpy()[4].tolist() == [5, 5, 17]
    # the C entry with reset[s] = 1 and no step for s: the flag is ignored, stream s keeps every byte
    dut, lib = rig.dut, emu_lib
    xs = rig.take([2, 0, 1])
    want = rig.want(xs)
    packed = torch.cat(xs)
    off = np.array([0, 2 * rig.step, 2 * rig.step, 3 * rig.step], np.int64)
    flags = torch.tensor([0, 1, 0], dtype=torch.uint8)
    out = scanning().RaggedScanOutput(torch.empty((3, 12)), torch.empty((3, 12)), torch.empty((3, 12)), torch.empty(3, dtype=torch.int32),
                                      torch.empty(3), torch.empty(3, dtype=torch.int32), off // rig.step)
    ref = dut._call_ref()
    before = dut.state.clone()
    ws = dut._ragged_ws
    assert lib.tcr_stream_scan_ragged_m(C.byref(fe.cfg), fe.plan.data_ptr(), C.byref(ref), 3, off.ctypes.data, 1, C.byref(dut.det),
                                        packed.data_ptr(), flags.data_ptr(), dut.state.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                        *(t.data_ptr() for t in out.tensors()), None) == 0, lib.tcr_last_error()
    assert_untouched(dut, before, [1])
    rig.check(out, want)                                  # (the oracle of stream 1 was not reset either)
    rig.ragged([1, 1, 1])


def test_push_ragged_mixed_with_push_and_push_many(emu_lib):
    fe, net, _, _, _ = setup(emu_lib)
    k, S = 2, 3
    det = dict(average_window_ms=120, min_count=2, detection_threshold=0.0, suppression_ms=120)      # W = 3, suppression 3 steps
    rig = Rig(emu_lib, fe, net, S, 40, 72, k=k, det=det, max_windows=8)
    plan = [("push", 1, None), ("ragged", [3, 0, 1], None), ("many", 4, [1]), ("ragged", [0, 6, 2], [0, 2]), ("push", 1, None),
            ("ragged", [9, 1, 0], None), ("many", 2, [2]), ("ragged", [1, 1, 11], None), ("push", 1, [0])]
    for kind, m, rst in plan:
        if rst:
            rig.reset(rst)
        if kind == "ragged":
            rig.ragged(m)
        else:
            rig.lockstep(m, kind == "many")
    assert rig.dut._pending is None


def test_push_ragged_equal_steps_is_push_many(emu_lib):
    St = streaming()
    fe, net, _, _, _ = setup(emu_lib)
    S, chunks = 3, [2, 9, 1]
    a = St.StreamingDetector(net, fe, S, max_windows=16, **DET)
    b = St.StreamingDetector(net, fe, S, max_windows=16, **DET)
    x = Cm.to_dev(emu_lib, segment_audio(S, sum(chunks) * 320, 73))
    pos = 0
    for m in chunks:
        piece = x[:, pos:pos + m * 320].contiguous()
        pos += m * 320
        want = a.push_many(piece)
        got = b.push_ragged(list(piece))
        assert got.offsets.tolist() == [0, m, 2 * m, 3 * m]
        assert_bitwise([t.reshape((S, m) + tuple(t.shape[1:])) for t in got.tensors()], want)
        assert_same_state(b, a)


def test_push_ragged_chunking_invariance(emu_lib):
    """max_windows = 1 (G = 1: several groups of a stream read the tail and carried columns, and a stream's groups span many
    chunks), 7 and the default give the same bits."""
    fe, net, _, _, _ = setup(emu_lib)
    plan = [[2, 0, 5], [11, 3, 0], [0, 1, 4]]
    rigs = [Rig(emu_lib, fe, net, 3, 13, 74, max_windows=mw) for mw in (1, 7, None)]
    for rig in rigs[1:]:
        rig.oracles = rigs[0].oracles                     # one set of oracles: advanced by the first rig, compared by all
    for counts in plan:
        xs = rigs[0].take(counts)
        want = rigs[0].want(xs)
        outs = []
        for rig in rigs:
            before = rig.dut.state.clone()
            outs.append(rig.dut.push_ragged(xs))
            rig.check(outs[-1], want)
            assert_untouched(rig.dut, before, [s for s, m in enumerate(counts) if m == 0])
        for o in outs[1:]:
            assert all(torch.equal(p, q) for p, q in zip(o.tensors(), outs[0].tensors()))


def test_push_ragged_short_call_against_the_tail_3010(emu_lib):
    """A step of 160 samples is less than the tail of 320: old tail samples survive a call of one step, twice in a row."""
    fe, net, _, _, _ = setup(emu_lib, win=480, hop=160)
    cfg = fe.cfg
    assert cfg.win - cfg.hop + (cfg.n_samples - cfg.win) % cfg.hop == 320
    rig = Rig(emu_lib, fe, net, 4, 6, 75, det=dict(DET, average_window_ms=50, suppression_ms=30), max_windows=16)
    rig.ragged([1, 0, 2, 3])
    rig.ragged([1, 0, 2, 3])


def planes_write_back_with_surviving_tail(lib):
    """The planes form of the write-back with old tail samples surviving a call, through the ragged and the dense caller: a 2-D graph at
    win 480 / hop 160, k = 1, so that a step of 160 samples leaves 160 of the tail's 320.  Outputs and every state part are the
    one-stream oracles' after every call, a pending reset waits for its stream's next step, and a stream without steps keeps every
    byte (Rig.ragged)."""
    from tests.test_detect_families import kws_graph
    fe, net = kws_graph(lib, "tiny_conv", win=480, hop=160)
    cfg = fe.cfg
    tail_len = cfg.win - cfg.hop + (cfg.n_samples - cfg.win) % cfg.hop
    assert tail_len == 320 and 0 < tail_len - 1 * cfg.hop == 160
    rig = Rig(lib, fe, net, 3, 5, 83, det=dict(DET, average_window_ms=50, suppression_ms=30), max_windows=2)
    assert rig.step == 160
    rig.ragged([1, 0, 2])
    rig.reset([0, 1])
    rig.ragged([1, 0, 1])
    assert rig.dut._pending.tolist() == [False, True, False]
    rig.lockstep(1, many=True)
    assert rig.dut._pending is None
    rig.ragged([0, 1, 1])
    assert state_parts(rig.dut)[3].cpu().numpy()[4].tolist() == [2, 2, 5]


def test_push_ragged_planes_write_back_with_surviving_tail(emu_lib):
    planes_write_back_with_surviving_tail(emu_lib)


@pytest.mark.parametrize("case", ["4020_k3", "4020_k49", "3010_log_mel_k2"])
def test_push_ragged_other_k(emu_lib, case):
    if case == "3010_log_mel_k2":
        fe, net, _, _, _ = setup(emu_lib, win=480, hop=160, method="log_mel_spectrogram")
        assert fe.n_frames == 98 and fe.n_coef == 64
        k, det, plan = 2, DET, [[3, 0, 9], [1, 5, 0]]
    elif case == "4020_k3":
        fe, net, _, _, _ = setup(emu_lib)
        k, det, plan = 3, DET, [[2, 0, 18], [7, 1, 1]]
    else:
        fe, net, _, _, _ = setup(emu_lib)
        k, det, plan = 49, dict(DET, average_window_ms=2000, suppression_ms=1000), [[1, 0, 3], [2, 1, 0]]
    rig = Rig(emu_lib, fe, net, 3, sum(max(c) for c in plan), 76, k=k, det=det, max_windows=8)
    for counts in plan:
        rig.ragged(counts)


@pytest.mark.parametrize("model", ["dscnn_s", "tiny_conv"])
def test_push_ragged_families(emu_lib, model):
    """DS-CNN, and a 2-D graph (the planes forms of the gather and the write-back)."""
    from tests.test_detect_families import MODELS
    fe, net = MODELS[model](emu_lib)
    rig = Rig(emu_lib, fe, net, 3, 14, 77, det=dict(DET, average_window_ms=100), max_windows=5)
    rig.ragged([4, 0, 9])
    rig.ragged([0, 2, 5])


def test_push_ragged_pieces_equal_scan_ragged(emu_lib):
    """A ragged corpus pushed c steps at a time -- every stream min(c, what remains), none once it has ended -- is bitwise its
    one-call ragged scan."""
    St, Sc = streaming(), scanning()
    fe, net, _, _, _ = setup(emu_lib)
    steps, c = [1, 24, 0, 40, 7], 9
    audio = segment_audio(len(steps), max(steps) * 320, 78)
    signals = [Cm.to_dev(emu_lib, audio[n, :m * 320]) for n, m in enumerate(steps)]
    want = Sc.KeywordScanner(net, fe, max_windows=16, **DET).scan_ragged(signals)
    det = St.StreamingDetector(net, fe, len(steps), max_windows=16, **DET)
    rows = [[] for _ in steps]
    for i0 in range(0, max(steps), c):
        out = det.push_ragged([x[i0 * 320:(i0 + c) * 320] for x in signals])
        assert out.steps.tolist() == [max(0, min(c, m - i0)) for m in steps]
        for n in range(len(steps)):
            rows[n].append([t[0] for t in out.signal(n)])
    for f, w in enumerate(want.tensors()):
        got = torch.cat([piece[f] for n in range(len(steps)) for piece in rows[n]])
        assert torch.equal(got, w), Sc.RaggedScanOutput.FIELDS[f]
    assert int(want.is_new.sum()) >= 1


def test_push_ragged_launch_log(emu_lib):
    """push_ragged reaches the carried-and-ragged forms; push_many and scan_ragged keep the forms they had."""
    from tests.test_net_configs import Log
    St, Sc = streaming(), scanning()
    fe, net, _, _, _ = setup(emu_lib)
    x = Cm.to_dev(emu_lib, segment_audio(2, 3 * 320, 79))
    det = St.StreamingDetector(net, fe, 2, max_windows=16, **DET)
    with Log(emu_lib) as g:
        det.push_ragged([x[0], x[1, :320]])
    for name in ("scan_stage_ragged_kernel<true>", "scan_gather_kernel<false, true, true>", "scan_carry_kernel<false, true>",
                 "scan_smooth_kernel<true, true>", "scan_suppress_kernel<true>"):
        assert g.has(name), (name, g.entries)
    for name in ("scan_stage_kernel", "scan_stage_ragged_kernel<false>", "scan_carry_kernel<false, false>", "scan_carry_kernel<true",
                 "scan_scatter_kernel", "scan_gather_kernel<false, true, false>", "scan_smooth_kernel<true, false>",
                 "scan_suppress_kernel<false>"):
        assert not g.has(name), (name, g.entries)
    with Log(emu_lib) as g:
        det.push_many(x)
    for name in ("scan_stage_kernel", "scan_gather_kernel<false, true, false>", "scan_carry_kernel<false, false>", "scan_scatter_kernel",
                 "scan_smooth_kernel<true, false>", "scan_suppress_kernel<false>"):
        assert g.has(name), (name, g.entries)
    assert not g.has("ragged") and not g.has("scan_smooth_kernel<true, true>"), g.entries
    for name in ("scan_carry_kernel<false, true>", "scan_carry_kernel<true", "scan_gather_kernel<false, true, true>", "scan_suppress_kernel<true>"):
        assert not g.has(name), (name, g.entries)
    with Log(emu_lib) as g:
        Sc.KeywordScanner(net, fe, max_windows=16, **DET).scan_ragged([x[0], x[1, :320]])
    for name in ("scan_stage_ragged_kernel<false>", "scan_gather_kernel<false, false, true>", "scan_smooth_kernel<false, true>",
                 "scan_suppress_kernel<true>"):
        assert g.has(name), (name, g.entries)
    assert not g.has("scan_stage_ragged_kernel<true>") and not g.has("carry") and not g.has("scan_stage_kernel"), g.entries
    from tests.test_detect_families import MODELS
    fe2, net2 = MODELS["tiny_conv"](emu_lib)
    x2 = Cm.to_dev(emu_lib, segment_audio(2, 2 * fe2.cfg.hop, 80))
    with Log(emu_lib) as g:
        St.StreamingDetector(net2, fe2, 2, max_windows=4, **DET).push_ragged([x2[0], x2[1, :0]])
    assert g.has("scan_gather_kernel<true, true, true>") and g.has("scan_carry_kernel<true, true>"), g.entries
    assert not g.has("scan_carry_kernel<true, false>") and not g.has("scan_carry_kernel<false"), g.entries


def test_push_ragged_argument_errors(emu_lib):
    St = streaming()
    lib = emu_lib
    fe, net, _, _, _ = setup(lib)
    rig = Rig(lib, fe, net, 2, 12, 81, max_windows=16)
    rig.ragged([3, 1])
    dut = rig.dut
    z = lambda n: torch.zeros(n)
    before = dut.state.clone()
    for signals, msg in [([z(320), z(100)], "not a multiple of k \\* hop"), ((z(420), [320, 100]), "not a multiple of k \\* hop"),
                         ((z(320), [640, -320]), "sample_offsets decrease at stream 1"), ([z(0), z(0)], "total_steps == 0"),
                         ((z(320), [320, 320]), "lengths sum to"), ([torch.zeros((1, 320)), z(0)], "1-D"),
                         ([z(320)], "expects 2 signals"), ([z(320), z(0), z(320)], "expects 2 signals"),
                         ((z(640), [640]), "expects 2 signals"), ((torch.zeros((2, 320)), [320, 320]), "packed 1-D")]:
        with pytest.raises(T.TcrError, match=msg):
            dut.push_ragged(signals)
    with pytest.raises(T.TcrError, match="max_windows"):
        St.StreamingDetector(net, fe, 2, max_windows=0).push_ragged([z(320), z(0)])
    # the C entries refuse on their own (status + message) with nothing launched: state, workspace and outputs keep their bytes
    d = dut.det
    ref = dut._call_ref()
    dep = Cm.make_frontend(lib, 640, 320, method="mfcc_deploy")
    buf = torch.full((1 << 16,), 7.0)
    p = buf.data_ptr()
    ws_before = dut._ragged_ws.clone()

    def call(offsets, n=None, ws=None, dc=d, samples=p, k=1, cfg=fe.cfg, state=True, reset=None, model=ref):
        off = np.asarray(offsets, np.int64)
        return lib.tcr_stream_scan_ragged_m(C.byref(cfg), fe.plan.data_ptr(), C.byref(model) if model is not None else None,
                                            len(off) - 1 if n is None else n, off.ctypes.data if len(off) else None, k, C.byref(dc), samples,
                                            reset, dut.state.data_ptr() if state else None, dut._ragged_ws.data_ptr(),
                                            dut._ragged_ws.numel() * 4 if ws is None else ws, p, p, p, p, p, p, None)
    S40 = [0] + [320] * 40
    for args, kw, msg in [(([320, 640, 640],), {}, b"sample_offsets must start at 0"),
                          (([0, 650, 970],), {}, b"length 650 of stream 0 is not a multiple of k * hop = 320"),
                          (([0, 640, 320],), {}, b"sample_offsets decrease at stream 1"),
                          (([0, 0, 0],), {}, b"total_steps == 0"),
                          (([0, 320],), dict(n=0), b"number of streams must be positive"),
                          (([0, 320],), dict(n=-1), b"number of streams must be positive"),
                          ((S40,), dict(ws=512), b"more than the max_signals"),
                          (([],), dict(n=2), b"null argument"),
                          (([0, 320, 320],), dict(samples=None), b"null argument"),
                          (([0, 320, 320],), dict(state=False), b"null argument"),
                          (([0, 320, 320],), dict(model=None), b"null"),
                          (([0, 320, 320],), dict(k=0), b"frames per step"),
                          (([0, 320, 320],), dict(k=50), b"frames per step"),
                          (([0, 320, 320],), dict(cfg=dep.cfg), b"float64 deploy front-end"),
                          (([0, 320, 320],), dict(dc=T._lib.DetectCfg(0, 1, 0, 0.5)), b"average_steps"),
                          (([0, 320, 320],), dict(dc=T._lib.DetectCfg(4, 5, 0, 0.5)), b"min_count")]:
        assert call(*args, **kw) == -1, (args, kw, lib.tcr_last_error())
        assert msg in lib.tcr_last_error(), (args, kw, lib.tcr_last_error())
        assert lib.tcr_last_error().startswith(b"tcr_stream_scan_ragged_m: "), lib.tcr_last_error()
    assert call([0, 320, 320], ws=1024) == -3 and b"one window" in lib.tcr_last_error()       # (TCR_ERR_WORKSPACE, as tcr_scan_ragged)
    # the TC-ResNet entry is the same call
    ss = net.fold_bn()
    off = np.array([0, 0, 0], np.int64)
    assert lib.tcr_stream_scan_ragged(C.byref(fe.cfg), fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), 2, off.ctypes.data, 1,
                                      C.byref(d), p, None, dut.state.data_ptr(), dut._ragged_ws.data_ptr(), dut._ragged_ws.numel() * 4,
                                      p, p, p, p, p, p, None) == -1
    assert lib.tcr_last_error() == b"tcr_stream_scan_ragged: no stream has a whole step (total_steps == 0)"
    bits = lambda t: t.view(torch.int32)
    assert bool((buf == 7.0).all()) and torch.equal(bits(dut.state), bits(before)) and torch.equal(bits(dut._ragged_ws), bits(ws_before))
    rig.ragged([0, 4])
    rig.ragged([2, 2])


def test_ragged_chunks_read_what_packed_reads(tmp_path):
    """The tools' ragged reader (audio_input.Recordings.ragged_chunks): every chunk holds each file's next whole steps, none once it
    has ended, and a file's pieces put together are its part of `packed()`."""
    from tcresnet_amd.audio_input import Recordings
    from tests.test_scan_ragged import write_wav
    rng = np.random.RandomState(82)
    pcm = [rng.randint(-32768, 32767, n).astype(np.int16) for n in (33333, 1000, 12800, 0)]
    wavs = [str(tmp_path / f"{i}.wav") for i in range(len(pcm))]
    for w, x in zip(wavs, pcm):
        write_wav(w, x)
    step = 640
    det = SimpleNamespace(step_samples=step, frontend=SimpleNamespace(cfg=SimpleNamespace(sample_rate=16000)), device=torch.device("cpu"), lib=None)
    rec = Recordings(wavs, det)
    packed, lengths = rec.packed()
    assert lengths == [33280, 640, 12800, 0]
    first = np.concatenate([[0], np.cumsum(lengths)])
    for sec in (0.1, 0.5, 100.0):
        c = int(sec * 16000) // step
        parts = list(rec.ragged_chunks(sec))
        assert [i0 for i0, _, _ in parts] == list(range(0, 52, c))
        pieces = [[] for _ in wavs]
        for i0, buf, lens in parts:
            assert lens == [max(0, min(c * step, n - i0 * step)) for n in lengths] and buf.shape == (sum(lens),) and buf.dtype == torch.float32
            at = 0
            for n, m in enumerate(lens):
                pieces[n].append(buf[at:at + m])
                at += m
        for n in range(len(wavs)):
            assert torch.equal(torch.cat(pieces[n]), packed[first[n]:first[n + 1]]), (sec, n)
    with pytest.raises(SystemExit, match="shorter than one step"):
        list(rec.ragged_chunks(0.01))


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
GPU_DET = dict(average_window_ms=1000, min_count=3, detection_threshold=0.3, suppression_ms=1500)


def gpu_plan(seed, S, hi, calls, never=None):
    """Seeded steps 0..hi per stream and call, with exact zeros in every call and (never) one stream without steps in any."""
    rng = np.random.RandomState(seed)
    plan = rng.randint(0, hi + 1, (calls, S))
    for c in range(calls):
        plan[c, rng.choice(S, max(1, S // 8), replace=False)] = 0
    if never is not None:
        plan[:, never] = 0
    assert (plan == 0).any(axis=1).all() and (plan.max(axis=1) > 0).all()
    return plan.tolist()


def run_gpu_plan(lib, fe, net, plan, seed, k=1, det=GPU_DET, max_windows=(None,)):
    S = len(plan[0])
    total = int(np.sum(plan, axis=0).max())
    rigs = [Rig(lib, fe, net, S, total, seed, k=k, det=det, many=True, max_windows=mw) for mw in max_windows]
    for rig in rigs[1:]:
        rig.oracles = rigs[0].oracles
    for counts in plan:
        xs = rigs[0].take(counts)
        want = rigs[0].want(xs)
        for rig in rigs:
            before = rig.dut.state.clone()
            rig.check(rig.dut.push_ragged(xs), want)
            assert_untouched(rig.dut, before, [s for s, m in enumerate(counts) if m == 0])
    return rigs[0]


@pytest.mark.gpu
def test_gpu_push_ragged_64_streams(hip_lib):
    fe, net, _, _, _ = setup(hip_lib)
    plan = gpu_plan(90, 64, 300, 3, never=11)
    rig = run_gpu_plan(hip_lib, fe, net, plan, 91, max_windows=(512, None))
    assert state_parts(rig.dut)[3][4, 11].item() == 0


@pytest.mark.gpu
def test_gpu_push_ragged_tcresnet14_3010_k2(hip_lib):
    fe, net, _, _, _ = setup(hip_lib, "TCResNet14", 1.5, win=480, hop=160)
    run_gpu_plan(hip_lib, fe, net, gpu_plan(92, 8, 120, 3), 93, k=2, det=dict(GPU_DET, average_window_ms=500, suppression_ms=600))


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["dscnn_s", "tiny_conv"])
def test_gpu_push_ragged_families(hip_lib, model):
    from tests.test_detect_families import MODELS
    fe, net = MODELS[model](hip_lib)
    run_gpu_plan(hip_lib, fe, net, gpu_plan(94, 8, 60, 3), 95, det=dict(GPU_DET, average_window_ms=300, suppression_ms=400))


@pytest.mark.gpu
def test_gpu_push_ragged_planes_write_back_with_surviving_tail(hip_lib):
    planes_write_back_with_surviving_tail(hip_lib)


@pytest.mark.gpu
def test_gpu_cli_ragged_chunk_seconds(hip_lib, tmp_path):
    """scan_audio.py and sweep_audio.py with --ragged_chunk_seconds 1 print what --ragged prints, byte for byte; the flag is
    refused next to --chunk_seconds and next to --ragged."""
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    lengths = [96000, 61234, 20000, 300]                  # the second is written at 48 kHz; the last has no whole step
    wavs = cli_files(tmp_path, lengths, [16000, 48000, 16000, 16000], 51)
    labels = ["_silence_", "_unknown_"] + [f"w{i}" for i in range(10)]
    common = ["--frozen", path, "--wav", *wavs, "--labels", ",".join(labels), "--frames_per_step", "2", "--average_window_ms", "200",
              "--min_count", "2", "--suppression_ms", "400"]
    scan = lambda *extra: [os.path.join(ROOT, "tc-resnet_amd", "scan_audio.py"), *common, "--detection_threshold", "0.3", "--summary", *extra]
    rows = [(wavs[0], 1000, 2000, "w0"), (wavs[0], 4000, 5500, "w3"), (wavs[1], 2000, 3000, "w7"), (wavs[2], 500, 900, "w1")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{a},{b},{c}\n" for f, a, b, c in rows))
    sweep = lambda *extra: [os.path.join(ROOT, "tc-resnet_amd", "sweep_audio.py"), *common, "--events", str(ev_csv), "--thresholds", "0:0.9:0.1",
                            "--tolerance_ms", "500", "--target_fa_per_hour", "1000", "--per_label", *extra]
    new = ("--ragged_chunk_seconds", "1")
    res = run_all([scan("--ragged"), scan(*new), sweep("--ragged"), sweep(*new), scan(*new, "--chunk_seconds", "1"), scan(*new, "--ragged"),
                   sweep(*new, "--chunk_seconds", "1"), sweep(*new, "--ragged")])
    for r in res[:4]:
        assert r[0] == 0, r[2]
    assert len(res[0][1].splitlines()) >= 3 and res[1][1] == res[0][1]
    summary = lambda r: [ln for ln in r[2].splitlines() if ln.startswith("{")]
    assert len(summary(res[0])) == 1 and summary(res[1]) == summary(res[0])
    assert res[1][2] == res[0][2]
    assert len(res[2][1].splitlines()) == 101 and res[3][1] == res[2][1]
    assert res[3][2] == res[2][2] and len(summary(res[2])) == 1
    for r in res[4:]:
        assert r[0] != 0 and r[1] == "" and "--ragged_chunk_seconds" in r[2], r
