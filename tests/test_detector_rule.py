"""The detector tail (stream_detect_kernel, scan_smooth_kernel, scan_suppress_kernel) against one restatement of its rule
(tests/detector_ref.py), bitwise, on synthetic posteriors at the edges of the suppression walk, of the lane mapping and of the
smoothing loop, and on a small real model for the carried state.  Every check is a function of `lib` and runs on the emulator
(`-m "not gpu"`) and on the MI355X (`-m gpu`); each asserts on the reference side that its inputs reach the edges it is there for."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from tests import common as Cm
from tests import detector_ref as D
from tests.test_detect_grid import bits, np_detect, softmax_rows
from tests.test_scan import scanning
from tests.test_stream_scan import state_parts
from tests.test_streaming import RefDetector, setup, streaming

F = np.float32
NAMES = ("smoothed", "top", "score", "is_new")
PAD = 96                                                # sentinel rows in front of and behind every output


# ---- 1. the restatement agrees with the two older ones --------------------------------------------------------------------------
def test_reference_agrees_with_np_detect_and_ref_detector():
    rng = np.random.RandomState(1)
    edges = set()
    for ncls, W, mc, supp, steps in ((3, 1, 1, 0, 40), (5, 4, 2, 40, 190), (12, 9, 9, 3, 70), (7, 50, 5, 60, 220), (4, 8, 1, 25, 133)):
        probs = softmax_rows(rng, steps, ncls, runs=True)
        thr = float(np.median(probs.max(axis=1))) * 0.8
        want = np_detect(probs, W, mc, supp, thr)
        got = D.detect(probs, W, mc, supp, thr)
        for name, g, w in zip(NAMES, got[:4], want):
            assert np.array_equal(bits(g), bits(w)), (name, ncls, W)
        edges |= got[5]
        # in pieces, with a reset: RefDetector step by step, this reference call by call
        ref = RefDetector(1, W, mc, supp, thr)
        cuts, reset_at = sorted({0, 1, 2, 2 + W, steps // 2, steps // 2 + 1, steps}), steps // 2
        state, pieces = None, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            out = D.detect(probs[a:b], W, mc, supp, thr, state, reset=a == reset_at)
            state = out[4]
            pieces.append(out[:4])
            edges |= out[5]
        step_wise = [ref.step(probs[i:i + 1], reset=(0,) if i == reset_at else ()) for i in range(steps)]
        for q, name in enumerate(NAMES):
            g, w = np.concatenate([p[q] for p in pieces]), np.concatenate([r[q] for r in step_wise])
            assert np.array_equal(bits(g), bits(w)), (name, ncls, W)
        assert state.integers(W) == [ref.n[0] % W, min(ref.n[0], W), ref.prev[0], ref.prev_step[0], ref.n[0]]
        assert np.array_equal(state.ring, np.stack(ref.ring[0]))
    assert D.BRANCHES <= edges and ref.branches <= D.BRANCHES
    assert {"head wraps", "window reads two earlier calls", "suppressed by an earlier call's detection"} <= edges, edges


# ---- the fresh tail through the library --------------------------------------------------------------------------------------------
def padded(n, width, dtype, fill, dev):
    """A sentinel-filled buffer with room for n rows of `width` between two pads -> (buffer, the view of the n rows)."""
    buf = torch.full(((n + 2 * PAD) * width,), fill, dtype=dtype, device=dev)
    return buf, buf[PAD * width:(PAD + n) * width]


def redetect_padded(lib, probs, det, offsets=None, smoothed=True):
    """tcr_detect_redetect on probs [N, steps, C] (offsets given: tcr_detect_redetect_ragged on packed probs [total, C]) with every
    output in the middle of a sentinel-filled buffer -> (smoothed or None, top, score, is_new) as NumPy; both pads are checked."""
    dev = Cm.device_of(lib)
    p = torch.from_numpy(np.ascontiguousarray(probs, F)).to(dev)
    ncls, rows = p.shape[-1], int(np.prod(p.shape[:-1]))
    bufs = [padded(rows, ncls, torch.float32, -7.0, dev), padded(rows, 1, torch.int32, -9, dev), padded(rows, 1, torch.float32, -7.0, dev),
            padded(rows, 1, torch.int32, -9, dev)]
    ptr = [v.data_ptr() for _, v in bufs]
    d = T._lib.DetectCfg(*det)
    if offsets is None:
        rc = lib.tcr_detect_redetect(p.shape[0], p.shape[1], ncls, p.data_ptr(), C.byref(d), ptr[0] if smoothed else None, *ptr[1:], None)
    else:
        off = torch.from_numpy(np.asarray(offsets, np.int64)).to(dev)
        rc = lib.tcr_detect_redetect_ragged(len(offsets) - 1, off.data_ptr(), rows, ncls, p.data_ptr(), C.byref(d),
                                            ptr[0] if smoothed else None, *ptr[1:], None)
    lib.check(rc, "redetect")
    out = []
    for q, ((buf, view), width) in enumerate(zip(bufs, (ncls, 1, 1, 1))):
        host = buf.cpu().numpy()
        fill = host.dtype.type(-7.0 if host.dtype == F else -9)
        assert (host[:PAD * width] == fill).all() and (host[(PAD + rows) * width:] == fill).all(), (NAMES[q], "pad written")
        body = host[PAD * width:(PAD + rows) * width]
        if q == 0 and not smoothed:
            assert (body == fill).all(), "smoothed == NULL: written"
            out.append(None)
        else:
            out.append(body.reshape(p.shape if q == 0 else p.shape[:-1]))
    return out


def same_bits(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        diff = bits(g) != bits(w)
        assert not diff.any(), (what, name, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def check_fresh(lib, signals, det):
    """signals: a list of [steps, C] arrays that share det = (W, min_count, suppression, threshold).  Every signal once as a dense
    call (signals of one length together), with and without `smoothed`, and all of them in one ragged call with signals without
    steps first, last and in between: bitwise the reference, and each ragged signal's rows those of its dense call.  Returns per
    signal the reference's outputs and edges."""
    ref = [D.detect(s, *det) for s in signals]
    by_len = {}
    for n, s in enumerate(signals):
        by_len.setdefault(len(s), []).append(n)
    dense = [None] * len(signals)
    for idx in by_len.values():
        want = [np.stack([ref[n][q] for n in idx]) for q in range(4)]
        got = redetect_padded(lib, np.stack([signals[n] for n in idx]), det)
        same_bits(got, want, ("dense", det, idx))
        same_bits(redetect_padded(lib, np.stack([signals[n] for n in idx]), det, smoothed=False), want, ("dense, no smoothed", det, idx))
        for j, n in enumerate(idx):
            dense[n] = [g[j] for g in got]
    lens = [0]
    for n, s in enumerate(signals):
        lens += [len(s)] + ([0] if n % 2 == 0 else [])
    lens.append(0)
    off = np.concatenate([[0], np.cumsum(lens)])
    packed = np.concatenate(signals)
    for sm in (True, False):
        got = redetect_padded(lib, packed, det, offsets=off, smoothed=sm)
        at = 0
        for n, s in enumerate(signals):
            rows = [None if g is None else g[at:at + len(s)] for g in got]
            same_bits(rows, ref[n][:4], ("ragged", sm, det, n))
            same_bits(rows, dense[n], ("ragged against dense", sm, det, n))
            at += len(s)
    return ref


# ---- 2a. walk geometry ------------------------------------------------------------------------------------------------------------
GEOM = (1, 1, None, 0.5)                                # W = 1, min_count = 1, threshold 0.5; four classes
LONG = 16389                                            # two passes of 8192 steps and five steps


def geometry_rows(labels):
    """labels [steps] (-1: a quiet row of 0.25; a label: 0.7 there and 0.1 elsewhere) -> probs [steps, 4]."""
    labels = np.asarray(labels)
    rows = np.full((len(labels), 4), 0.25, F)
    c = labels >= 0
    rows[c] = F(0.1)
    rows[np.nonzero(c)[0], labels[c]] = F(0.7)
    return rows


def geometry_det(supp):
    return (GEOM[0], GEOM[1], supp, GEOM[3])


def fired(ref):
    return np.nonzero(ref[3])[0].tolist()


def check_walk_lengths(lib):
    lengths = (1, 255, 256, 257, 8191, 8192, 8193, LONG)
    refs = check_fresh(lib, [geometry_rows(np.arange(m) % 2) for m in lengths], geometry_det(0))
    edges = set()
    for m, r in zip(lengths, refs):
        assert r[3].all() and len(r[3]) == m            # every step fires
        assert "fires at the last step" in r[5]
        edges |= r[5]
    assert {"fires at a pass's first step", "fires at a pass's last step", "fires at a probe's last step", "fires in a later pass"} <= edges


def check_walk_lone_candidates(lib):
    at = [0, 255, 256, 8191, 8192, 8193, 16383, 16384, LONG - 1]
    labels = np.full(LONG, -1)
    labels[at] = np.arange(len(at)) % 4
    r, = check_fresh(lib, [geometry_rows(labels)], geometry_det(0))
    assert fired(r) == at
    assert {"fires at a pass's first step", "fires at a pass's last step", "fires at a probe's last step", "fires at the last step",
            "last label fires", "fires in a later pass"} <= r[5], r[5]


def check_walk_suppression_crossings(lib):
    edges = set()
    for supp in (1, 2, 255, 256, 257, 8192, 8193, 20000):
        labels = np.full(LONG, -1)
        labels[8190] = 0
        labels[8191:] = 1 + np.arange(LONG - 8191) % 3
        r, = check_fresh(lib, [geometry_rows(labels)], geometry_det(supp))
        f = fired(r)
        nxt = 8190 + supp + 1
        assert f[0] == 8190 and (f[1] == nxt if nxt < LONG else len(f) == 1), (supp, f[:3])
        assert "suppressed" in r[5]
        edges |= r[5]
    assert {"suppressed across a pass", "suppressed across a probe", "fires at a pass's first step", "fires in a later pass"} <= edges, edges


def check_walk_same_label_runs(lib):
    signals, want = [], []
    for start in (10, 8000):
        for m in (1, 2, 3):
            for r in (-1, 0, 1):
                run = 256 * m + r
                labels = np.full(start + run + 5, -1)
                labels[start:start + run + 1] = 1                   # label a fires, then `run` further candidates of label a
                labels[start + run + 1] = 2                         # label b
                signals.append(geometry_rows(labels))
                want.append([start, start + run + 1])
    refs = check_fresh(lib, signals, geometry_det(0))
    edges = set()
    for r, w in zip(refs, want):
        assert fired(r) == w
        assert "same label" in r[5]
        edges |= r[5]
    assert {"fires behind a probe of its own label", "fires in a later pass"} <= edges, edges


def check_walk_empty_passes(lib):
    only2, gap = np.full(LONG, -1), np.full(LONG, -1)
    only2[[16385, 16387]] = [1, 2]
    gap[[5, 8000, 16386]] = [1, 3, 2]
    a, b = check_fresh(lib, [geometry_rows(only2), geometry_rows(gap)], geometry_det(0))
    assert fired(a) == [16385, 16387] and "first behind passes without candidates" in a[5]
    assert fired(b) == [5, 8000, 16386] and "fires behind a pass without candidates" in b[5]


def test_walk_lengths(emu_lib):
    check_walk_lengths(emu_lib)


def test_walk_lone_candidates(emu_lib):
    check_walk_lone_candidates(emu_lib)


def test_walk_suppression_crossings(emu_lib):
    check_walk_suppression_crossings(emu_lib)


def test_walk_same_label_runs(emu_lib):
    check_walk_same_label_runs(emu_lib)


def test_walk_empty_passes(emu_lib):
    check_walk_empty_passes(emu_lib)


# ---- 2b. class counts and lanes -----------------------------------------------------------------------------------------------------
CLASS_COUNTS = [1, 2, 3, 5, 12, 85, 86, 128, 129, 255, 256]


def check_class_count(lib, ncls):
    """Two signals of 300 steps.  From 255 classes on, the last class dominates steps 100 .. 139 of the first signal."""
    rng = np.random.RandomState(200 + ncls)
    x = rng.randn(2, 300, ncls).astype(F)
    for n in range(2):
        pos = 0
        while pos < 300:
            m = int(rng.randint(3, 40))                         # (runs shorter than the suppression among them)
            x[n, pos:pos + m, rng.randint(ncls)] += rng.uniform(2.0, 4.0)
            pos += m
    if ncls >= 255:
        x[0, 100:140, ncls - 1] += F(9.0)
    e = np.exp(x - x.max(axis=2, keepdims=True))
    probs = (e / e.sum(axis=2, keepdims=True)).astype(F)
    thr = min(1.2 / ncls, 0.9)
    for W in (1, 3):
        refs = check_fresh(lib, [probs[0], probs[1]], (W, min(2, W), 7, thr))
        edges = refs[0][5] | refs[1][5]
        assert int(refs[0][3].sum()) >= 1 and int(refs[1][3].sum()) >= 1
        if ncls >= 2:
            assert {"same label", "suppressed", "new label"} <= edges, edges
        if ncls >= 255:
            assert "last label fires" in refs[0][5] and ncls - 1 in refs[0][1][refs[0][3] == 1]
            assert ("label 255 fires" in refs[0][5]) == (ncls == 256)


@pytest.mark.parametrize("ncls", CLASS_COUNTS)
def test_class_counts(emu_lib, ncls):
    check_class_count(emu_lib, ncls)


# ---- 2c. smoothing ------------------------------------------------------------------------------------------------------------------
WINDOWS = [1, 2, 7, 8, 9, 15, 16, 17, 50, 64, 130, 135]


def check_smoothing(lib, ncls):
    rng = np.random.RandomState(300 + ncls)
    probs = [softmax_rows(rng, 130, ncls, runs=True) for _ in range(2)]
    for W in WINDOWS:
        if W >= 3:
            assert D.order_matters(probs[0], W) and D.order_matters(probs[1], W), W
        for mc in sorted({1, (W + 1) // 2, W}):
            refs = check_fresh(lib, probs, (W, mc, 5, 1.5 / ncls))
            assert ("warming up" in refs[0][5]) == (mc > 1)
            assert int((refs[0][1] == -1).sum()) == min(mc - 1, 130)


@pytest.mark.parametrize("ncls", [5, 12])
def test_smoothing_windows(emu_lib, ncls):
    check_smoothing(emu_lib, ncls)


# ---- 2d. ties, threshold and gate -----------------------------------------------------------------------------------------------------
def check_ties_threshold_gate(lib):
    # two classes with bit-equal smoothed maxima at W = 2 (0.5 + 0.3 and 0.3 + 0.5): the lower index wins
    pair = np.array([[0.1, 0.5, 0.1, 0.3], [0.1, 0.3, 0.1, 0.5]], F)
    tie = np.tile(pair, (3, 1))
    r, = check_fresh(lib, [tie], (2, 1, 0, 0.2))
    assert "tie" in r[5] and r[1].tolist() == [1, 1, 1, 1, 1, 1]
    assert (bits(r[0][1:, 1]) == bits(r[0][1:, 3])).all()
    # ... in the grid's own smoothing kernel as well: at the detector's threshold its detections are the rule's
    grid = scanning().detection_grid(torch.from_numpy(tie[None]).to(Cm.device_of(lib)), [(2, 1, 0)], [0.2], 4, lib=lib)[0]
    assert grid.cpu().numpy().reshape(4).tolist() == np.bincount(r[1][r[3] == 1], minlength=4).tolist() == [0, 1, 0, 0]
    # the threshold is strict
    rows = geometry_rows([-1, 2, -1, 2])
    at = F(0.7)
    r, = check_fresh(lib, [rows], (1, 1, 0, float(at)))
    assert "score equals threshold" in r[5] and fired(r) == []
    r, = check_fresh(lib, [rows], (1, 1, 0, float(np.nextafter(at, F(0)))))
    assert fired(r) == [1]
    # W = 5 with min_count 5: four warm-up rows of -1 / 0
    rng = np.random.RandomState(4)
    r, = check_fresh(lib, [softmax_rows(rng, 12, 6, runs=True)], (5, 5, 0, 0.1))
    assert r[1][:4].tolist() == [-1] * 4 and (r[2][:4] == 0).all() and (r[1][4:] >= 0).all() and fired(r)[0] == 4


def test_ties_threshold_gate(emu_lib):
    check_ties_threshold_gate(emu_lib)


# ---- 4. carried state against the rule ---------------------------------------------------------------------------------------------------
SETTINGS = [(1, 1, 0), (8, 8, 3), (9, 2, 12), (20, 3, 30)]              # W, min_count, suppression in steps
STEP_MS = 20.0                                                          # k = 1 at 640 / 320


def carried_model(lib, ncls, seed):
    """TCResNet8-1.0 at 640 / 320: tests.test_streaming.setup, and its construction with another class count."""
    if ncls == 12:
        return setup(lib, seed=seed)[:2]
    fe = Cm.make_frontend(lib, 640, 320)
    arch = R.make_tcresnet("TCResNet8", 1.0, in_channels=fe.n_coef, num_classes=ncls)
    p, s = R.init_params(arch, seed)
    R.randomize_bn(arch, p, s, seed + 1)
    return fe, Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef, num_classes=ncls)


def mixed_audio(n_streams, n_samples, seed):
    """Quiet noise, loud noise and tones of two levels in segments of 3 .. 13 steps, a different cut per stream: the random nets' top
    class moves within a suppression interval and outside it from the first steps on (tests.test_streaming.segment_audio's moves
    once a second)."""
    rng = np.random.RandomState(seed)
    out = np.zeros((n_streams, n_samples), F)
    for s in range(n_streams):
        pos = 0
        while pos < n_samples:
            m = min(int(rng.randint(3, 14)) * 320, n_samples - pos)
            kind = int(rng.randint(4))
            amp = (0.003, 0.6, 0.3, 0.1)[kind]
            if kind < 2:
                out[s, pos:pos + m] = rng.uniform(-1, 1, m) * amp
            else:
                out[s, pos:pos + m] = amp * np.sin(2 * np.pi * rng.uniform(200, 4000) * np.arange(m) / 16000)
            pos += m
    return out


def carried_plan(W, S):
    """(kind, steps per stream, streams reset in front of the call).  The ragged call leaves streams 0 (mod 4) without steps; stream 0's
    reset is pending through it and applies with the push behind it."""
    rag = [(0, 1, W + 2, 2)[s % 4] for s in range(S)]
    plan = [("push", 1, ()), ("push", 1, ()), ("many", 3, ()), ("many", W - 1, (1,)), ("many", W, ()), ("many", W + 1, ()),
            ("ragged", rag, (0, 2)), ("push", 1, ()), ("many", 2 * W + 3, (S - 1,))]
    return [p for p in plan if p[1]]


def push_plan(W, S):
    """60 single steps, so that stream_detect_kernel meets every branch of the rule, and resets in front of two of them."""
    return [("push", 1, {25: (1,), 40: (0, S - 1)}.get(i, ())) for i in range(60)]


def check_carried(lib, S, ncls, settings, net_seed, seed, plan_of=carried_plan):
    St, Sc = streaming(), scanning()
    fe, net = carried_model(lib, ncls, net_seed)
    step = fe.cfg.hop
    longest = max(sum(max(m) if isinstance(m, list) else m for _, m, _ in plan_of(W, S)) for W, _, _ in settings)
    audio = mixed_audio(S, longest * step, seed)
    x = Cm.to_dev(lib, audio)
    first = Sc.KeywordScanner(net, fe, average_window_ms=STEP_MS, min_count=1, detection_threshold=0.0, suppression_ms=0).scan(x).probs
    first = first.cpu().numpy()
    edges = set()
    for W, mc, supp in settings:
        # the threshold: the median score of a first pass over the same audio, so that candidates and non-candidates both occur
        # (over the first three streams, which every stream count has: the edges they reach do not depend on S)
        scores = np.concatenate([D.detect(first[s], W, mc, supp, 0.0)[2][mc - 1:] for s in range(3)])
        thr = float(np.median(scores))
        det = St.StreamingDetector(net, fe, S, average_window_ms=W * STEP_MS, min_count=mc, detection_threshold=thr,
                                   suppression_ms=supp * STEP_MS)
        assert (det.average_steps, det.suppression_steps) == (W, supp)
        states, pos, pending = [None] * S, [0] * S, set()
        for kind, m, rst in plan_of(W, S):
            per = m if isinstance(m, list) else [m] * S
            if rst:
                det.reset(list(rst))
                pending |= set(rst)
            sig = [x[s, pos[s] * step:(pos[s] + per[s]) * step].contiguous() for s in range(S)]
            if kind == "push":
                out = [t.unsqueeze(1) for t in det.push(torch.stack(sig))]
            elif kind == "many":
                out = list(det.push_many(torch.stack(sig)))
            else:
                r = det.push_ragged(sig)
                out = [[f[0] for f in r.signal(s)] for s in range(S)]
            ints = state_parts(det)[3].cpu().numpy()
            ring = state_parts(det)[2].cpu().numpy()
            for s in range(S):
                o = [f.cpu().numpy() for f in out[s]] if kind == "ragged" else [f[s].cpu().numpy() for f in out]
                assert o[1].shape == (per[s], ncls)
                if per[s]:                                       # (without steps: untouched, and a reset stays pending)
                    ref = D.detect(o[1], W, mc, supp, thr, states[s], reset=s in pending)
                    pending.discard(s)
                    same_bits(o[2:], ref[:4], (kind, W, s))
                    states[s] = ref[4]
                    edges |= ref[5]
                    pos[s] += per[s]
                st = states[s]
                assert ints[:, s].tolist() == st.integers(W), (kind, W, s, ints[:, s].tolist(), st.integers(W))
                for d in range(1, min(st.n, W) + 1):
                    assert np.array_equal(bits(ring[(st.n - d) % W, s]), bits(st.ring[-d])), (kind, W, s, d)
        assert not pending
    return edges


CARRIED_EDGES = D.BRANCHES | {"suppressed by an earlier call's detection", "window reads two earlier calls", "head wraps"}


def test_carried_state_follows_the_rule(emu_lib):
    edges = check_carried(emu_lib, 3, 12, SETTINGS, 2, 70)
    assert CARRIED_EDGES <= edges, CARRIED_EDGES - edges


def test_carried_state_35_classes(emu_lib):
    check_carried(emu_lib, 3, 35, SETTINGS[2:3], 0, 71)


PUSH_EDGES = D.BRANCHES | {"suppressed at the interval's last step", "fires at the first step behind the interval", "head wraps"}


def test_pushes_follow_the_rule(emu_lib):
    edges = check_carried(emu_lib, 3, 12, SETTINGS[2:3], 2, 72, plan_of=push_plan)
    assert PUSH_EDGES <= edges, PUSH_EDGES - edges


def check_tie_in_a_stream(lib):
    """A network whose last layer is zero gives every class the same probability, bit for bit: class 0 wins in a push, in a many-step
    push and in a scan, whatever the window."""
    St = streaming()
    fe, _, arch, p, s = setup(lib)
    p = dict(p)
    p["TCResNet8/fc/weights"] = np.zeros_like(p["TCResNet8/fc/weights"])
    net = Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef)
    x = Cm.to_dev(lib, mixed_audio(2, 12 * fe.cfg.hop, 73))
    det = St.StreamingDetector(net, fe, 2, average_window_ms=9 * STEP_MS, min_count=1, detection_threshold=0.05, suppression_ms=0)
    state = None
    for i in range(3):
        out = [t.cpu().numpy() for t in det.push(x[:, i * 320:(i + 1) * 320].contiguous())]
        assert (bits(out[1]) == bits(out[1])[0, 0]).all()                # (every probability is the same float)
        ref = D.detect(out[1][:1], 9, 1, 0, 0.05, state)
        state = ref[4]
        assert "tie" in ref[5] and ref[1][0] == 0
        for n in range(2):
            same_bits([o[n:n + 1] for o in out[2:]], ref[:4], ("push", i, n))
    out = [t.cpu().numpy() for t in det.push_many(x[:, 3 * 320:].contiguous())]
    ref = D.detect(out[1][0], 9, 1, 0, 0.05, state)
    assert "tie" in ref[5] and (ref[1] == 0).all() and "head wraps" in ref[5]
    for n in range(2):
        same_bits([o[n] for o in out[2:]], ref[:4], ("push_many", n))


def test_tie_in_a_stream(emu_lib):
    check_tie_in_a_stream(emu_lib)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_walk_lengths(hip_lib):
    check_walk_lengths(hip_lib)


@pytest.mark.gpu
def test_gpu_walk_lone_candidates(hip_lib):
    check_walk_lone_candidates(hip_lib)


@pytest.mark.gpu
def test_gpu_walk_suppression_crossings(hip_lib):
    check_walk_suppression_crossings(hip_lib)


@pytest.mark.gpu
def test_gpu_walk_same_label_runs(hip_lib):
    check_walk_same_label_runs(hip_lib)


@pytest.mark.gpu
def test_gpu_walk_empty_passes(hip_lib):
    check_walk_empty_passes(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("ncls", CLASS_COUNTS)
def test_gpu_class_counts(hip_lib, ncls):
    check_class_count(hip_lib, ncls)


@pytest.mark.gpu
@pytest.mark.parametrize("ncls", [5, 12])
def test_gpu_smoothing_windows(hip_lib, ncls):
    check_smoothing(hip_lib, ncls)


@pytest.mark.gpu
def test_gpu_ties_threshold_gate(hip_lib):
    check_ties_threshold_gate(hip_lib)


@pytest.mark.gpu
def test_gpu_carried_state_follows_the_rule(hip_lib):
    edges = check_carried(hip_lib, 23, 12, SETTINGS, 2, 70)
    assert CARRIED_EDGES <= edges, CARRIED_EDGES - edges


@pytest.mark.gpu
def test_gpu_carried_state_35_classes(hip_lib):
    check_carried(hip_lib, 23, 35, SETTINGS[2:3], 0, 71)


@pytest.mark.gpu
def test_gpu_pushes_follow_the_rule(hip_lib):
    edges = check_carried(hip_lib, 23, 12, SETTINGS[2:3], 2, 72, plan_of=push_plan)
    assert PUSH_EDGES <= edges, PUSH_EDGES - edges


@pytest.mark.gpu
def test_gpu_tie_in_a_stream(hip_lib):
    check_tie_in_a_stream(hip_lib)
