"""The event side of detection scoring (sweep_kernel behind tcr_detect_sweep / _ragged / tcr_detect_grid, mine_event_kernel and
mine_classify_kernel behind tcr_mine_detections) on dense and boundary-straddling event layouts (tests/event_layouts.py): several
staging rounds of 256 events per pass, rounds in which exactly 256 finish, events on the first and last step of a pass, one over three
passes, events past the valid steps and past the signal, mining over many workgroups, empty CSR rows, event lengths around the 64-step
probe, labels outside 0 .. C - 1 at the C ABI, non-finite scores.  Every reference is a restated rule that another test file already
owns (`fast_sweep` / `naive_sweep`, `np_rule`, `reference_tables`); everything is integers and bytes and must match exactly.
Emulator (`-m "not gpu"`) and MI355X (`-m gpu`): the checks are functions of `lib` and run on both."""
import functools

import numpy as np
import pytest
import torch

from tcresnet_amd.runtime import stream_of
from tests import common as Cm
from tests.event_layouts import PROBE_LENGTHS, STAGED, alternating_labels, check_layout, event_layouts, three_pass_event
from tests.test_detect_grid import grid_lib, reference_tables
from tests.test_mine import np_rule
from tests.test_scan import scanning
from tests.test_sweep import PASS, check_result, fast_sweep, naive_sweep, sweep_lib, synthetic

NCLS = 4
STEPS = 3 * PASS + 77
VALID = [STEPS, STEPS - 100, PASS, STEPS]               # (the last signal has no events)
N = len(VALID)
SUPPS = (0, 3)
# -inf, +inf, a value the scores hold (they are k / 64), and a linspace: 18 thresholds, two workgroups of them, the second partial
THR = np.concatenate([[-np.inf, np.inf, 0.5], np.linspace(0.02, 0.98, 15)]).astype(np.float32)
SWEEP_LAYOUTS = ["every_step", "every_other", "adjacent_pairs", "adjacent_triples", "n255", "n256", "n257", "n512", "n513", "three_pass",
                 "whole_signal", "probe_lengths"]
WITH_BOUNDARY = ["n255", "n256", "n257", "n512", "n513"]
ONE_STEP = ["every_step", "every_other"]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def grid_scores(rng, shape):
    return (rng.randint(0, 64, size=shape) / 64.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_inputs():
    """top / score [N, STEPS]: signal 0 alternates between two labels on every step (with an event of the first label: a hit, a false
    accept inside the event, a duplicate, over and over), 1 .. 3 are test_sweep's synthetic signals; and per layout the events of signals
    0 .. 2 (signal 3 has none)."""
    rng = np.random.RandomState(71)
    a, b = alternating_labels(NCLS)
    syn_top, syn_score = synthetic(3, STEPS, NCLS, 72)
    top = np.concatenate([np.where(np.arange(STEPS) % 2 == 0, a, b).astype(np.int32)[None], syn_top])
    score = np.concatenate([grid_scores(rng, (1, STEPS)), syn_score])
    per_signal = [event_layouts(STEPS, NCLS, rng) for _ in range(N - 1)]
    events = {name: [per_signal[n][name] for n in range(N - 1)] + [[]] for name in SWEEP_LAYOUTS}
    return top, score, events


def packed(x, valid=VALID):
    """[.., N, STEPS] -> the signals' valid steps one after the other, [.., sum(valid)]."""
    return np.ascontiguousarray(np.concatenate([x[..., n, :v] for n, v in enumerate(valid)], axis=-1))


OFFSETS = np.concatenate([[0], np.cumsum(VALID)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def sweep_reference(name, supp):
    top, score, events = sweep_inputs()
    return fast_sweep(top, score, THR, supp, NCLS, VALID, events[name])


def assert_layout_is_reached(name):
    """The conditions that keep a layout's checks from passing vacuously, on the layout and on the reference's output alone."""
    top, score, events = sweep_inputs()
    evs = events[name]
    for ev in evs:
        check_layout(ev)
    assert any(l >= v for ev, v in zip(evs, VALID) for _, l, _ in ev)                      # events past the valid steps
    refs = [sweep_reference(name, supp) for supp in SUPPS]
    det, hits, dups = (sum(int(r[q].sum()) for r in refs) for q in range(3))
    false_accepts = det - hits - dups
    if name in WITH_BOUNDARY:
        k = int(name[1:])
        for ev in evs[:N - 1]:
            assert len(ev) == k + 4 and all(f == l for f, l, _ in ev[:k]) and [e[0] for e in ev[:k]] == list(range(k))
            assert ev[k][1] == PASS - 1 and ev[k + 1][:2] == (PASS, PASS) and ev[k + 2][:2] == (PASS + 1, 3 * PASS + 5) and ev[k + 3][1] >= STEPS
            # staging rounds of pass 0: full rounds while 256 events finish, then a short one
            in_pass0 = sum(1 for f, _, _ in ev if f < PASS)
            assert in_pass0 == k + 1 and in_pass0 // STAGED + 1 == {255: 2, 256: 2, 257: 2, 512: 3, 513: 3}[k]
    if name in ONE_STEP:
        assert hits > 0 and false_accepts > 0 and dups == 0
    elif name == "adjacent_pairs":                      # two detections in a row never share a label: no duplicate fits in two steps
        assert hits > 0 and false_accepts > 0 and dups == 0
    else:
        assert hits > 0 and dups > 0 and false_accepts > 0, (name, hits, dups, false_accepts)
    if name in WITH_BOUNDARY + ["three_pass"]:
        # the three-pass event: at some threshold a detection of its label in each pass it spans -- a hit and two duplicates or more
        f, l, lab = three_pass_event(STEPS, NCLS)
        assert f // PASS == 1 and l // PASS == 3
        mine = refs[0][3][:, 0].astype(bool) & (top[0] == lab)          # [T, STEPS]: signal 0's detections of the event's label
        parts = [slice(max(f, p * PASS), min(l, (p + 1) * PASS - 1) + 1) for p in (1, 2, 3)]
        assert any(all(mine[t, s].any() for s in parts) for t in range(len(THR)))


# ---- 1, 2. dense and ragged sweeps -----------------------------------------------------------------------------------------------
def check_sweeps(lib, name):
    """The dense call (valid_steps) and the ragged call (the same signals packed by their valid steps) against one reference."""
    top, score, events = sweep_inputs()
    assert_layout_is_reached(name)
    for supp in SUPPS:
        ref = sweep_reference(name, supp)
        res = sweep_lib(lib, top, score, THR, supp, NCLS, events=events[name], valid_steps=VALID, return_fired=True)
        check_result(res, ref)
        rag = sweep_lib(lib, packed(top), packed(score), THR, supp, NCLS, events=events[name], step_offsets=OFFSETS, return_fired=True)
        check_result(rag, ref[:3] + (packed(ref[3]),))


def test_reference_walks_agree_on_dense_layouts():
    """`fast_sweep` stands in for `naive_sweep` above: the two are equal on dense layouts too (short signals: the naive walk is steps x events)."""
    steps = 450
    rng = np.random.RandomState(5)
    a, b = alternating_labels(NCLS)
    syn_top, syn_score = synthetic(1, steps, NCLS, 6)
    top = np.concatenate([np.where(np.arange(steps) % 2 == 0, a, b).astype(np.int32)[None], syn_top])
    score = np.concatenate([grid_scores(rng, (1, steps)), syn_score])
    lay = event_layouts(steps, NCLS, rng)
    thr = [-np.inf, 0.25, 0.5, np.inf]
    for name in ("every_step", "adjacent_triples", "whole_signal"):
        for supp in SUPPS:
            x = naive_sweep(top, score, thr, supp, NCLS, [steps, steps - 100], [lay[name]] * 2)
            y = fast_sweep(top, score, thr, supp, NCLS, [steps, steps - 100], [lay[name]] * 2)
            for p, q in zip(x, y):
                assert np.array_equal(p, q), (name, supp)
            # (a duplicate needs two detections in one event: more than `supp` steps apart)
            assert x[1].sum() > 0 and (x[2].sum() > 0) == (name == "whole_signal" or (name == "adjacent_triples" and supp == 0))


@pytest.mark.parametrize("name", SWEEP_LAYOUTS)
def test_sweep_dense_and_ragged(emu_lib, name):
    check_sweeps(emu_lib, name)


# ---- 3. grid ---------------------------------------------------------------------------------------------------------------------
GRID_POINTS = [(W, mc, supp) for W in (2, 5) for mc in (1, 2) for supp in SUPPS]
GRID_THR = [-np.inf, 0.45, 0.6, 0.75, np.inf]
GRID_LAYOUTS = ["n513", "three_pass", "whole_signal"]


@functools.lru_cache(maxsize=None)
def grid_probs():
    """One-hot-like rows from the sweep's top and score: the top label holds 0.4 + score / 2, the others share the rest (top = -1: a
    uniform row)."""
    top, score, _ = sweep_inputs()
    p = (np.float32(0.4) + np.float32(0.5) * score).astype(np.float32)
    p = np.where(top >= 0, p, np.float32(1.0 / NCLS)).astype(np.float32)
    probs = np.repeat(((np.float32(1) - p) / np.float32(NCLS - 1))[..., None], NCLS, axis=-1).astype(np.float32)
    np.put_along_axis(probs, np.maximum(top, 0)[..., None].astype(np.int64), p[..., None], axis=-1)
    return np.ascontiguousarray(probs)


def check_grid(lib, name):
    _, _, events = sweep_inputs()
    probs = grid_probs()
    want = reference_tables([probs[n, :v] for n, v in enumerate(VALID)], GRID_POINTS, GRID_THR, events[name])
    assert sum(int(w[1].sum()) for w in want) > 0 and sum(int(w[2].sum()) for w in want) > 0
    assert len({np.concatenate([x.ravel() for x in w]).tobytes() for w in want}) >= 4      # the points differ
    got = grid_lib(lib, probs, GRID_POINTS, GRID_THR, events=events[name], valid=VALID)
    for j in range(len(GRID_POINTS)):
        for q in range(3):
            assert np.array_equal(got[q][j], want[j][q]), (name, GRID_POINTS[j], ("detections", "hits", "duplicates")[q])


@pytest.mark.parametrize("name", GRID_LAYOUTS)
def test_grid(emu_lib, name):
    check_grid(emu_lib, name)


# ---- 4. mining -------------------------------------------------------------------------------------------------------------------
MINE_LENS = [0, 700, 0, 2500, 130, 0]                   # empty signals lead, sit in the middle and trail
MINE_OFF = np.concatenate([[0], np.cumsum(MINE_LENS)]).astype(np.int64)
LONG = 3
MINE_LAYOUTS = ["every_step", "whole_signal", "probe_lengths"]


@functools.lru_cache(maxsize=None)
def mine_inputs():
    """Packed top in -1 .. NCLS (both ends are no candidates), is_new at about 0.3, scores on a grid; in the long signal a stretch that
    alternates between two labels and fires on every step, and in front of it a stretch that never fires (an event over it has its first
    matching step several probes in)."""
    rng = np.random.RandomState(81)
    total = int(MINE_OFF[-1])
    top = rng.randint(-1, NCLS + 1, total).astype(np.int32)
    is_new = (rng.rand(total) < 0.3).astype(np.int32)
    score = grid_scores(rng, total)
    a, b = alternating_labels(NCLS)
    lo = int(MINE_OFF[LONG])
    top[lo + 900:lo + 1300] = np.where(np.arange(400) % 2 == 0, a, b)
    is_new[lo + 900:lo + 1300] = 1
    per_signal = [event_layouts(m, NCLS, rng) for m in MINE_LENS]
    f, _, lab = next(e for e in per_signal[LONG]["probe_lengths"] if e[1] - e[0] + 1 == 300)
    is_new[lo + f:lo + f + 100] = 0
    top[lo + f + 100], is_new[lo + f + 100] = lab, 1
    events = {name: [per_signal[n][name] for n in range(len(MINE_LENS))] for name in MINE_LAYOUTS}
    return top, score, is_new, events


def mine_lib(lib, top, score, is_new, offsets, events):
    Sc = scanning()
    dev = Cm.device_of(lib)
    return Sc.mine_detections(torch.from_numpy(top).to(dev), torch.from_numpy(score).to(dev), torch.from_numpy(is_new).to(dev), offsets, NCLS,
                              events, lib)


def assert_mined(md, want, top, score):
    steps, kind, event, hit = want
    assert md.step.cpu().numpy().tolist() == steps.tolist()
    assert md.kind.cpu().numpy().tolist() == kind.tolist()
    assert md.event.cpu().numpy().tolist() == event.tolist()
    assert md.event_hit.cpu().numpy().tolist() == hit.tolist()
    assert np.array_equal(md.label.cpu().numpy(), top[steps]) and np.array_equal(md.value.cpu().numpy(), score[steps])


def check_mining(lib, name):
    """Each layout twice: as it is, and with the long signal's events removed (an empty CSR row between full ones)."""
    top, score, is_new, events = mine_inputs()
    seen_kinds, missed = set(), False
    for drop_long in (False, True):
        evs = [[] if drop_long and n == LONG else ev for n, ev in enumerate(events[name])]
        E = sum(len(ev) for ev in evs)
        assert [len(ev) > 0 for ev in evs] == [False, True, False, not drop_long, True, False]
        want = np_rule(top, is_new, MINE_OFF, evs, NCLS)
        assert_mined(mine_lib(lib, top, score, is_new, MINE_OFF, evs), want, top, score)
        steps, kind, event, hit = want
        seen_kinds |= set(kind.tolist())
        missed |= bool((hit < 0).any())
        if name == "every_step":
            assert E > 4 * 2                            # more than one workgroup of mine_event_kernel (four events each)
            assert (hit < 0).any() and (hit >= 0).any()
        if name == "probe_lengths" and not drop_long:
            flat = [(n, *e) for n, ev in enumerate(evs) for e in ev]
            assert {l - f + 1 for _, f, l, _ in flat} >= set(PROBE_LENGTHS)
            late = [h - (MINE_OFF[n] + f) for (n, f, _, _), h in zip(flat, hit) if h >= 0]
            assert max(late) > 64 and min(late) == 0    # a first matching step several probes in
            assert any(l >= MINE_LENS[n] for n, _, l, _ in flat)       # an event that outruns its signal
            assert ((kind == 0) & (event >= 0)).any() and ((kind == 0) & (event < 0)).any()
    if name != "every_step":                            # (one-step events hold no duplicate)
        assert seen_kinds == {0, 1, 2}
    else:
        assert seen_kinds == {0, 1}
    assert missed or name == "whole_signal"


def test_mining_inputs_hold_every_case():
    """Over the three layouts together: every kind occurs and some events are missed (in the reference)."""
    top, score, is_new, events = mine_inputs()
    assert top.min() == -1 and top.max() == NCLS
    kinds, missed = set(), 0
    for name in MINE_LAYOUTS:
        _, kind, _, hit = np_rule(top, is_new, MINE_OFF, events[name], NCLS)
        kinds |= set(kind.tolist())
        missed += int((hit < 0).sum())
    assert kinds == {0, 1, 2} and missed > 0


@pytest.mark.parametrize("name", MINE_LAYOUTS)
def test_mining(emu_lib, name):
    check_mining(emu_lib, name)


# ---- 5. sweep and mining agree ---------------------------------------------------------------------------------------------------
AGREE_LAYOUTS = ["every_step", "adjacent_triples", "n513", "whole_signal"]
AGREE_THR = [0.25, 0.75]


def check_sweep_and_mining_agree(lib, name, supp=0):
    """Mining with is_new = the reference's fired[t]: its kinds, binned by signal and label, are the device sweep's counts at t."""
    top, score, events = sweep_inputs()
    evs = events[name]
    ref = fast_sweep(top, score, AGREE_THR, supp, NCLS, VALID, evs)
    ptop, pscore = packed(top), packed(score)
    sw = sweep_lib(lib, ptop, pscore, AGREE_THR, supp, NCLS, events=evs, step_offsets=OFFSETS)
    ev_label = np.array([lab for ev in evs for _, _, lab in ev], np.int64)
    sizes = set()
    for t in range(len(AGREE_THR)):
        is_new = packed(ref[3][t]).astype(np.int32)
        md = mine_lib(lib, ptop, pscore, is_new, OFFSETS, evs)
        steps = md.step.cpu().numpy()
        assert steps.tolist() == np.flatnonzero(is_new).tolist()
        sig = np.searchsorted(OFFSETS, steps, side="right") - 1
        got = np.zeros((3, N, NCLS), np.int64)
        np.add.at(got, (md.kind.cpu().numpy().astype(np.int64), sig, ptop[steps]), 1)
        det, hits, dup = (x[:, t].cpu().numpy() for x in (sw.detections, sw.hits, sw.duplicates))
        assert np.array_equal(got[1], hits) and np.array_equal(got[2], dup) and np.array_equal(got.sum(0), det)
        assert np.array_equal(hits, ref[1][:, t]) and np.array_equal(dup, ref[2][:, t])
        hit = md.event_hit.cpu().numpy()
        assert np.array_equal(np.bincount(ev_label[hit >= 0], minlength=NCLS), hits.sum(0))
        assert hits.sum() > 0 and (got[0].sum() > 0) and (dup.sum() > 0 or name == "every_step")
        sizes.add(steps.size)
    assert len(sizes) == 2                              # the thresholds change the detections


@pytest.mark.parametrize("name", AGREE_LAYOUTS)
def test_sweep_and_mining_agree(emu_lib, name):
    check_sweep_and_mining_agree(emu_lib, name)


# ---- 6. labels outside 0 .. C - 1, at the C ABI ----------------------------------------------------------------------------------
def csr(lib, events):
    """The events' CSR packed by hand (the Python wrappers refuse labels outside 0 .. C - 1): device tensors offsets int32 [N + 1],
    first / last int64, label int32."""
    dev = Cm.device_of(lib)
    off = np.concatenate([[0], np.cumsum([len(ev) for ev in events])]).astype(np.int32)
    rows = np.array([e for ev in events for e in ev], np.int64).reshape(-1, 3)
    host = [off, rows[:, 0], rows[:, 1], rows[:, 2].astype(np.int32)]
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host]


def relabel(events):
    """Every third event's label becomes -1 or C, in turn."""
    out = [[(f, l, lab if j % 3 else (-1, NCLS)[(j // 3) % 2]) for j, (f, l, lab) in enumerate(ev)] for ev in events]
    assert {lab for ev in out for _, _, lab in ev} >= {-1, NCLS, 0, NCLS - 1}
    return out


def check_sweep_labels_out_of_range(lib, name="n257", supp=0):
    top, score, events = sweep_inputs()
    evs = relabel(events[name])
    thr = THR[:5]
    ref = fast_sweep(top, score, thr, supp, NCLS, VALID, evs)
    plain = fast_sweep(top, score, thr, supp, NCLS, VALID, events[name], want_fired=False)
    assert ref[1].sum() > 0 and ref[2].sum() > 0 and ref[1].sum() < plain[1].sum() and np.array_equal(ref[0], plain[0])
    dev = Cm.device_of(lib)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_top, d_score, d_valid, d_thr = t(top), t(score), t(np.array(VALID, np.int64)), t(thr)
    ev = csr(lib, evs)
    det, hits, dups = (torch.full((N, len(thr), NCLS), -5, dtype=torch.int32, device=dev) for _ in range(3))
    fired = torch.full((len(thr), N, STEPS), 7, dtype=torch.uint8, device=dev)
    rc = lib.tcr_detect_sweep(N, STEPS, NCLS, d_top.data_ptr(), d_score.data_ptr(), d_valid.data_ptr(), supp, len(thr), d_thr.data_ptr(),
                              *(x.data_ptr() for x in ev), det.data_ptr(), hits.data_ptr(), dups.data_ptr(), fired.data_ptr(), stream_of(dev))
    lib.check(rc, "tcr_detect_sweep")
    for got, want in zip((det, hits, dups, fired), ref):
        assert np.array_equal(got.cpu().numpy(), want)


def check_mining_labels_out_of_range(lib, name="probe_lengths"):
    top, score, is_new, events = mine_inputs()
    evs = relabel(events[name])
    steps, kind, event, hit = np_rule(top, is_new, MINE_OFF, evs, NCLS)
    label = np.array([lab for ev in evs for _, _, lab in ev])
    outside = (label < 0) | (label >= NCLS)
    inside_such = (event >= 0) & outside[np.maximum(event, 0)]
    assert inside_such.any() and not kind[inside_such].any() and (hit[outside] == -1).all() and (hit[~outside] >= 0).any()
    dev = Cm.device_of(lib)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    total, E = int(MINE_OFF[-1]), len(label)
    d_top, d_score, d_new, d_off = t(top), t(score), t(is_new), t(MINE_OFF)
    ev = csr(lib, evs)
    nws = lib.tcr_mine_workspace_bytes(total, 0)
    assert nws > 0
    ws = torch.empty((nws + 3) // 4, dtype=torch.int32, device=dev)
    c_step = torch.full((total,), -5, dtype=torch.int64, device=dev)
    c_label, c_event = (torch.full((total,), -5, dtype=torch.int32, device=dev) for _ in range(2))
    c_value = torch.zeros(total, dtype=torch.float32, device=dev)
    c_kind = torch.full((total,), 9, dtype=torch.uint8, device=dev)
    count, e_hit = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((E,), -5, dtype=torch.int64, device=dev)
    rc = lib.tcr_mine_detections(len(MINE_LENS), d_off.data_ptr(), total, NCLS, d_top.data_ptr(), d_score.data_ptr(), d_new.data_ptr(),
                                 *(x.data_ptr() for x in ev), E, ws.data_ptr(), ws.numel() * 4, c_step.data_ptr(), c_label.data_ptr(),
                                 c_value.data_ptr(), c_kind.data_ptr(), c_event.data_ptr(), count.data_ptr(), e_hit.data_ptr(), stream_of(dev))
    lib.check(rc, "tcr_mine_detections")
    n = int(count.item())
    assert n == steps.size
    assert c_step[:n].cpu().numpy().tolist() == steps.tolist() and c_kind[:n].cpu().numpy().tolist() == kind.tolist()
    assert c_event[:n].cpu().numpy().tolist() == event.tolist() and e_hit.cpu().numpy().tolist() == hit.tolist()
    assert np.array_equal(c_label[:n].cpu().numpy(), top[steps])


def test_sweep_labels_out_of_range(emu_lib):
    check_sweep_labels_out_of_range(emu_lib)


def test_mining_labels_out_of_range(emu_lib):
    check_mining_labels_out_of_range(emu_lib)


# ---- 7. non-finite scores in the sweep -------------------------------------------------------------------------------------------
def check_sweep_non_finite_scores(lib, name="n256"):
    """NaN, +inf and -inf scores at steps inside events: float32 `>` decides (a NaN never fires, +inf fires at every finite threshold
    and at -inf, never at +inf; -inf never fires)."""
    top, score, events = sweep_inputs()
    score = score.copy()
    rng = np.random.RandomState(91)
    inside = np.zeros((N, STEPS), bool)
    for n, ev in enumerate(events[name]):
        for f, l, _ in ev:
            inside[n, f:min(l, VALID[n] - 1) + 1] = True
    pick = inside & (top >= 0) & (rng.rand(N, STEPS) < 0.3)
    what = rng.randint(3, size=(N, STEPS))
    nan, pinf, ninf = (pick & (what == q) for q in range(3))
    score[nan], score[pinf], score[ninf] = np.nan, np.inf, -np.inf
    assert min(int(m.sum()) for m in (nan, pinf, ninf)) > 50
    thr = [-np.inf, 0.5, np.inf]
    for supp in SUPPS:
        ref = fast_sweep(top, score, thr, supp, NCLS, VALID, events[name])
        fired = ref[3].astype(bool)
        assert fired[0][pinf].any() and fired[1][pinf].any() and not fired[2].any()
        assert not fired[:, nan].any() and not fired[:, ninf].any()
        assert ref[1][:, :2].sum() > 0 and ref[2][:, :2].sum() > 0
        res = sweep_lib(lib, top, score, thr, supp, NCLS, events=events[name], valid_steps=VALID, return_fired=True)
        check_result(res, ref)


def test_sweep_non_finite_scores(emu_lib):
    check_sweep_non_finite_scores(emu_lib)


# ---- MI355X ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SWEEP_LAYOUTS)
def test_gpu_sweep_dense_and_ragged(hip_lib, name):
    check_sweeps(hip_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRID_LAYOUTS)
def test_gpu_grid(hip_lib, name):
    check_grid(hip_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MINE_LAYOUTS)
def test_gpu_mining(hip_lib, name):
    check_mining(hip_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", AGREE_LAYOUTS)
def test_gpu_sweep_and_mining_agree(hip_lib, name):
    check_sweep_and_mining_agree(hip_lib, name)


@pytest.mark.gpu
def test_gpu_labels_out_of_range(hip_lib):
    check_sweep_labels_out_of_range(hip_lib)
    check_mining_labels_out_of_range(hip_lib)


@pytest.mark.gpu
def test_gpu_sweep_non_finite_scores(hip_lib):
    check_sweep_non_finite_scores(hip_lib)
