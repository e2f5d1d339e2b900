"""Composing labelled test recordings (tcr_compose, tcr_pcm_energy, composing.Composer, compose_audio.py).  Every reference is a
direct NumPy statement of the rule in include/tcresnet_hip.h (`np_compose`, `np_pcm`, np.sum) or existing project code (the input
stage, `gather_clips`, `scan`, `sweep`, `WavFile`); nothing compares the feature with itself, and every comparison is bitwise.
Emulator (`-m "not gpu"`) and MI355X (`-m gpu`) run the same bodies."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_scan_ragged import run_all, scanning
from tests.test_streaming import frozen_artifact, setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = T._lib.COMPOSE_TILE
GAINS = [0.0, 1.0, -1.0, 0.37, 5.0]
_CACHE = {}


def composing():
    from tcresnet_amd import composing as Cp
    return Cp


def make_pool(lib, clips):
    from tcresnet_amd import runtime
    from tcresnet_amd.datasets.augmentation_factory import PcmPool
    runtime.set_default(lib, Cm.device_of(lib))
    try:
        return PcmPool(clips)
    finally:
        runtime.set_default(None, None)


def dev_t(lib, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(Cm.device_of(lib))


# ---- the rule, in NumPy ------------------------------------------------------------------------------------------------------------
def np_pcm(x):
    return np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)     # (np.rint: ties to even)


def np_compose(pcm, bg, t):
    """t: the tables (lengths, po, clip_off, len, first, gain, and bg_off / bg_len / bg_phase / bg_vol or bg_vol None) -> packed float32."""
    off = np.concatenate([[0], np.cumsum(t["lengths"])]).astype(np.int64)
    out = np.zeros(int(off[-1]), np.float32)
    scale = np.float32(1.0 / 32768.0)
    for n, L in enumerate(t["lengths"]):
        L = int(L)
        fg = np.zeros(L, np.float32)
        for j in range(int(t["po"][n]), int(t["po"][n + 1])):
            f, m, c = int(t["first"][j]), int(t["len"][j]), int(t["clip_off"][j])
            lo, hi = max(f, 0), min(f + m, L)
            if hi > lo:
                fg[lo:hi] = (pcm[c + lo - f:c + hi - f].astype(np.float32) * scale) * np.float32(t["gain"][j])
        if t.get("bg_vol") is not None and t["bg_vol"][n] != 0:
            i = np.arange(L, dtype=np.int64)
            b = bg[int(t["bg_off"][n]) + (int(t["bg_phase"][n]) + i) % int(t["bg_len"][n])].astype(np.float32) * scale
            o = b * np.float32(t["bg_vol"][n]) + fg
        else:
            o = fg
        out[off[n]:off[n + 1]] = np.clip(o, np.float32(-1), np.float32(1))
    return out


def raw_compose(lib, pool, bgpool, t, floats=True, pcm=True, guard=4, fill=(7.0, 77)):
    """tcr_compose itself, into buffers with `guard` elements on both sides: (float32 or None, int16 or None); the guards are checked."""
    dev = Cm.device_of(lib)
    off = np.concatenate([[0], np.cumsum(t["lengths"])]).astype(np.int64)
    total, N = int(off[-1]), len(t["lengths"])
    pad = lambda a, dt: dev_t(lib, np.asarray(a, dt) if len(a) else np.zeros(1, dt))
    keep = [pad(off, np.int64), pad(t["po"], np.int32), pad(t["clip_off"], np.int64), pad(t["len"], np.int32), pad(t["first"], np.int64),
            pad(t["gain"], np.float32)]
    mixed = t.get("bg_vol") is not None
    bgt = [pad(t[k], dt) for k, dt in (("bg_off", np.int64), ("bg_len", np.int64), ("bg_phase", np.int64), ("bg_vol", np.float32))] if mixed else []
    fbuf = torch.full((total + 2 * guard,), fill[0], dtype=torch.float32, device=dev) if floats else None
    pbuf = torch.full((total + 2 * guard,), fill[1], dtype=torch.int16, device=dev) if pcm else None
    p = lambda b: None if b is None else b.data_ptr() + guard * b.element_size()
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    lib.check(lib.tcr_compose(N, keep[0].data_ptr(), total, pool.data.data_ptr(), *(x.data_ptr() for x in keep[1:]),
                              bgpool.data.data_ptr() if mixed else None, *([x.data_ptr() for x in bgt] or [None] * 4), p(fbuf), p(pbuf), stream),
              "tcr_compose")
    res = []
    for b, f in ((fbuf, fill[0]), (pbuf, fill[1])):
        if b is None:
            res.append(None)
            continue
        a = b.cpu().numpy()
        assert (a[:guard] == f).all() and (a[guard + total:] == f).all(), "a guard element was written"
        res.append(a[guard:guard + total])
    return res


# ---- 1. the edge table ---------------------------------------------------------------------------------------------------------------
def edge_case(rot):
    """(clips, background recordings, tables).  `rot` rotates which recording gets which background."""
    rng = np.random.RandomState(3 + rot)
    r16 = lambda n: rng.randint(-32768, 32768, n).astype(np.int16)
    clips = [r16(50), np.array([-32768, 32767, -32768, 32767, 12345, -1], np.int16), r16(20), r16(30), r16(10), np.zeros(0, np.int16), r16(10),
             r16(40), r16(2 * TILE + 20), r16(5)] + [r16(3) for _ in range(40)]
    cl = np.array([len(c) for c in clips], np.int64)
    co = np.concatenate([[0], np.cumsum(cl)[:-1]]).astype(np.int64)
    lengths = [0, 1, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 0, 7]
    rows = {n: [] for n in range(len(lengths))}           # per recording: (clip, first, gain)
    rows[1] = [(9, -2, 1.0)]                                                  # longer than the whole recording
    rows[3] = [(0, -10, 0.37), (2, 100, -1.0), (3, 120, 1.0),                 # a negative first; two touching clips;
               (4, 200, 1.0), (5, 215, 1.0), (6, 220, 0.37),                  # a zero-length clip between two others;
               (7, TILE - 1 - 5, 5.0)]                                        # running past the end
    rows[4] = [(10 + k, 10 + 4 * k, GAINS[k % 5]) for k in range(40)]         # 40 clips of 3 samples inside one tile
    rows[5] = [(1, 3, 5.0), (1, 20, 1.0), (1, TILE - 2, -1.0)]                # the extremes, clipped and not
    rows[6] = [(8, -3, 1.0)]                                                  # spans three tiles (and the whole recording)
    rows[8] = [(1, 2, 0.0)]
    po, tab = [0], []
    for n in range(len(lengths)):
        tab += rows[n]
        po.append(len(tab))
    t = dict(lengths=np.array(lengths, np.int64), po=np.array(po, np.int32), clip_off=co[[r[0] for r in tab]], len=cl[[r[0] for r in tab]].astype(np.int32),
             first=np.array([r[1] for r in tab], np.int64), gain=np.array([r[2] for r in tab], np.float32))
    bgs = [r16(1), r16(5), r16(TILE - 1), r16(TILE), r16(TILE + 1), r16(3 * TILE)]
    bl = np.array([len(b) for b in bgs], np.int64)
    bo = np.concatenate([[0], np.cumsum(bl)[:-1]]).astype(np.int64)
    #          recording: 0    1    2    3    4    5    6    7    8
    which = np.roll(np.array([0, 0, 1, 2, 3, 4, 5, 1, 5]), rot)
    last = np.roll(np.array([0, 0, 1, 1, 0, 1, 1, 0, 0]), rot)                # phase bg_len - 1 (else 0)
    vol = np.roll(np.array([0.1, 1.0, 0.1, 0.1, 1.0, 0.1, 0.1, 1.0, 0.0], np.float32), rot)
    t.update(bg_off=bo[which], bg_len=bl[which], bg_phase=np.where(last, bl[which] - 1, 0), bg_vol=vol)
    return clips, bgs, t


def edge_kinds(t):
    """Which of the listed cases the tables hold (read off the tables, not the output)."""
    off = np.concatenate([[0], np.cumsum(t["lengths"])])
    rec = np.repeat(np.arange(len(t["lengths"])), np.diff(t["po"]))
    f, m, L = t["first"], t["len"].astype(np.int64), t["lengths"][rec]
    lo, hi = np.maximum(f, 0), np.minimum(f + m, L)
    same = rec[:-1] == rec[1:]
    kinds = set()
    if ((np.diff(t["po"]) == 0) & (t["lengths"] > 0)).any(): kinds.add("none")
    if ((f < 0) & (f + m > 0)).any(): kinds.add("negative first")
    if ((f < L) & (f + m > L) & (f > 0)).any(): kinds.add("past the end")
    if ((f <= 0) & (f + m >= L) & (m > L)).any(): kinds.add("longer than the recording")
    if (same & (f[:-1] + m[:-1] == f[1:]) & (m[:-1] > 0) & (m[1:] > 0)).any(): kinds.add("touching")
    if (same[:-1] & same[1:] & (m[1:-1] == 0) & (m[:-2] > 0) & (m[2:] > 0)).any(): kinds.add("zero-length between")
    if ((hi > lo) & ((off[rec] + lo) // TILE + 2 <= (off[rec] + hi - 1) // TILE)).any(): kinds.add("three tiles")
    tiles = ((off[rec] + lo) // TILE)[(m == 3) & (hi - lo == 3) & ((off[rec] + lo) // TILE == (off[rec] + hi - 1) // TILE)]
    if tiles.size and np.bincount(tiles).max() >= 40: kinds.add("40 in a tile")
    if set(np.float32(GAINS).tolist()) <= set(t["gain"].tolist()): kinds.add("gains")
    return kinds


ALL_KINDS = {"none", "negative first", "past the end", "longer than the recording", "touching", "zero-length between", "three tiles", "40 in a tile",
             "gains"}


def check_edge_table(lib):
    seen_bg = set()
    for rot in (0, 4):
        clips, bgs, t = edge_case(rot)
        pool, bgpool = make_pool(lib, clips), make_pool(lib, bgs)
        pcm, bg = np.concatenate(clips), np.concatenate(bgs)
        assert edge_kinds(t) == ALL_KINDS, ALL_KINDS - edge_kinds(t)
        assert {-32768, 32767} <= set(pcm[int(t["clip_off"][np.flatnonzero(t["len"] == 6)[0]]):][:6].tolist())
        assert np.cumsum(t["lengths"])[3] % 4 == 3 and np.cumsum(t["lengths"])[1] % 2 == 1       # odd packed offsets
        live = t["lengths"] > 0
        seen_bg |= {(int(a), "last" if p else "first", float(v)) for a, p, v in zip(t["bg_len"][live], t["bg_phase"][live] > 0, t["bg_vol"][live])}
        want = np_compose(pcm, bg, t)
        assert (want == 1.0).any() and (want == -1.0).any() and np.abs(want).max() <= 1.0          # the clip acts
        for run in (0, 1, 3):                           # TCR_TUNE_COMPOSE_RUN: tiles per workgroup (0: the default)
            lib.tcr_tune(34, run)
            try:
                both = raw_compose(lib, pool, bgpool, t)
            finally:
                lib.tcr_tune(34, 0)
            assert np.array_equal(both[0].view(np.int32), want.view(np.int32)) and np.array_equal(both[1], np_pcm(want)), run
        only_f = raw_compose(lib, pool, bgpool, t, pcm=False)
        only_p = raw_compose(lib, pool, bgpool, t, floats=False)
        assert only_f[1] is None and only_p[0] is None
        assert np.array_equal(only_f[0].view(np.int32), want.view(np.int32)) and np.array_equal(only_p[1], np_pcm(want))
        # no background anywhere
        quiet = dict(t, bg_vol=None)
        want_q = np_compose(pcm, bg, quiet)
        got_q = raw_compose(lib, pool, bgpool, quiet)
        assert np.array_equal(got_q[0].view(np.int32), want_q.view(np.int32)) and np.array_equal(got_q[1], np_pcm(want_q))
        assert not np.array_equal(want_q, want)
        # every recording alone is what it is inside the table: no sample depends on a neighbour
        off = np.concatenate([[0], np.cumsum(t["lengths"])])
        for n in np.flatnonzero(live):
            a, b = int(t["po"][n]), int(t["po"][n + 1])
            solo = dict(lengths=t["lengths"][n:n + 1], po=np.array([0, b - a], np.int32), **{k: t[k][a:b] for k in ("clip_off", "len", "first", "gain")},
                        **{k: t[k][n:n + 1] for k in ("bg_off", "bg_len", "bg_phase", "bg_vol")})
            got = raw_compose(lib, pool, bgpool, solo)
            assert np.array_equal(got[0].view(np.int32), want[off[n]:off[n + 1]].view(np.int32)), n
            assert np.array_equal(got[1], np_pcm(want[off[n]:off[n + 1]])), n
    lens = {a for a, _, _ in seen_bg}
    assert lens == {1, 5, TILE - 1, TILE, TILE + 1, 3 * TILE}, lens
    assert {p for _, p, _ in seen_bg} == {"first", "last"} and {v for _, _, v in seen_bg} == {0.0, float(np.float32(0.1)), 1.0}


# ---- 2. against the input stage ------------------------------------------------------------------------------------------------------
def check_input_stage(lib, desired, batch, seed):
    """B recordings of `desired` samples, one clip each at first = shift, the background from its crop on: tcr_augment_fwd on the same
    draws (tests/test_augment.py's)."""
    from tcresnet_amd.datasets import augmentation_factory as F
    from tests.test_augment import _pools
    Cp = composing()
    rng = np.random.RandomState(seed)
    clips, bgs = _pools(rng, desired=desired)
    pool, bgpool = make_pool(lib, clips), make_pool(lib, bgs)
    idx = rng.randint(0, len(clips), batch)
    idx[:6] = np.arange(6)                              # a full clip, a short one, a long one, an empty one, one sample, desired - 1
    shift = rng.randint(-desired // 10, desired // 10, batch).astype(np.int32)
    shift[:4] = [0, -desired // 10, desired // 10 - 1, 7]
    bg_idx = rng.randint(0, len(bgs), batch)
    crop = np.array([rng.randint(0, len(bgs[i]) - desired + 1) for i in bg_idx], np.int64)
    vol = np.where(rng.uniform(size=batch) < 0.7, rng.uniform(0, 0.1, batch), 0.0).astype(np.float32)
    vol[0], vol[1] = 1.0, 0.0
    assert (shift != 0).any() and (vol == 0).any() and (vol > 0).any() and (pool.lengths[idx] == 0).any() and (pool.lengths[idx] < desired).any()
    want = F.anchored_slice_or_pad_with_shift(pool, idx, desired, "wav", 16000, background_data=bgpool, is_training=True,
                                              draws=(shift, bg_idx, crop, vol))[..., 0]
    plan = Cp.CompositionPlan(16000, np.full(batch, desired), np.arange(batch + 1), pool.offsets[idx], np.minimum(pool.lengths[idx], desired),
                              shift, np.ones(batch, np.float32), np.zeros(batch), bgpool.offsets[bg_idx], bgpool.lengths[bg_idx], crop, vol)
    got = Cp.Composer(pool, np.zeros(len(clips)), ["x"], bgpool).compose(plan)
    assert torch.equal(got.signals[0].reshape(batch, desired), want)
    assert (want.abs() == 1.0).any()


# ---- 3. round trip with mining -------------------------------------------------------------------------------------------------------
def small_pool(lib, seed, n=14, ncls=12, amp=32768, lo=3000, hi=9000):
    """Random clips of 0.19 - 0.56 s with labels 2 .. ncls - 1, and two empty ones ("silent" samples, label 0)."""
    rng = np.random.RandomState(seed)
    clips = [rng.randint(-amp, amp, int(m)).astype(np.int16) for m in rng.randint(lo, hi, n)] + [np.zeros(0, np.int16)] * 2
    labels = np.concatenate([2 + np.arange(n) % (ncls - 2), [0, 0]])
    return clips, labels, make_pool(lib, clips)


def check_round_trip(lib):
    Cp, Sc = composing(), scanning()
    clips, labels, pool = small_pool(lib, 5)
    cmp_ = Cp.Composer(pool, labels, [f"c{i}" for i in range(12)])
    plan = cmp_.plan(3, 4.0, 320, min_gap_ms=100, max_gap_ms=400, seed=2)
    assert len(plan.place_len) >= 6 and plan.bg_vol is None and (plan.place_gain == 1).all()
    rec = cmp_.compose(plan, floats=True, pcm=True)
    packed, off = rec.signals[0], plan.sample_offsets
    m = int(plan.place_len.max())
    _, got = Sc.gather_clips(packed, off, plan.place_recording.astype(np.int32), plan.place_first, m, False, True, lib)
    got = got.cpu().numpy()
    for j, c in enumerate(plan.place_clip):
        assert np.array_equal(got[j, :len(clips[c])], clips[c]), j
    L = int(plan.lengths[0])
    _, whole = Sc.gather_clips(packed, off, np.arange(3, dtype=np.int32), np.zeros(3, np.int64), L, False, True, lib)
    assert torch.equal(whole.reshape(-1), rec.pcm)


# ---- 4. energy -----------------------------------------------------------------------------------------------------------------------
def check_energy(lib):
    Cp = composing()
    rng = np.random.RandomState(8)
    lens = [0, 1, 7, 16000, 9, 300001, 16, 15, 33]
    pcm = rng.randint(-32768, 32768, sum(lens) + 3).astype(np.int16)
    off = 3 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)            # odd pool offsets
    assert (off % 2 == 1).any() and (off % 8 != 0).any()
    pcm[off[3]:off[3] + 16000] = -32768                  # the largest sums
    pcm[off[5]:off[5] + 300001] = -32768
    want = np.array([np.sum(pcm[o:o + m].astype(np.int64) ** 2) for o, m in zip(off, lens)], np.int64)
    assert want[5] == 300001 * 2 ** 30
    data = dev_t(lib, pcm)
    got = Cp.pcm_energy(data, off, lens, lib).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want)
    order = rng.permutation(len(lens))                   # the same table in another order: the same per-clip values
    again = Cp.pcm_energy(data, off[order], np.array(lens)[order], lib).cpu().numpy()
    assert np.array_equal(again, want[order])
    assert Cp.pcm_energy(data, [], [], lib).numel() == 0


# ---- 5. the plan ---------------------------------------------------------------------------------------------------------------------
def np_energy(clips):
    return np.array([np.sum(c.astype(np.int64) ** 2) for c in clips], np.int64)


def check_plan(lib):
    Cp = composing()
    clips, labels, pool = small_pool(lib, 6, amp=2000)
    rng = np.random.RandomState(4)
    bgs = [(1000 * (2 * rng.randint(0, 2, m) - 1)).astype(np.int16) for m in (40000, 23456)]     # constant power: every stretch has the mean
    bgpool = make_pool(lib, bgs)
    names = [f"c{i}" for i in range(12)]
    cmp_ = Cp.Composer(pool, labels, names, bgpool)
    secs, step = [10.0, 0.0, 7.3, 12.01], 320
    keys = ("lengths", "place_offsets", "place_clip_off", "place_len", "place_first", "place_gain", "place_label", "bg_off", "bg_len", "bg_phase", "bg_vol")
    a, b, c = (cmp_.plan(4, secs, step, seed=s) for s in (3, 3, 4))
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype for k in keys) and a.events == b.events
    assert not np.array_equal(a.place_first, c.place_first)
    assert a.lengths.tolist() == [int(s * 16000) // step * step for s in secs] and not (a.lengths % step).any()
    assert len(a.place_len) >= 6 and (a.place_len > 0).all() and (a.place_gain == 1).all() and (a.bg_vol == np.float32(0.1)).all()
    assert set(a.place_clip.tolist()) <= set(np.flatnonzero(pool.lengths > 0).tolist())            # empty clips are never placed
    assert np.array_equal(a.place_label, labels[a.place_clip]) and np.array_equal(a.place_clip_off, pool.offsets[a.place_clip])
    for p in (a, c):
        gap = (p.place_first[1:] - (p.place_first + p.place_len)[:-1])[p.place_recording[1:] == p.place_recording[:-1]]
        assert gap.size >= 3 and (gap >= 1.5 * 16000).all() and (gap <= 4.0 * 16000).all()
        assert (p.place_first >= 0).all() and (p.place_first + p.place_len <= p.lengths[p.place_recording]).all()
        assert (p.bg_phase >= 0).all() and (p.bg_phase < p.bg_len).all()
    # the events are the placements' cropped extents
    flat = [(n, *e) for n, evs in enumerate(a.events) for e in evs]
    assert len(flat) == len(a.place_len)
    for j, (n, s, e, lab) in enumerate(flat):
        assert n == a.place_recording[j] and s == 1000.0 * a.place_first[j] / 16000 and lab == a.place_label[j]
        assert e == 1000.0 * (a.place_first[j] + a.place_len[j]) / 16000
    cropped = Cp.CompositionPlan(16000, [100], [0, 2], [0, 0], [50, 80], [-20, 60], [1, 1], [3, 4])
    assert cropped.events == [[(0.0, 1000.0 * 30 / 16000, 3), (1000.0 * 60 / 16000, 1000.0 * 100 / 16000, 4)]]
    only = cmp_.plan(2, 30.0, step, classes=[3, 7], seed=1)
    assert set(only.place_label.tolist()) == {3, 7}
    # snr_db: the float64 formula from NumPy energies
    clip_sq, bg_sq = np_energy(clips), np_energy(bgs)
    got_sq = cmp_.energies()
    assert np.array_equal(got_sq[0], clip_sq) and np.array_equal(got_sq[1], bg_sq) and cmp_.energies() is got_sq
    snr = cmp_.plan(3, 20.0, step, snr_db=10, seed=5)
    which = np.searchsorted(bgpool.offsets, snr.bg_off[snr.place_recording], side="right") - 1
    want = np.sqrt(10.0 ** (10 / 10.0) * float(np.float32(0.1)) ** 2 * (bg_sq[which] / bgpool.lengths[which])
                   * snr.place_len.astype(np.float64) / clip_sq[snr.place_clip]).astype(np.float32)
    assert len(want) >= 6 and np.array_equal(snr.place_gain, want)
    ranged = cmp_.plan(3, 20.0, step, snr_db=(0, 20), seed=5)
    which = np.searchsorted(bgpool.offsets, ranged.bg_off[ranged.place_recording], side="right") - 1
    db = 10 * np.log10(ranged.place_gain.astype(np.float64) ** 2 * clip_sq[ranged.place_clip] / ranged.place_len
                       / (float(np.float32(0.1)) ** 2 * bg_sq[which] / bgpool.lengths[which]))
    assert len(set(ranged.place_gain.tolist())) > 3 and (db > -1e-3).all() and (db < 20 + 1e-3).all() and db.max() - db.min() > 3
    # a zero-energy clip gets gain 1
    zpool = make_pool(lib, [np.zeros(500, np.int16)])
    zplan = Cp.Composer(zpool, [2], names, bgpool).plan(1, 10.0, step, snr_db=10, seed=0)
    assert len(zplan.place_gain) >= 1 and (zplan.place_gain == 1).all()
    # measured: foreground over background power inside each event, from a foreground-only and a background-only render
    fg_only = Cp.CompositionPlan(16000, snr.lengths, snr.place_offsets, snr.place_clip_off, snr.place_len, snr.place_first, snr.place_gain, snr.place_label)
    bg_only = Cp.CompositionPlan(16000, snr.lengths, np.zeros(4, np.int32), [], [], [], [], [], snr.bg_off, snr.bg_len, snr.bg_phase, snr.bg_vol)
    f = cmp_.compose(fg_only).signals[0].cpu().numpy().astype(np.float64)
    g = cmp_.compose(bg_only).signals[0].cpu().numpy().astype(np.float64)
    assert np.abs(f).max() < 0.5 and np.abs(f).max() + np.abs(g).max() < 1.0                      # nothing clips: the definition holds exactly
    mix = cmp_.compose(snr).signals[0].cpu().numpy()
    assert np.array_equal(mix, (g.astype(np.float32) + f.astype(np.float32)))
    for n, evs in enumerate(snr.events):
        for s, e, _ in evs:
            lo, hi = int(snr.sample_offsets[n] + round(s * 16)), int(snr.sample_offsets[n] + round(e * 16))
            db = 10 * np.log10(np.sum(f[lo:hi] ** 2) / np.sum(g[lo:hi] ** 2))
            assert abs(db - 10.0) < 1e-3, (n, s, db)


# ---- 6. into the pipeline ------------------------------------------------------------------------------------------------------------
def check_pipeline(lib):
    Cp, Sc = composing(), scanning()
    fe, net, _, _, _ = setup(lib)
    sc = Sc.KeywordScanner(net, fe, average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=40)
    clips, labels, pool = small_pool(lib, 7)
    rng = np.random.RandomState(2)
    bgs = [rng.randint(-3000, 3000, 30001).astype(np.int16)]
    bgpool = make_pool(lib, bgs)
    cmp_ = Cp.Composer(pool, labels, [f"c{i}" for i in range(12)], bgpool)
    plan = cmp_.plan(3, [6.0, 0.01, 5.0], sc.step_samples, seed=11)
    assert plan.lengths.tolist() == [96000, 0, 80000] and len(plan.place_len) >= 3
    rec = cmp_.compose(plan, floats=True, pcm=True)
    out = sc.scan_ragged(rec.signals)
    want = np_compose(np.concatenate(clips), np.concatenate(bgs),
                      dict(lengths=plan.lengths, po=plan.place_offsets, clip_off=plan.place_clip_off, len=plan.place_len, first=plan.place_first,
                           gain=plan.place_gain, bg_off=plan.bg_off, bg_len=plan.bg_len, bg_phase=plan.bg_phase, bg_vol=plan.bg_vol))
    for n in (0, 2):
        a, b = int(plan.sample_offsets[n]), int(plan.sample_offsets[n + 1])
        solo = sc.scan(Cm.to_dev(lib, want[a:b])[None])
        for x, y in zip(out.signal(n), solo):
            assert torch.equal(x, y), n
    res = sc.sweep(out, [0.0, 0.5], events=rec.events)                    # the default tolerance with the default gaps: no overlap refusal
    counts = np.zeros((3, 12), np.int64)
    np.add.at(counts, (plan.place_recording, plan.place_label), 1)
    assert np.array_equal(res.events, counts) and counts.sum() == len(plan.place_len)
    mined = sc.mine(out, rec.signals, rec.events, k=4, kinds=("false_accept", "hit", "miss"), pcm=True)
    assert len(mined) >= 1
    again = Cp.Composer(mined.to_pool(), mined.label, cmp_.label_names, bgpool)
    replan = again.plan(1, 8.0, sc.step_samples, snr_db=5, seed=1)
    redo = again.compose(replan)
    assert len(replan.place_len) >= 1 and redo.signals[0].shape[0] == 8 * 16000 and bool(torch.isfinite(redo.signals[0]).all())


# ---- 7. the command line -------------------------------------------------------------------------------------------------------------
def wav_tree(root):
    """3 labels x 4 clips of 0.3 - 1 s and one 2.5 s noise file, as the dataset loader reads them."""
    from tcresnet_amd.audio_input import write_wav
    rng = np.random.RandomState(12)
    for label in ("left", "right", "stop"):
        os.makedirs(os.path.join(root, "valid", label))
        for i in range(4):
            write_wav(os.path.join(root, "valid", label, f"{i}.wav"), rng.randint(-20000, 20000, rng.randint(4800, 16001)).astype(np.int16), 16000)
    os.makedirs(os.path.join(root, "valid", "_background_noise_"))
    write_wav(os.path.join(root, "valid", "_background_noise_", "noise.wav"), rng.randint(-8000, 8000, 40000).astype(np.int16), 16000)


CLI = ["--dataset_split_name", "valid", "--num_recordings", "3", "--seconds", "6", "--min_gap_ms", "1200", "--max_gap_ms", "2000", "--seed", "4",
       "--snr_db", "3:9"]


def check_cli_output(lib, out_dir, stdout, stderr, data_dir):
    """compose_audio.py's files against the API's run of the same plan."""
    from tcresnet_amd import compose_audio, runtime
    from tcresnet_amd.audio_input import WavFile
    Cp = composing()
    runtime.set_default(lib, Cm.device_of(lib))
    try:
        args = compose_audio.check_arguments(compose_audio.parse_arguments(["--dataset_path", data_dir, "--output_dir", out_dir, *CLI]))
        cmp_ = Cp.Composer.from_dataset(compose_audio.open_dataset(args))
    finally:
        runtime.set_default(None, None)
    assert cmp_.label_names == ["__null__", "left", "right", "stop"] and len(cmp_.pool) == 12 and len(cmp_.background) == 1
    plan = cmp_.plan(3, 6.0, 320, min_gap_ms=1200, max_gap_ms=2000, snr_db=(3.0, 9.0), seed=4)
    rec = cmp_.compose(plan, floats=False, pcm=True)
    assert rec.signals is None and len(plan.place_len) >= 4
    pcm = rec.pcm.cpu().numpy()
    wavs = [os.path.join(out_dir, f"rec_{n:04d}.wav") for n in range(3)]
    assert stdout.split() == wavs + [os.path.join(out_dir, "events.csv")]
    for n, path in enumerate(wavs):
        wav = WavFile(path)
        assert (wav.rate, wav.channels, wav.length) == (16000, 1, 96000)
        assert wav.read_pcm(0, wav.length).tobytes() == pcm[n * 96000:(n + 1) * 96000].tobytes()
    with open(os.path.join(out_dir, "events.csv"), newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert list(rows[0]) == ["file", "start_ms", "end_ms", "label"]
    got = [[] for _ in wavs]
    for r in rows:
        got[wavs.index(r["file"])].append((float(r["start_ms"]), float(r["end_ms"]), cmp_.label_names.index(r["label"])))
    assert got == plan.events
    info = json.loads(stderr.strip().splitlines()[-1])
    assert info["recordings"] == 3 and info["seconds"] == 18.0 and sum(info["events"].values()) == len(plan.place_len)
    assert info["events"] == {k: [cmp_.label_names[l] for l in plan.place_label].count(k) for k in info["events"]}
    return wavs, len(plan.place_len)


def test_compose_audio_flags_are_refused():
    from tcresnet_amd import compose_audio
    base = ["--dataset_path", "d", "--output_dir", "o", "--num_recordings", "2", "--seconds", "3"]
    for extra, msg in [(["--num_recordings", "0"], "--num_recordings"), (["--min_gap_ms", "0"], "--min_gap_ms"), (["--max_gap_ms", "100"], "--max_gap_ms"),
                       (["--snr_db", "9:3"], "--snr_db"), (["--snr_db", "loud"], "--snr_db"), (["--step_samples", "0"], "step of 0 samples")]:
        with pytest.raises(SystemExit, match=msg):
            compose_audio.check_arguments(compose_audio.parse_arguments(base + extra))
    args = compose_audio.check_arguments(compose_audio.parse_arguments(base + ["--frames_per_step", "2", "--snr_db", "5"]))
    assert args.step_samples == 640 and args.snr_db == 5.0 and args.dataset_split_name == "valid"


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    Cp = composing()
    dev = Cm.device_of(lib)
    err = lambda: lib.tcr_last_error().decode()
    p = lambda t: None if t is None else t.data_ptr()
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)
    pcm = torch.zeros(64, dtype=torch.int16, device=dev)
    off, po, co, ln, first = i64(0, 16), torch.tensor([0, 1], dtype=torch.int32, device=dev), i64(0), torch.tensor([8], dtype=torch.int32, device=dev), i64(2)
    gain, vol = torch.ones(1, device=dev), torch.ones(1, device=dev)
    out, out_pcm = torch.full((24,), 7.0, device=dev), torch.full((24,), 77, dtype=torch.int16, device=dev)
    base = dict(n=1, off=off, total=16, pcm=pcm, po=po, co=co, ln=ln, first=first, gain=gain, bg=pcm, bg_off=i64(0), bg_len=i64(4), bg_phase=i64(0),
                vol=vol, out=p(out), out_pcm=p(out_pcm))

    def call(**kw):
        a = dict(base, **kw)
        ptr = lambda k: a[k] if isinstance(a[k], int) or a[k] is None else a[k].data_ptr()
        return lib.tcr_compose(a["n"], ptr("off"), a["total"], *(ptr(k) for k in ("pcm", "po", "co", "ln", "first", "gain", "bg", "bg_off", "bg_len",
                                                                                   "bg_phase", "vol", "out", "out_pcm")), None)

    for k in ("off", "pcm", "po", "co", "ln", "first", "gain"):
        assert call(**{k: None}) == -1 and "tcr_compose: null argument" in err(), k
    assert call(n=0) == -1 and "number of signals must be positive (got 0)" in err()
    assert call(total=-1) == -1 and "total_samples must be >= 0 (got -1)" in err()
    assert call(out=None, out_pcm=None) == -1 and "out and out_pcm are both null" in err()
    for k in ("bg", "bg_off", "bg_len", "bg_phase"):
        assert call(**{k: None}) == -1 and "bg_vol given without bg / bg_off / bg_len / bg_phase" in err(), k
    assert call(out=p(out) + 4) == -1 and "out must be 16-byte aligned" in err()
    assert call(out_pcm=p(out_pcm) + 2) == -1 and "out_pcm must be 8-byte aligned" in err()
    assert call(total=2 ** 31 * TILE + 1) == -1 and "samples are too many for one launch" in err()
    assert call(total=0) == 0
    assert bool((out == 7.0).all()) and bool((out_pcm == 77).all())                     # nothing was launched
    assert call() == 0 and call(vol=None, bg=None, bg_off=None, bg_len=None, bg_phase=None) == 0
    assert bool((out[:16] == 0).all()) and bool((out[16:] == 7.0).all()) and bool((out_pcm[16:] == 77).all())
    sq = torch.full((2,), 5, dtype=torch.int64, device=dev)
    en = lambda pcm_=pcm, o=co, m=i64(8), n=1, s=sq: lib.tcr_pcm_energy(p(pcm_), p(o), p(m), n, p(s), None)
    assert en(n=-1) == -1 and "tcr_pcm_energy: n_clips must be >= 0 (got -1)" in err()
    for kw in (dict(pcm_=None), dict(o=None), dict(m=None), dict(s=None)):
        assert en(**kw) == -1 and "tcr_pcm_energy: null argument" in err()
    assert en(n=2 ** 31) == -1 and "clips are too many for one launch" in err()
    assert en(n=0) == 0 and sq.tolist() == [5, 5]
    assert en() == 0 and sq.tolist() == [0, 5]
    # the Python layer
    plan = lambda first, ln_, gain_=(1, 1): Cp.CompositionPlan(16000, [100, 100], [0, 0, 2], [0, 0], ln_, first, gain_, [2, 3])
    with pytest.raises(T.TcrError, match=r"recording 1: placements 0 \(samples 10 .. 29\) and 1 \(from 29\) overlap or are not sorted"):
        plan([10, 29], [20, 5])
    with pytest.raises(T.TcrError, match="recording 1: placements 0 .* overlap or are not sorted"):
        plan([50, 10], [5, 5])
    plan([10, 30], [20, 5])                             # touching is allowed
    with pytest.raises(T.TcrError, match="recording 1: placement 1 has a gain that is not finite"):
        plan([10, 30], [20, 5], (1, float("nan")))
    with pytest.raises(T.TcrError, match="recording 0: a background volume that is not finite"):
        Cp.CompositionPlan(16000, [100], [0, 0], [], [], [], [], [], [0], [5], [0], [float("inf")])
    with pytest.raises(T.TcrError, match="recording 0: background of 5 samples at phase 5"):
        Cp.CompositionPlan(16000, [100], [0, 0], [], [], [], [], [], [0], [5], [5], [0.5])
    clips, labels, pool = small_pool(lib, 9, n=4)
    names = [f"c{i}" for i in range(12)]
    bare = Cp.Composer(pool, labels, names)
    with pytest.raises(T.TcrError, match="snr_db needs a background pool"):
        bare.plan(1, 5.0, 320, snr_db=10)
    with pytest.raises(T.TcrError, match="snr_db needs a background pool"):
        Cp.Composer(pool, labels, names, make_pool(lib, [np.ones(100, np.int16)])).plan(1, 5.0, 320, snr_db=10, background_volume=0.0)
    for kw in (dict(min_gap_ms=0), dict(min_gap_ms=-5), dict(min_gap_ms=2000, max_gap_ms=1999)):
        with pytest.raises(T.TcrError, match="0 < min_gap_ms <= max_gap_ms"):
            bare.plan(1, 5.0, 320, **kw)
    with pytest.raises(T.TcrError, match="no clip with samples"):
        bare.plan(1, 5.0, 320, classes=[0])
    with pytest.raises(T.TcrError, match="the pool is on"):
        Cp.Composer(pool, labels, names, device="cpu" if dev.type == "cuda" else "cuda")
    with pytest.raises(T.TcrError, match="lies outside the pool"):
        bare.compose(Cp.CompositionPlan(16000, [100], [0, 1], [int(pool.data.shape[0]) - 3], [8], [0], [1], [2]))
    with pytest.raises(T.TcrError, match="no background pool"):
        bare.compose(Cp.CompositionPlan(16000, [100], [0, 0], [], [], [], [], [], [0], [5], [0], [0.5]))
    with pytest.raises(T.TcrError, match="without pcm=True"):
        bare.compose(bare.plan(1, 1.0, 320)).write_wavs("unused")


# ---- emulator ------------------------------------------------------------------------------------------------------------------------
def test_compose_edge_table_equals_rule(emu_lib):
    check_edge_table(emu_lib)


@pytest.mark.parametrize("desired,batch", [(16000, 12), (1003, 9)])
def test_compose_equals_input_stage(emu_lib, desired, batch):
    check_input_stage(emu_lib, desired, batch, desired)


def test_compose_round_trip_with_gather(emu_lib):
    check_round_trip(emu_lib)


def test_pcm_energy_equals_numpy(emu_lib):
    check_energy(emu_lib)


def test_plan_draws_events_and_snr(emu_lib):
    check_plan(emu_lib)


def test_composed_recordings_through_scan_sweep_mine(emu_lib):
    check_pipeline(emu_lib)


def test_compose_audio_writes_what_the_api_composes(emu_lib, tmp_path, capsys):
    from tcresnet_amd import compose_audio, runtime
    data, out_dir = str(tmp_path / "data"), str(tmp_path / "out")
    wav_tree(data)
    runtime.set_default(emu_lib, "cpu")
    try:
        assert compose_audio.main(compose_audio.parse_arguments(["--dataset_path", data, "--output_dir", out_dir, *CLI])) == 0
    finally:
        runtime.set_default(None, None)
    cap = capsys.readouterr()
    check_cli_output(emu_lib, out_dir, cap.out, cap.err, data)


def test_compose_refusals(emu_lib):
    check_refusals(emu_lib)


# ---- MI355X --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_compose_edge_table_equals_rule(hip_lib):
    check_edge_table(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("desired,batch", [(16000, 12), (1003, 9)])
def test_gpu_compose_equals_input_stage(hip_lib, desired, batch):
    check_input_stage(hip_lib, desired, batch, desired)


@pytest.mark.gpu
def test_gpu_compose_round_trip_and_energy(hip_lib):
    check_round_trip(hip_lib)
    check_energy(hip_lib)


@pytest.mark.gpu
def test_gpu_plan_draws_events_and_snr(hip_lib):
    check_plan(hip_lib)


@pytest.mark.gpu
def test_gpu_composed_recordings_through_scan_sweep_mine(hip_lib):
    check_pipeline(hip_lib)


@pytest.mark.gpu
def test_gpu_compose_refusals(hip_lib):
    check_refusals(hip_lib)


@pytest.mark.gpu
def test_gpu_compose_audio_into_sweep_audio(hip_lib, tmp_path):
    data, out_dir = str(tmp_path / "data"), str(tmp_path / "out")
    wav_tree(data)
    script = os.path.join(ROOT, "tc-resnet_amd", "compose_audio.py")
    (code, so, se), = run_all([[script, "--dataset_path", data, "--output_dir", out_dir, *CLI]])
    assert code == 0, se
    wavs, placed = check_cli_output(hip_lib, out_dir, so, se, data)
    fe, net, _, _, _ = setup(hip_lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    labels = ["__null__", "left", "right", "stop"] + [f"w{i}" for i in range(8)]
    sweep = os.path.join(ROOT, "tc-resnet_amd", "sweep_audio.py")
    (code, so, se), = run_all([[sweep, "--frozen", path, "--wav", *wavs, "--events", os.path.join(out_dir, "events.csv"), "--ragged", "--labels",
                                ",".join(labels), "--keywords", "left,right,stop", "--thresholds", "0.2,0.5", "--per_label"]])
    assert code == 0, se
    rows = list(csv.DictReader(so.splitlines()))
    assert len(rows) == 6 and sum(int(r["events"]) for r in rows if r["threshold"] == "0.5") == placed
