"""Reverberation (tcr_reverb, reverberation.py, Composer.reverberated, compose_audio.py --rir_*).  The reference is tests/reverb_ref.py:
the rule of include/tcresnet_hip.h in NumPy, bitwise on a fixed-point grid of responses, an int64 sum for integer rows and the float64
dot product with the fmaf-chain bound for arbitrary responses; the layers above are compared with the project's own NumPy rules
(`np_compose`, oracle.augment_ref) applied to the reference's wet clips.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`) run the
same bodies; the emulator also runs the workgroups last to first."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests import reverb_configs as Rc
from tests import reverb_ref as Rr

TILE, STAGE, MAX = Rc.T, Rc.D, Rc.MAX
POISON_F, POISON_P = 7.0, 77


def reverberation():
    from tcresnet_amd import reverberation as Rv
    return Rv


def make_pool(lib, clips):
    from tests.test_compose import make_pool as mk
    return mk(lib, clips)


def dev_t(lib, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(Cm.device_of(lib))


# ---- the call, into guarded buffers -------------------------------------------------------------------------------------------------
def raw_reverb(lib, xs, hs, clip_ir, ms, fmt="i16", outs="both", in_off=None, ir_off=None, guard=5, seed=0):
    """tcr_reverb itself.  xs: int16 clips (fmt "f32": passed decoded), hs: float32 responses, clip j under hs[clip_ir[j]] with ms[j]
    outputs; in_off / ir_off: where each clip / response starts in its buffer (default: packed), the rest of the buffers is finite
    garbage.  Outputs into buffers with `guard` poisoned elements on both sides, which are checked.  -> (float32 | None, int16 | None)."""
    dev = Cm.device_of(lib)
    rng = np.random.RandomState(1000 + seed)
    n = np.array([len(x) for x in xs], np.int64)
    L = np.array([len(h) for h in hs], np.int64)
    in_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if in_off is None else np.asarray(in_off, np.int64)
    ir_off = np.concatenate([[0], np.cumsum(L)[:-1]]).astype(np.int64) if ir_off is None else np.asarray(ir_off, np.int64)
    size = int((in_off + n).max()) + 3 if len(xs) else 3
    pool = rng.randint(-30000, 30000, size).astype(np.int16)
    pool[pool == 0] = 11
    for o, x in zip(in_off, xs):
        pool[o:o + len(x)] = x
    data = pool if fmt == "i16" else Rr.decode(pool)
    bank = np.full(int((ir_off + L).max()) + 2, 0.8125, np.float32)
    for o, h in zip(ir_off, hs):
        bank[o:o + len(h)] = h
    ms = np.asarray(ms, np.int64)
    out_off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    tile_off = np.concatenate([[0], np.cumsum((ms + TILE - 1) // TILE)]).astype(np.int64)
    total = int(out_off[-1])
    keep = [dev_t(lib, a) for a in (data, in_off, n, bank, ir_off, L.astype(np.int32), np.asarray(clip_ir, np.int32), out_off, tile_off)]
    fbuf = torch.full((total + 2 * guard,), POISON_F, dtype=torch.float32, device=dev) if outs in ("f", "both") else None
    pbuf = torch.full((total + 2 * guard,), POISON_P, dtype=torch.int16, device=dev) if outs in ("p", "both") else None
    p = lambda b: None if b is None else b.data_ptr() + guard * b.element_size()
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    lib.check(lib.tcr_reverb(len(xs), keep[0].data_ptr(), 1 if fmt == "i16" else 0, int(data.size), keep[1].data_ptr(), keep[2].data_ptr(),
                             keep[3].data_ptr(), int(bank.size), keep[4].data_ptr(), keep[5].data_ptr(), keep[6].data_ptr(), keep[7].data_ptr(),
                             keep[8].data_ptr(), int(tile_off[-1]), p(fbuf), p(pbuf), stream), "tcr_reverb")
    res = []
    for b, f in ((fbuf, POISON_F), (pbuf, POISON_P)):
        if b is None:
            res.append(None)
            continue
        a = b.cpu().numpy()
        assert (a[:guard] == f).all() and (a[guard + total:] == f).all(), "a guard element was written"
        res.append(a[guard:guard + total])
    return res


def row_inputs(row):
    """The row's clips and responses: responses on the grid of reverb_ref, clips over the whole int16 range; a loud row: full scale
    against all-ones responses."""
    rng = np.random.RandomState(100 + row.seed + len(row.clips) + int(row.n.sum() % 97))
    xs, hs = [], []
    for j, (n, L) in enumerate(zip(row.n, row.L)):
        if row.loud:
            xs.append(np.full(n, 32767 if j % 2 == 0 else -32768, np.int16))
            hs.append(np.ones(L, np.float32))
        else:
            xs.append(rng.randint(-32768, 32768, int(n)).astype(np.int16))
            hs.append(Rr.grid_response(rng, int(L), 1.0 if L < 64 else 0.25))
    return xs, hs


def subset(n, L, m, rng, cap=4096):
    """Every output, or for m > cap at most cap of them: the first and last 17 of every tile and of the clip, the chain's edges
    L - 2, L - 1, L, n - 1, n, n + L - 2, and random ones."""
    if m <= cap:
        return np.arange(m, dtype=np.int64)
    must = [np.arange(17), np.arange(m - 17, m), np.array([L - 2, L - 1, L, n - 1, n, n + L - 2])]
    for t0 in range(0, m, TILE):
        must += [np.arange(t0, t0 + 17), np.arange(t0 + TILE - 17, t0 + TILE)]
    must = np.unique(np.concatenate(must))
    must = must[(must >= 0) & (must < m)]
    assert must.size <= cap
    extra = rng.randint(0, m, cap - must.size)
    return np.unique(np.concatenate([must, extra])).astype(np.int64)


def check_row(lib, row):
    xs, hs = row_inputs(row)
    f, p = raw_reverb(lib, xs, hs, np.arange(len(xs)), row.m, row.fmt, row.outs, row.in_off, row.ir_off, seed=row.seed)
    rng = np.random.RandomState(7)
    rails = set()
    for j, (x, h) in enumerate(zip(xs, hs)):
        a, m = int(row.out_off[j]), int(row.m[j])
        idx = subset(len(x), len(h), m, rng)
        want = Rr.chain(x, h, idx)
        if f is not None:
            assert np.array_equal(f[a:a + m][idx].view(np.int32), want.view(np.int32)), (row.name, j)
        if p is not None:
            assert np.array_equal(p[a:a + m][idx], Rr.np_pcm(want)), (row.name, j)
        rails |= set(Rr.np_pcm(want).tolist()) & {-32768, 32767}
        if row.loud:
            assert np.abs(want).max() > 1.0
        if m > len(x) + len(h) - 1:
            assert not want[idx >= len(x) + len(h) - 1].any() and (idx.size < m or (idx >= len(x) + len(h) - 1).sum() == m - (len(x) + len(h) - 1))
        if idx.size < m and f is not None:              # a long row: every output within the chain's bound of the float64 convolution
            y, bound = Rr.dot64(x, h, m)
            assert (np.abs(f[a:a + m].astype(np.float64) - y) <= bound).all(), (row.name, j)
    if row.loud:
        assert rails == {-32768, 32767}                 # (asserted on the reference: both rails are reached)


# ---- exact integer rows -------------------------------------------------------------------------------------------------------------
def check_integer_rows(lib):
    """Integer taps and small |pcm|: every partial sum S of h pcm stays below 2^24, so y = S / 32768 exactly whatever the order."""
    rng = np.random.RandomState(21)
    for n, L, fmt in ((5000, 700, "i16"), (TILE + 3, 33, "f32"), (40, STAGE + 5, "i16")):
        x = rng.randint(-15, 16, n).astype(np.int16)
        h = rng.randint(-3, 4, L).astype(np.float32)
        x[:3], h[0] = [15, -15, 7], 3.0
        if fmt == "i16":                                # a stretch that saturates the int16 output at both rails
            x[20:20 + 8] = [32767, 0, 0, 0, -32768, 0, 0, 0]
        S = np.convolve(x.astype(np.int64), h.astype(np.int64))
        assert np.abs(np.convolve(np.abs(x).astype(np.int64), np.abs(h).astype(np.int64))).max() < 2 ** 24
        f, p = raw_reverb(lib, [x], [h], [0], [n + L - 1], fmt, "both", [3], [1])
        assert np.array_equal(f.view(np.int32), (S.astype(np.float64) / 32768.0).astype(np.float32).view(np.int32)), (n, L)
        assert np.array_equal(p, np.clip(S, -32768, 32767).astype(np.int16)), (n, L)
        if fmt == "i16":
            assert {-32768, 32767} <= set(p.tolist())


# ---- noise rows ---------------------------------------------------------------------------------------------------------------------
NOISE_ROWS = [("short-rooms-i16", (0.02, 0.05), [2500, TILE + 9, 40], "i16"), ("short-rooms-f32", (0.01, 0.03), [TILE - 5, 700], "f32")]
NOISE_ROWS_GPU = NOISE_ROWS + [("second-in-a-room", 0.3, [16000, 16000], "i16")]


def check_noise_row(lib, name, rt60, lengths, fmt):
    """Responses off the grid: every output within (terms + 1) 2^-24 sum |h x| of the float64 dot product."""
    Rv = reverberation()
    irs = Rv.ImpulseResponses.synthetic(len(lengths), rt60, 16000, seed=3, device=Cm.device_of(lib), lib=lib)
    hs = irs.numpy()
    rng = np.random.RandomState(9)
    xs = [rng.randint(-32768, 32768, n).astype(np.int16) for n in lengths]
    ms = [len(x) + len(h) - 1 for x, h in zip(xs, hs)]
    f, _ = raw_reverb(lib, xs, hs, np.arange(len(xs)), ms, fmt, "f")
    worst, a = 0.0, 0
    for x, h, m in zip(xs, hs, ms):
        y, bound = Rr.dot64(x, h, m)
        err = np.abs(f[a:a + m].astype(np.float64) - y)
        assert bound.min() > 0
        worst = max(worst, float((err / bound).max()))
        a += m
    print("REVERB_CONFIGS_ERR " + json.dumps({"row": name, "lib": lib.kind, "taps": [len(h) for h in hs], "lengths": list(lengths),
                                               "worst_err_over_bound": worst}))
    assert worst <= 1.0, (name, worst)


# ---- invariance ---------------------------------------------------------------------------------------------------------------------
def check_invariance(lib):
    """A clip alone, in the middle of a table, at another pool offset and with its response elsewhere in the bank: the same bits.  On
    the emulator the workgroups of the table also run last to first."""
    rng = np.random.RandomState(31)
    x, h = rng.randint(-32768, 32768, TILE + 40).astype(np.int16), Rr.grid_response(rng, 77)
    m = len(x) + len(h) - 1
    alone = raw_reverb(lib, [x], [h], [0], [m])
    want = Rr.chain(x, h, np.arange(m))
    assert np.array_equal(alone[0].view(np.int32), want.view(np.int32)) and np.array_equal(alone[1], Rr.np_pcm(want))
    others = [rng.randint(-32768, 32768, k).astype(np.int16) for k in (14, TILE - 1, 0, 3)]
    h2 = Rr.grid_response(rng, 300)
    xs = others[:2] + [x] + others[2:]
    ir = [1, 1, 0, 1, 1]
    ms = [len(c) + len((h, h2)[r]) - 1 if len(c) else 0 for c, r in zip(xs, ir)]
    a = int(np.sum(ms[:2]))
    assert a % 2 == 1 and ms[1] > TILE                     # an odd output offset, behind a clip of two tiles
    table = raw_reverb(lib, xs, [h, h2], ir, ms)
    moved = raw_reverb(lib, xs, [h2, h], [1 - r for r in ir], ms, in_off=[7, 40, 2 * TILE + 1, 4 * TILE, 4 * TILE + 9], ir_off=[3, 310])
    runs = [table, moved]
    if lib.kind == "emu":
        was = lib._dll.tcr_emu_block_order(1)
        try:
            runs.append(raw_reverb(lib, xs, [h, h2], ir, ms))
        finally:
            lib._dll.tcr_emu_block_order(was)
    for run in runs:
        assert np.array_equal(run[0][a:a + m].view(np.int32), alone[0].view(np.int32)) and np.array_equal(run[1][a:a + m], alone[1])
        assert np.array_equal(run[0].view(np.int32), table[0].view(np.int32)) and np.array_equal(run[1], table[1])
    at = 0
    for c, r, k in zip(xs, ir, ms):                         # and the neighbours are what the rule says
        w = Rr.chain(c, (h, h2)[r], np.arange(k))
        assert np.array_equal(table[0][at:at + k].view(np.int32), w.view(np.int32))
        at += k


# ---- identity and the layers --------------------------------------------------------------------------------------------------------
def wet_reference(clips, hs, idx, tail):
    """Per clip the reference's wet int16 clip: np_pcm(chain) over n + min(L - 1, tail) outputs (idx -1: the clip itself)."""
    out = []
    for c, r in zip(clips, idx):
        if r < 0 or len(c) == 0:
            out.append(c.copy())
            continue
        h = hs[r]
        m = len(c) + (len(h) - 1 if tail is None else min(len(h) - 1, tail))
        out.append(Rr.np_pcm(Rr.chain(c, h, np.arange(m))))
    return out


def check_identity_and_layers(lib):
    from oracle import augment_ref as A
    from tcresnet_amd import composing as Cp
    from tcresnet_amd.datasets import augmentation_factory as F
    from tests.test_compose import np_compose
    Rv = reverberation()
    dev = Cm.device_of(lib)
    rng = np.random.RandomState(41)
    clips = [rng.randint(-32768, 32768, n).astype(np.int16) for n in (900, 1, 0, TILE + 3, 317, 640)]
    pool = make_pool(lib, clips)
    # the response [1.0] reproduces the pool byte for byte
    for irs, idx in ((Rv.ImpulseResponses.dry(dev, lib), np.zeros(len(clips), np.int64)),
                     (Rv.ImpulseResponses.from_arrays([np.ones(5)], device=dev, lib=lib), np.full(len(clips), -1))):
        same = Rv.reverberate(pool, irs, idx)
        assert np.array_equal(same.lengths, pool.lengths) and np.array_equal(same.offsets, pool.offsets)
        assert same.data.cpu().numpy()[:int(pool.lengths.sum())].tobytes() == np.concatenate(clips).tobytes()
    # a wet pool: the reference's wet clips, read by the composer and by the input stage
    hs = [Rr.grid_response(rng, L, 0.25) for L in (120, 33)]
    irs = Rv.ImpulseResponses.from_arrays(hs, normalize=None, device=dev, lib=lib)
    assert all(np.array_equal(a, b) for a, b in zip(irs.numpy(), hs))
    idx = np.array([0, 1, 0, 1, -1, 0])
    for tail_ms, tail in ((None, None), (2.0, 32)):
        wet = Rv.reverberate(pool, irs, idx, tail_ms)
        ref = wet_reference(clips, hs, idx, tail)
        assert wet.lengths.tolist() == [len(c) for c in ref] and wet.data.dtype == torch.int16
        assert np.array_equal(wet.offsets, np.concatenate([[0], np.cumsum(wet.lengths)[:-1]]))
        assert wet.data.cpu().numpy()[:int(wet.lengths.sum())].tobytes() == np.concatenate(ref).tobytes()
    assert wet.lengths.tolist() == [900 + 32, 1 + 32, 0, TILE + 3 + 32, 317, 640 + 32]
    bgs = [rng.randint(-3000, 3000, 5000).astype(np.int16)]
    bgpool = make_pool(lib, bgs)
    cmp_ = Cp.Composer(wet, np.arange(len(clips)) % 3, ["a", "b", "c"], bgpool)
    sq = cmp_.energies()[0]
    assert np.array_equal(sq, np.array([np.sum(c.astype(np.int64) ** 2) for c in ref]))
    t = dict(lengths=np.array([3000, 2 * TILE]), po=np.array([0, 2, 4], np.int32), clip_off=wet.offsets[[0, 4, 3, 1]],
             len=wet.lengths[[0, 4, 3, 1]].astype(np.int32), first=np.array([10, 1500, -5, TILE + 100], np.int64),
             gain=np.array([1.0, 0.37, 0.5, 1.0], np.float32), bg_off=np.zeros(2, np.int64), bg_len=np.full(2, 5000, np.int64),
             bg_phase=np.array([0, 4999], np.int64), bg_vol=np.array([0.1, 1.0], np.float32))
    plan = Cp.CompositionPlan(16000, t["lengths"], t["po"], t["clip_off"], t["len"], t["first"], t["gain"], [0, 1, 0, 1], t["bg_off"], t["bg_len"],
                              t["bg_phase"], t["bg_vol"])
    got = cmp_.compose(plan).signals[0].cpu().numpy()
    assert np.array_equal(got.view(np.int32), np_compose(np.concatenate(ref), np.concatenate(bgs), t).view(np.int32))
    # the training input stage on the wet pool
    desired, pick = 1000, np.array([0, 1, 2, 3, 4, 5, 0])
    shift = np.array([0, -100, 99, 7, 0, -3, 50], np.int32)
    crop, vol = np.array([0, 5, 100, 4000, 17, 1, 2], np.int64), np.array([0.0, 0.1, 0.05, 1.0, 0.0, 0.02, 0.1], np.float32)
    out = F.anchored_slice_or_pad_with_shift(wet, pick, desired, "wav", 16000, background_data=bgpool, is_training=True,
                                             draws=(shift, np.zeros(7, np.int64), crop, vol))[..., 0].cpu().numpy()
    want = A.augment_batch(np.concatenate(ref), wet.offsets[pick], wet.lengths[pick], shift, np.concatenate(bgs), crop, vol, desired)
    assert np.array_equal(out.view(np.int32), want.view(np.int32))
    # whole float32 recordings: lengths kept, or the tail appended
    sig = Rr.decode(np.concatenate([clips[0], clips[4]]))
    for tail in (False, True):
        y, lens = Rv.reverberate_signals(dev_t(lib, sig), [900, 317], irs, [1, -1], tail=tail)
        assert lens.tolist() == ([900 + 32, 317] if tail else [900, 317])
        w0 = Rr.chain(clips[0], hs[1], np.arange(int(lens[0])))
        assert np.array_equal(y.cpu().numpy().view(np.int32), np.concatenate([w0, Rr.decode(clips[4])]).view(np.int32))


def check_reverberated_composer(lib):
    from tcresnet_amd import composing as Cp
    from tests.test_compose import small_pool
    Rv = reverberation()
    dev = Cm.device_of(lib)
    clips, labels, pool = small_pool(lib, 5, n=10, lo=400, hi=1500)
    names = [f"c{i}" for i in range(12)]
    dry = Cp.Composer(pool, labels, names)
    irs = Rv.ImpulseResponses.synthetic(4, (0.005, 0.02), 16000, seed=2, device=dev, lib=lib)
    a, b, c = (dry.reverberated(irs, 0.6, None, seed=s) for s in (3, 3, 4))
    assert np.array_equal(a.ir_index, b.ir_index) and not np.array_equal(a.ir_index, c.ir_index)
    assert (a.ir_index == -1).any() and (a.ir_index >= 0).any() and a.ir_index.max() < 4
    assert np.array_equal(a.ir_index, Rv.draw_responses(len(clips), 4, 0.6, 3))
    assert torch.equal(a.pool.data, b.pool.data) and np.array_equal(a.labels, dry.labels) and a.label_names == dry.label_names
    grow = np.where((a.ir_index >= 0) & (pool.lengths > 0), irs.lengths[np.maximum(a.ir_index, 0)] - 1, 0)
    assert np.array_equal(a.pool.lengths, pool.lengths + grow) and grow.max() > 50
    pa, pb = (x.plan(2, 3.0, 320, min_gap_ms=100, max_gap_ms=300, seed=1) for x in (a, b))
    assert pa.events == pb.events and len(pa.place_len) >= 4
    ra, rb = a.compose(pa, pcm=True), b.compose(pb, pcm=True)
    assert torch.equal(ra.pcm, rb.pcm) and torch.equal(ra.signals[0], rb.signals[0])
    ends = [e - s for evs in pa.events for s, e, _ in evs]
    assert np.allclose(sorted(ends), sorted(1000.0 * pa.place_len / 16000))      # an event covers the wet clip, tail included
    tight = dry.reverberated(irs, 0.6, 1.0, seed=3)                               # tail_ms tightens them
    assert np.array_equal(tight.pool.lengths, pool.lengths + np.minimum(grow, 16))
    # probability 0: the dry composer's output
    none = dry.reverberated(irs, 0.0, None, seed=3)
    assert (none.ir_index == -1).all() and np.array_equal(none.pool.lengths, pool.lengths)
    pd, pn = (x.plan(2, 3.0, 320, min_gap_ms=100, max_gap_ms=300, seed=1) for x in (dry, none))
    assert pd.events == pn.events and torch.equal(dry.compose(pd, pcm=True).pcm, none.compose(pn, pcm=True).pcm)


def check_pipeline(lib):
    """A composed wet corpus goes through scan_ragged and sweep."""
    from tcresnet_amd import composing as Cp
    from tests.test_compose import small_pool
    from tests.test_scan_ragged import scanning
    from tests.test_streaming import setup
    Rv, Sc = reverberation(), scanning()
    fe, net, _, _, _ = setup(lib)
    sc = Sc.KeywordScanner(net, fe, average_window_ms=100, min_count=2, detection_threshold=0.0, suppression_ms=40)
    clips, labels, pool = small_pool(lib, 7, n=6)
    irs = Rv.ImpulseResponses.synthetic(3, 0.05, 16000, seed=1, device=Cm.device_of(lib), lib=lib)
    wet = Cp.Composer(pool, labels, [f"c{i}" for i in range(12)]).reverberated(irs, 0.8, tail_ms=30, seed=5)
    plan = wet.plan(2, [3.0, 2.0], sc.step_samples, min_gap_ms=1100, max_gap_ms=1300, seed=11)
    rec = wet.compose(plan)
    out = sc.scan_ragged(rec.signals)
    res = sc.sweep(out, [0.0, 0.5], events=rec.events)
    assert int(np.asarray(res.events).sum()) == len(plan.place_len) >= 1
    room, lens = Rv.reverberate_signals(*rec.signals, irs, [0, -1])               # the room over clips and background together
    assert lens.tolist() == plan.lengths.tolist()
    again = sc.scan_ragged((room, lens))
    assert len(again.signal(0)) == len(out.signal(0))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    Rv = reverberation()
    dev = Cm.device_of(lib)
    err = lambda: lib.tcr_last_error().decode()
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    pcm = torch.ones(64, dtype=torch.int16, device=dev)
    ir = torch.ones(8, dtype=torch.float32, device=dev)
    out, out_pcm = torch.full((24,), 7.0, device=dev), torch.full((24,), 77, dtype=torch.int16, device=dev)
    base = dict(n=1, data=pcm, fmt=1, size=64, in_off=i64(2), in_len=i64(8), ir=ir, floats=8, ir_off=i64(1), ir_len=i32(3), clip_ir=i32(0),
                out_off=i64(0, 10), tile_off=i64(0, 1), tiles=1, out=out.data_ptr(), out_pcm=out_pcm.data_ptr())
    order = ("n", "data", "fmt", "size", "in_off", "in_len", "ir", "floats", "ir_off", "ir_len", "clip_ir", "out_off", "tile_off", "tiles", "out", "out_pcm")

    def call(**kw):
        a = dict(base, **kw)
        return lib.tcr_reverb(*(a[k] if isinstance(a[k], int) or a[k] is None else a[k].data_ptr() for k in order), None)

    assert call(out=None, out_pcm=None) == -1 and "tcr_reverb: out and out_pcm are both null" in err()
    assert call(n=-1) == -1 and "n_clips must be >= 0 (got -1)" in err()
    for k in ("data", "in_off", "in_len", "ir", "ir_off", "ir_len", "clip_ir", "out_off", "tile_off"):
        assert call(**{k: None}) == -1 and "tcr_reverb: null argument" in err(), k
    for fmt in (2, -1):
        assert call(fmt=fmt) == -1 and f"unknown in_format {fmt}" in err()
    assert call(out=out.data_ptr() + 2) == -1 and "out must be 4-byte aligned" in err()
    assert call(out_pcm=out_pcm.data_ptr() + 1) == -1 and "out_pcm must be 2-byte aligned" in err()
    assert call(ir=ir.data_ptr() + 2) == -1 and "ir must be 4-byte aligned" in err()
    assert call(tiles=2 ** 31) == -1 and "tiles are too many for one launch" in err()
    assert call(tiles=-1) == -1 and "negative count" in err()
    assert call(n=0) == 0 and call(tiles=0) == 0
    assert bool((out == 7.0).all()) and bool((out_pcm == 77).all())                # nothing was launched, nothing written
    assert call() == 0 and call(out=None) == 0 and call(out_pcm=None) == 0
    assert out[:10].tolist() == [1 / 32768, 2 / 32768] + [3 / 32768] * 6 + [2 / 32768, 1 / 32768] and bool((out[10:] == 7.0).all())
    assert out_pcm[:10].tolist() == [1, 2, 3, 3, 3, 3, 3, 3, 2, 1] and bool((out_pcm[10:] == 77).all())
    # the Python layer
    R = Rv.ImpulseResponses
    with pytest.raises(T.TcrError, match=f"response 1 has 0 taps; 1 .. {MAX} are taken"):
        R.from_arrays([np.ones(3), np.zeros(0)], device=dev, lib=lib)
    with pytest.raises(T.TcrError, match=f"response 0 has {MAX + 1} taps"):
        R.from_arrays([np.ones(MAX + 1)], device=dev, lib=lib)
    with pytest.raises(T.TcrError, match="response 0 has taps that are not finite"):
        R.from_arrays([np.array([1.0, np.nan])], device=dev, lib=lib)
    with pytest.raises(T.TcrError, match="normalize must be 'energy', 'peak' or None"):
        R.from_arrays([np.ones(3)], normalize="loud", device=dev, lib=lib)
    with pytest.raises(T.TcrError, match="at least one response"):
        R.from_arrays([], device=dev, lib=lib)
    with pytest.raises(T.TcrError, match="a response lies outside the bank's 8 floats"):
        R(ir, [6], [3], lib)
    with pytest.raises(T.TcrError, match="ImpulseResponses.synthetic: count 0"):
        R.synthetic(0, 0.3, 16000, device=dev, lib=lib)
    with pytest.raises(T.TcrError, match="ImpulseResponses.synthetic"):
        R.synthetic(2, (0.3, 0.1), 16000, device=dev, lib=lib)
    bank = R.from_arrays([np.ones(3), np.ones(2)], device=dev, lib=lib)
    pool = make_pool(lib, [np.ones(10, np.int16), np.ones(4, np.int16)])
    with pytest.raises(T.TcrError, match=r"clip 1 asks for response 2 of a bank of 2 \(-1: dry\)"):
        Rv.reverberate(pool, bank, [0, 2])
    with pytest.raises(T.TcrError, match="clip 0 asks for response -2"):
        Rv.reverberate(pool, bank, [-2, 0])
    with pytest.raises(T.TcrError, match="1 responses for 2 clips"):
        Rv.reverberate(pool, bank, [0])
    with pytest.raises(T.TcrError, match="tail_ms must be >= 0"):
        Rv.reverberate(pool, bank, [0, 1], tail_ms=-1)
    with pytest.raises(T.TcrError, match="clips outside the audio's"):
        Rv.reverb(lib, pool.data, [0, 12], [10, 4], bank, [0, 1], [10, 4])
    with pytest.raises(T.TcrError, match="clip 1 asks for response 5 of a bank of 2"):
        Rv.reverb(lib, pool.data, [0, 10], [10, 4], bank, [0, 5], [10, 4])
    with pytest.raises(T.TcrError, match="neither floats nor pcm"):
        Rv.reverb(lib, pool.data, [0], [10], bank, [0], [10], floats=False, pcm=False)
    with pytest.raises(T.TcrError, match="a negative output length"):
        Rv.reverb(lib, pool.data, [0], [10], bank, [0], [-1])
    with pytest.raises(T.TcrError, match="expected packed float32"):
        Rv.reverberate_signals(pool.data, [14], bank, [0])
    with pytest.raises(T.TcrError, match=r"probability must be in \[0, 1\]"):
        Rv.draw_responses(3, 2, 1.5)


# ---- host only ----------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_class():
    seen = set().union(*(r.cls for r in Rc.ROWS))
    assert seen == Rc.ALL_CLASSES, Rc.ALL_CLASSES ^ seen
    assert len({r.name for r in Rc.ROWS}) == len(Rc.ROWS)
    assert (TILE, STAGE, MAX) == (T._lib.REVERB_TILE, T._lib.REVERB_STAGE, T._lib.REVERB_TAPS_MAX)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcresnet_hip.h")).read()
    for name, v in (("TILE", TILE), ("STAGE", STAGE), ("TAPS_MAX", MAX)):
        assert f"#define TCR_REVERB_{name} {v}\n" in hdr
    assert "tile-edges" == Rc.EDGE_ROW.name and len(Rc.EDGE_ROW.clips) == 300 and {int(m) % TILE for m in Rc.EDGE_ROW.m} >= {TILE - 2, TILE - 1, 0, 1, 2}


def test_reference_step_is_the_fmaf_step():
    assert Rr.check_grid_argument() >= 300
    # and the reference is the plain chain on a case small enough to write out
    x, h = np.array([32767, -32768, 3], np.int16), np.array([0.5, -0.25], np.float32)
    xs = Rr.decode(x).astype(np.float64)
    want = [0.5 * xs[0], -0.25 * xs[0] + 0.5 * xs[1], -0.25 * xs[1] + 0.5 * xs[2], -0.25 * xs[2], 0.0]
    assert Rr.chain(x, h, np.arange(5)).tolist() == [float(np.float32(v)) for v in want]
    y, bound = Rr.dot64(x, h, 5)
    assert np.allclose(y, want) and bound[4] == 0 and bound[1] == 3 * 2.0 ** -24 * (0.25 * xs[0] + 0.5 * -xs[1])


def test_synthetic_responses_hit_drr_and_rt60():
    Rv = reverberation()

    class Host:                                         # (host arithmetic only: no library call is made)
        kind = "emu"
    for rt60, drr in ((0.3, 6.0), (0.6, 0.0)):
        irs = Rv.ImpulseResponses.synthetic(3, rt60, 16000, seed=4, drr_db=drr, lib=Host())
        for h in irs.numpy():
            h = h.astype(np.float64)
            assert h.size == int(np.ceil(rt60 * 16000)) and h[0] == np.abs(h).max() and abs(np.sum(h * h) - 1.0) < 1e-5
            assert abs(10 * np.log10(h[0] ** 2 / np.sum(h[1:] ** 2)) - drr) < 1e-4
            edc = 10 * np.log10(np.cumsum((h[1:] ** 2)[::-1])[::-1] / np.sum(h[1:] ** 2))      # Schroeder's backward integral
            fit = np.flatnonzero((edc < -5) & (edc > -25))
            slope = np.polyfit(fit / 16000.0, edc[fit], 1)[0]
            assert abs(-60.0 / slope - rt60) < 0.1 * rt60, (rt60, -60.0 / slope)
    ranged = Rv.ImpulseResponses.synthetic(8, (0.1, 0.4), 16000, seed=1, lib=Host())
    assert len(set(ranged.lengths.tolist())) == 8 and ranged.lengths.min() >= 1600 and ranged.lengths.max() <= 6400
    again = Rv.ImpulseResponses.synthetic(8, (0.1, 0.4), 16000, seed=1, lib=Host())
    assert torch.equal(ranged.data, again.data)
    assert Rv.ImpulseResponses.synthetic(1, 2.0, 16000, lib=Host()).lengths.tolist() == [MAX]
    peak = Rv.ImpulseResponses.from_arrays([[0.5, -2.0, 1.0]], normalize="peak", lib=Host()).numpy()[0]
    assert peak.tolist() == [0.25, -1.0, 0.5]


def test_compose_audio_rir_flags_are_refused():
    from tcresnet_amd import compose_audio
    base = ["--dataset_path", "d", "--output_dir", "o", "--num_recordings", "2", "--seconds", "3"]
    for extra, msg in [(["--rir_dir", "x", "--rir_rt60", "0.3"], "exclude each other"), (["--rir_count", "4"], "--rir_count needs --rir_dir or --rir_rt60"),
                       (["--rir_probability", "0.5"], "--rir_probability needs"), (["--rir_tail_ms", "5"], "--rir_tail_ms needs"),
                       (["--rir_seed", "1"], "--rir_seed needs"), (["--rir_dir", "x", "--rir_count", "4"], "it needs --rir_rt60"),
                       (["--rir_rt60", "0.3", "--rir_count", "0"], "--rir_count must be >= 1"),
                       (["--rir_rt60", "0.3", "--rir_probability", "1.5"], r"--rir_probability must be in \[0, 1\]"),
                       (["--rir_rt60", "0.3", "--rir_tail_ms", "-1"], "--rir_tail_ms must be >= 0"), (["--rir_rt60", "0.5:0.2"], "--rir_rt60 0.5:0.2"),
                       (["--rir_rt60", "0"], "--rir_rt60 0"), (["--rir_rt60", "long"], "--rir_rt60 long")]:
        with pytest.raises(SystemExit, match=msg):
            compose_audio.check_arguments(compose_audio.parse_arguments(base + extra))
    args = compose_audio.check_arguments(compose_audio.parse_arguments(base + ["--rir_rt60", "0.2:0.4", "--rir_count", "3"]))
    assert args.rir_rt60 == (0.2, 0.4) and args.rir_count == 3 and args.rir_probability is None
    args.rir_dir, args.rir_rt60 = "/no/such/dir", None
    with pytest.raises(SystemExit, match="no such directory"):
        compose_audio.open_responses(args, "cpu")


# ---- files and the command line -----------------------------------------------------------------------------------------------------
def check_from_files(lib, tmp):
    from tcresnet_amd.audio_input import write_wav
    from tcresnet_amd.resampling import Resampler
    Rv = reverberation()
    dev = Cm.device_of(lib)
    rng = np.random.RandomState(51)
    h = np.zeros(400)
    h[37] = 0.9                                         # the direct path behind a pre-delay, an early reflection, a decaying tail
    h[60] = -0.5
    h[38:] += 0.2 * rng.standard_normal(400 - 38) * np.exp(-np.arange(400 - 38) / 60.0) * (np.arange(400 - 38) > 30)
    pcm16 = np.clip(np.rint(h * 32768), -32768, 32767).astype(np.int16)
    assert int(np.argmax(np.abs(pcm16))) == 37
    p16 = os.path.join(tmp, "room16.wav")
    write_wav(p16, pcm16, 16000)
    t = np.arange(1500)                                 # at 48 kHz: a band-limited pulse at sample 300 (100 at 16 kHz) and a slow tail
    h48 = 0.8 * np.exp(-0.5 * ((t - 300) / 6.0) ** 2) - 0.3 * np.exp(-0.5 * ((t - 700) / 9.0) ** 2) + 0.05 * np.sin(t / 40.0) * np.exp(-t / 400.0) * (t > 330)
    p48 = os.path.join(tmp, "room48.wav")
    pcm48 = np.rint(h48 * 32768).astype(np.int16)
    write_wav(p48, pcm48, 48000)
    irs = Rv.ImpulseResponses.from_files([p16, p48], 16000, device=dev, lib=lib)
    got = irs.numpy()
    want = pcm16[37:].astype(np.float64) / 32768.0
    assert np.array_equal(got[0], (want / np.sqrt(np.sum(want * want))).astype(np.float32))
    rs = Resampler(48000, 16000, 1, device=dev, lib=lib).resample(dev_t(lib, pcm48).reshape(1, -1)).reshape(-1).cpu().numpy().astype(np.float64)
    at = int(np.argmax(np.abs(rs)))
    assert abs(at - 100) <= 1 and rs.size == 500
    assert np.array_equal(got[1], (rs[at:] / np.sqrt(np.sum(rs[at:] ** 2))).astype(np.float32))
    for g in got:                                       # the direct path sits at tap 0
        assert int(np.argmax(np.abs(g))) == 0 and abs(float(np.sum(g.astype(np.float64) ** 2)) - 1.0) < 1e-5
    cut = Rv.ImpulseResponses.from_files([p16, p48], 16000, max_ms=5.0, device=dev, lib=lib)
    assert cut.lengths.tolist() == [80, 80]
    with pytest.raises(T.TcrError, match="is silent"):
        write_wav(os.path.join(tmp, "silent.wav"), np.zeros(10, np.int16), 16000)
        Rv.ImpulseResponses.from_files([os.path.join(tmp, "silent.wav")], 16000, device=dev, lib=lib)


RIR_CLI = ["--rir_rt60", "0.01:0.03", "--rir_count", "3", "--rir_probability", "0.7", "--rir_tail_ms", "10", "--rir_seed", "6"]


def check_cli_output(lib, out_dir, stdout, stderr, data_dir, extra, make_irs):
    """compose_audio.py's files against the API's run of the same plan on the same wet pool."""
    from tcresnet_amd import compose_audio, composing as Cp, runtime
    from tcresnet_amd.audio_input import WavFile
    from tests.test_compose import CLI
    runtime.set_default(lib, Cm.device_of(lib))
    try:
        args = compose_audio.check_arguments(compose_audio.parse_arguments(["--dataset_path", data_dir, "--output_dir", out_dir, *CLI, *extra]))
        cmp_ = Cp.Composer.from_dataset(compose_audio.open_dataset(args))
        wet = cmp_.reverberated(make_irs(), 0.7, 10.0, seed=6)
    finally:
        runtime.set_default(None, None)
    assert (wet.ir_index >= 0).any() and (wet.pool.lengths > cmp_.pool.lengths).any()
    plan = wet.plan(3, 6.0, 320, min_gap_ms=1200, max_gap_ms=2000, snr_db=(3.0, 9.0), seed=4)
    pcm = wet.compose(plan, floats=False, pcm=True).pcm.cpu().numpy()
    wavs = [os.path.join(out_dir, f"rec_{n:04d}.wav") for n in range(3)]
    assert stdout.split() == wavs + [os.path.join(out_dir, "events.csv")]
    for n, path in enumerate(wavs):
        wav = WavFile(path)
        assert wav.length == 96000 and wav.read_pcm(0, wav.length).tobytes() == pcm[n * 96000:(n + 1) * 96000].tobytes()
    with open(os.path.join(out_dir, "events.csv"), newline="") as fh:
        rows = list(csv.DictReader(fh))
    got = [[] for _ in wavs]
    for r in rows:
        got[wavs.index(r["file"])].append((float(r["start_ms"]), float(r["end_ms"]), wet.label_names.index(r["label"])))
    assert got == plan.events and len(plan.place_len) >= 4
    info = json.loads(stderr.strip().splitlines()[-1])
    assert info["recordings"] == 3 and info["wet_clips"] == int((wet.ir_index >= 0).sum()) and info["responses"] == len(make_irs())


def check_cli(lib, tmp_path, capsys):
    from tcresnet_amd import compose_audio, runtime
    from tests.test_compose import CLI, wav_tree
    Rv = reverberation()
    dev = Cm.device_of(lib)
    data = str(tmp_path / "data")
    wav_tree(data)

    def run(out_dir, extra):
        runtime.set_default(lib, dev)
        try:
            assert compose_audio.main(compose_audio.parse_arguments(["--dataset_path", data, "--output_dir", out_dir, *CLI, *extra])) == 0
        finally:
            runtime.set_default(None, None)
        return capsys.readouterr()

    cap = run(str(tmp_path / "syn"), RIR_CLI)
    check_cli_output(lib, str(tmp_path / "syn"), cap.out, cap.err, data, RIR_CLI,
                     lambda: Rv.ImpulseResponses.synthetic(3, (0.01, 0.03), 16000, seed=6, device=dev, lib=lib))
    rirs = str(tmp_path / "rirs")
    os.makedirs(rirs)
    check_from_files(lib, rirs)
    os.remove(os.path.join(rirs, "silent.wav"))
    flags = ["--rir_dir", rirs] + RIR_CLI[4:]
    cap = run(str(tmp_path / "dir"), flags)
    check_cli_output(lib, str(tmp_path / "dir"), cap.out, cap.err, data, flags,
                     lambda: Rv.ImpulseResponses.from_files([os.path.join(rirs, "room16.wav"), os.path.join(rirs, "room48.wav")], 16000, device=dev, lib=lib))


# ---- emulator -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", Rc.ROWS, ids=lambda r: r.name)
def test_reverb_row_equals_rule(emu_lib, row):
    check_row(emu_lib, row)


def test_reverb_integer_rows_are_exact(emu_lib):
    check_integer_rows(emu_lib)


@pytest.mark.parametrize("name,rt60,lengths,fmt", NOISE_ROWS, ids=[r[0] for r in NOISE_ROWS])
def test_reverb_noise_rows_within_chain_bound(emu_lib, name, rt60, lengths, fmt):
    check_noise_row(emu_lib, name, rt60, lengths, fmt)


def test_reverb_is_invariant_to_neighbours_offsets_and_block_order(emu_lib):
    check_invariance(emu_lib)


def test_reverberate_identity_pool_composer_and_input_stage(emu_lib):
    check_identity_and_layers(emu_lib)


def test_reverberated_composer_is_seeded(emu_lib):
    check_reverberated_composer(emu_lib)


def test_wet_corpus_through_scan_and_sweep(emu_lib):
    check_pipeline(emu_lib)


def test_reverb_refusals(emu_lib):
    check_refusals(emu_lib)


def test_compose_audio_rir_writes_what_the_api_composes(emu_lib, tmp_path, capsys):
    check_cli(emu_lib, tmp_path, capsys)


# ---- MI355X -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row", Rc.ROWS + [Rc.EDGE_ROW, Rc.LONG_ROW], ids=lambda r: r.name)
def test_gpu_reverb_row_equals_rule(hip_lib, row):
    check_row(hip_lib, row)


@pytest.mark.gpu
def test_gpu_reverb_integer_rows_are_exact(hip_lib):
    check_integer_rows(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name,rt60,lengths,fmt", NOISE_ROWS_GPU, ids=[r[0] for r in NOISE_ROWS_GPU])
def test_gpu_reverb_noise_rows_within_chain_bound(hip_lib, name, rt60, lengths, fmt):
    check_noise_row(hip_lib, name, rt60, lengths, fmt)


@pytest.mark.gpu
def test_gpu_reverb_is_invariant_to_neighbours_and_offsets(hip_lib):
    check_invariance(hip_lib)


@pytest.mark.gpu
def test_gpu_reverberate_identity_pool_composer_and_input_stage(hip_lib):
    check_identity_and_layers(hip_lib)


@pytest.mark.gpu
def test_gpu_reverberated_composer_is_seeded(hip_lib):
    check_reverberated_composer(hip_lib)


@pytest.mark.gpu
def test_gpu_wet_corpus_through_scan_and_sweep(hip_lib):
    check_pipeline(hip_lib)


@pytest.mark.gpu
def test_gpu_reverb_refusals(hip_lib):
    check_refusals(hip_lib)


@pytest.mark.gpu
def test_gpu_compose_audio_rir_writes_what_the_api_composes(hip_lib, tmp_path, capsys):
    check_cli(hip_lib, tmp_path, capsys)
