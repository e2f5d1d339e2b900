"""Time of composing labelled test recordings on the device (composing.Composer.compose: tcr_compose; tcr_pcm_energy) next to what a
user has without it, on the corpus shapes of the other detection benches: 64 x 1 hour, and 255 signals of 1 - 10 s plus one of
10 minutes (scan_bench.py's --ragged corpus), one word per ~3 s (1 s clips, gaps of 1.5 - 2.5 s) over looping minute-long noise.

    python scripts/compose_bench.py [--reps 5] [--out profiles/compose_bench.json] [--shapes hours,ragged] [--pool 100000]

The pool is `--pool` one-second clips and six one-minute background recordings of random int16 in ONE device tensor.  Legs per shape
(medians over --reps timed calls after a warm-up call, device events around the Python call, so compose's table uploads are inside;
the legs alternate within a rep; the two slow baselines run --slow_reps times):
  compose_f32      Composer.compose(plan) -> packed float32
  compose_i16      Composer.compose(plan, floats=False, pcm=True) -> packed int16
  compose_f32_runK compose_f32 with K tiles per workgroup instead of 4 (TCR_TUNE_COMPOSE_RUN; 1: every tile searches its tables)
  host             (a) the same composition in NumPy on 16 host threads (one recording per task: the tiled background, one
                   slice-multiply-add per placement, the clip) and the upload of the packed float32: what a user does today
  torch            (b) plain torch on the device: zeros, per recording the tiled background scaled, one slice-multiply-add per
                   placement, clamp
  copy_f32 / _i16  (c) a device-to-device copy of the output's bytes: the bandwidth ceiling
(a) and (b) are asserted bitwise equal to compose's output before anything is timed.  GB/s: the bytes a leg has to move -- compose:
the output written, 2 bytes of background per sample and 2 per placed sample read; copy: the output read and written.
And once: tcr_pcm_energy over the whole pool and the backgrounds in one call (`energy`), next to torch's (v.long() ** 2).sum over the
same clips (`energy_torch`) and a copy of the pool's bytes (`energy_copy`)."""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd import _lib                                         # noqa: E402
from tcresnet_amd.composing import Composer, pcm_energy               # noqa: E402
from tcresnet_amd.datasets.augmentation_factory import PcmPool        # noqa: E402
from scripts.scan_bench import corpus_steps, time_ms                  # noqa: E402

SR, HOP, CLIP, MINUTE = 16000, 320, 16000, 60 * 16000
SCALE = np.float32(1.0 / 32768.0)


def view_pool(data, lengths, lib):
    """A PcmPool over `data` (a device tensor that already holds the clips one after the other)."""
    pool = PcmPool.__new__(PcmPool)
    pool.lib, pool.device, pool.data = lib, data.device, data
    pool.lengths = np.asarray(lengths, np.int64)
    pool.offsets = np.concatenate([[0], np.cumsum(pool.lengths)[:-1]]).astype(np.int64)
    return pool


def host_compose(pcm, bg, plan, dev, threads=16):
    out = np.empty(plan.total_samples, np.float32)

    def one(n):
        a, L = int(plan.sample_offsets[n]), int(plan.lengths[n])
        bo, bl, ph = int(plan.bg_off[n]), int(plan.bg_len[n]), int(plan.bg_phase[n])
        o = np.tile(bg[bo:bo + bl], -(-(ph + L) // bl))[ph:ph + L].astype(np.float32)
        o *= SCALE
        o *= plan.bg_vol[n]
        for j in range(int(plan.place_offsets[n]), int(plan.place_offsets[n + 1])):
            f, m, c = int(plan.place_first[j]), int(plan.place_len[j]), int(plan.place_clip_off[j])
            o[f:f + m] += pcm[c:c + m].astype(np.float32) * SCALE * plan.place_gain[j]
        np.clip(o, -1.0, 1.0, out=out[a:a + L])

    with cf.ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(plan.n_recordings)))
    return torch.from_numpy(out).to(dev)


def torch_compose(pcm, bg, plan):
    out = torch.zeros(plan.total_samples, dtype=torch.float32, device=pcm.device)
    for n in range(plan.n_recordings):
        a, L = int(plan.sample_offsets[n]), int(plan.lengths[n])
        bo, bl, ph = int(plan.bg_off[n]), int(plan.bg_len[n]), int(plan.bg_phase[n])
        out[a:a + L] = bg[bo:bo + bl].repeat(-(-(ph + L) // bl))[ph:ph + L].to(torch.float32).mul_(float(SCALE)).mul_(float(plan.bg_vol[n]))
    first = (plan.sample_offsets[plan.place_recording] + plan.place_first).tolist()
    for f, m, c, g in zip(first, plan.place_len.tolist(), plan.place_clip_off.tolist(), plan.place_gain.tolist()):
        out[f:f + m] += pcm[c:c + m].to(torch.float32).mul_(float(SCALE)).mul_(g)
    return out.clamp_(-1.0, 1.0)


def shape_row(args, composer, name, seconds):
    dev = composer.device
    plan = composer.plan(len(seconds), seconds, HOP, min_gap_ms=1500, max_gap_ms=2500, snr_db=(0, 20), seed=0)
    total, placed = plan.total_samples, int(plan.place_len.sum())
    want = composer.compose(plan)
    ref = want.signals[0]
    pcm_host, bg_host = composer.pool.data.cpu().numpy(), composer.background.data.cpu().numpy()
    assert torch.equal(host_compose(pcm_host, bg_host, plan, dev), ref)
    assert torch.equal(torch_compose(composer.pool.data, composer.background.data, plan), ref)
    i16 = composer.compose(plan, floats=False, pcm=True).pcm
    assert torch.equal(i16, (ref * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16))
    del want, i16
    dst32, dst16 = torch.empty_like(ref), torch.empty(total, dtype=torch.int16, device=dev)
    src16 = torch.empty(total, dtype=torch.int16, device=dev)
    fast = {"compose_f32_ms": lambda: composer.compose(plan), "compose_i16_ms": lambda: composer.compose(plan, floats=False, pcm=True),
            "copy_f32_ms": lambda: dst32.copy_(ref), "copy_i16_ms": lambda: dst16.copy_(src16)}

    def with_run(run):                                  # TCR_TUNE_COMPOSE_RUN: tiles per workgroup (the default is 4)
        def call():
            composer.lib.tcr_tune(34, run)
            try:
                return composer.compose(plan)
            finally:
                composer.lib.tcr_tune(34, 0)
        return call

    for run in (1, 2, 8):
        assert torch.equal(with_run(run)().signals[0], ref)
        fast[f"compose_f32_run{run}_ms"] = with_run(run)
    slow = {"host_ms": lambda: host_compose(pcm_host, bg_host, plan, dev), "torch_ms": lambda: torch_compose(composer.pool.data, composer.background.data, plan)}
    for fn in fast.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in list(fast) + list(slow)}
    for r in range(args.reps):
        for k, fn in fast.items():
            res[k].append(time_ms(fn))
        if r < args.slow_reps:
            for k, fn in slow.items():
                res[k].append(time_ms(fn))
    med = {k: round(statistics.median(v), 4) for k, v in res.items()}
    row = {"workload": f"{name}: {plan.n_recordings} recordings, {total / SR / 3600:.3f} h, {len(plan.place_len)} placements of {CLIP} samples "
                       f"(gaps 1.5 - 2.5 s, snr_db 0 .. 20), background volume 0.1 over {len(composer.background)} x 60 s",
           **med, "reps": args.reps, "slow_reps": args.slow_reps}
    moved32, moved16 = 4.0 * total + 2.0 * total + 2.0 * placed, 2.0 * total + 2.0 * total + 2.0 * placed
    row.update(compose_f32_GBps=round(moved32 / med["compose_f32_ms"] / 1e6, 1), compose_i16_GBps=round(moved16 / med["compose_i16_ms"] / 1e6, 1),
               copy_f32_GBps=round(8.0 * total / med["copy_f32_ms"] / 1e6, 1), copy_i16_GBps=round(4.0 * total / med["copy_i16_ms"] / 1e6, 1),
               speedup_over_host=round(med["host_ms"] / med["compose_f32_ms"], 1), speedup_over_torch=round(med["torch_ms"] / med["compose_f32_ms"], 1),
               raw={k: [round(x, 4) for x in v] for k, v in res.items()})
    return row


def energy_row(args, data, lengths, lib):
    dev = data.device
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    n_clip = int((np.asarray(lengths) == CLIP).sum())
    got = pcm_energy(data, offsets, lengths, lib)

    def by_torch():
        parts = [data[i * CLIP:min(i + 8192, n_clip) * CLIP].view(-1, CLIP).long().pow_(2).sum(1) for i in range(0, n_clip, 8192)]
        tail = [data[o:o + m].long().pow_(2).sum().reshape(1) for o, m in zip(offsets[n_clip:].tolist(), lengths[n_clip:])]
        return torch.cat(parts + tail)

    assert torch.equal(got, by_torch())
    dst = torch.empty_like(data)
    legs = {"energy_ms": lambda: pcm_energy(data, offsets, lengths, lib), "energy_torch_ms": by_torch, "energy_copy_ms": lambda: dst.copy_(data)}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(time_ms(fn))
    med = {k: round(statistics.median(v), 4) for k, v in res.items()}
    nbytes = 2.0 * data.numel()
    return {"workload": f"{n_clip} clips of {CLIP} samples and {len(lengths) - n_clip} of {MINUTE} in one call", **med,
            "energy_GBps": round(nbytes / med["energy_ms"] / 1e6, 1), "energy_copy_GBps": round(2 * nbytes / med["energy_copy_ms"] / 1e6, 1),
            "raw": {k: [round(x, 4) for x in v] for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow_reps", type=int, default=2, help="timed calls of the host and torch baselines")
    ap.add_argument("--pool", type=int, default=100000, help="one-second clips in the pool")
    ap.add_argument("--shapes", default="hours,ragged")
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, lib = torch.device("cuda"), _lib.get()
    n_bg = 6
    g = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(-20000, 20000, (args.pool * CLIP + n_bg * MINUTE,), device=dev, generator=g, dtype=torch.int32).to(torch.int16)
    lengths = [CLIP] * args.pool + [MINUTE] * n_bg
    pool, bg = view_pool(data[:args.pool * CLIP], lengths[:args.pool], lib), view_pool(data[args.pool * CLIP:], lengths[args.pool:], lib)
    composer = Composer(pool, np.arange(args.pool) % 10 + 2, [f"c{i}" for i in range(12)], bg)
    rows = {"energy": energy_row(args, data, lengths, lib)}
    print(json.dumps({"energy": rows["energy"]}), flush=True)
    shapes = {"hours": (f"{args.signals}x3600s", [3600.0] * args.signals),
              "ragged": ("255x1-10s+600s", (corpus_steps() * HOP / SR).tolist())}
    for key in args.shapes.split(","):
        name, seconds = shapes[key]
        rows[name] = shape_row(args, composer, name, seconds)
        print(json.dumps({name: {k: v for k, v in rows[name].items() if k != "raw"}}), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "compose_tile": _lib.COMPOSE_TILE, **rows}, fh, indent=1)


if __name__ == "__main__":
    main()
