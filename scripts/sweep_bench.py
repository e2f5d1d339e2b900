"""Time of a detection sweep (KeywordScanner.sweep / detection_sweep: tcr_detect_sweep, T thresholds in one call) over the top / score
of a scan of 64 x 1-hour signals, next to the scan of the same audio.  TCResNet8-1.0 at 4020, k = 1, the default detector settings
(W = 50, min_count 3, suppression 75 steps), noise in 1 s segments of random loudness; T = 256 thresholds at quantiles of the warm scores; one labelled event per 10 s of
audio (1 s long, random labels) for the scored legs.

    python scripts/sweep_bench.py [--reps 5] [--out profiles/sweep_bench.json]
    python scripts/sweep_bench.py --trace_one         # each sweep leg twice (for rocprofv3 --kernel-trace --stats)
    python scripts/sweep_bench.py --grid [--kernel_stats DIR] [--out profiles/detect_grid_bench.json]
    python scripts/sweep_bench.py --grid --trace_one  # the grid call twice (for rocprofv3 --kernel-trace --stats -d DIR)

--grid: the detector grid (tcr_detect_grid) on the same shape: 3 windows x 3 min_counts x 3 suppressions x T thresholds from the scan's
probs, next to 27 x (redetect + sweep) and to what there was before it, 27 x (scan + sweep).  The probs rotate through three copies
(1.6 GB, past the 256 MB Infinity Cache) so that no leg finds its input cached by the one before.  --kernel_stats DIR adds the kernels'
own times from the *kernel_stats.csv of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR` run of --grid --trace_one.

Each number is the median over --reps timed calls (device events around the Python call: the host's event / threshold copies
included) after a warm-up call; the legs alternate within a rep.  Weights and audio are random."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd.scanning import KeywordScanner, ScanOutput, detection_grid, detection_sweep     # noqa: E402
from scripts.stream_bench import build                                # noqa: E402
from scripts.scan_bench import time_ms                                # noqa: E402

SR, HOP = 16000, 320
HOUR = 3600 * SR


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--thresholds", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace_one", action="store_true")
    ap.add_argument("--grid", action="store_true", help="the detector-grid leg (tcr_detect_grid)")
    ap.add_argument("--kernel_stats", default=None, help="--grid: directory of a rocprofv3 --kernel-trace --stats run of --grid --trace_one")
    args = ap.parse_args()
    dev = torch.device("cuda")
    fe, net = build(640, HOP, "TCResNet8", 1.0, dev)
    scanner = KeywordScanner(net, fe)
    N, T = args.signals, args.thresholds
    g = torch.Generator(device="cuda").manual_seed(0)
    # noise in 1 s segments of random loudness (0.01 or 0.5): the random net's top class moves with it
    loud = torch.where(torch.rand((N, HOUR // SR), device=dev, generator=g) < 0.5, 0.01, 0.5).repeat_interleave(SR, dim=1)
    audio = ((torch.rand((N, HOUR), device=dev, generator=g) - 0.5) * 2).mul_(loud).contiguous()
    del loud
    out = scanner.scan(audio)
    steps = int(out.top.shape[1])
    warm = out.score[out.top >= 0].float()
    thr = torch.quantile(warm[torch.randperm(warm.numel(), device=dev, generator=g)[:1 << 24]],
                         torch.linspace(0, 1, T, device=dev)).cpu().numpy().astype(np.float32)
    rng = np.random.RandomState(0)
    starts = np.arange(0, steps - 50, 500, dtype=np.int64)
    events = [np.stack([starts, starts + 49, rng.randint(12, size=len(starts))], axis=1) for _ in range(N)]
    if args.grid:
        return grid_leg(args, fe, net, scanner, audio, out, thr, events)
    supp = scanner.suppression_steps
    one = (out.top[:1].contiguous(), out.score[:1].contiguous())
    sweep = lambda top, score, ev=None, fired=False: detection_sweep(top, score, thr, supp, 12, events=ev, step_seconds=HOP / SR,
                                                                     return_fired=fired)
    legs = {
        "sweep_events_ms": lambda: time_ms(lambda: sweep(out.top, out.score, events)),
        "sweep_no_events_ms": lambda: time_ms(lambda: sweep(out.top, out.score)),
        "sweep_events_fired_ms": lambda: time_ms(lambda: sweep(out.top, out.score, events, True)),
        "sweep_1x1h_events_ms": lambda: time_ms(lambda: sweep(*one, events[:1])),
        "scan_ms": lambda: time_ms(lambda: scanner.scan(audio)),
    }
    if args.trace_one:
        for k in ("sweep_events_ms", "sweep_no_events_ms", "sweep_1x1h_events_ms"):
            legs[k]()
            torch.cuda.synchronize()
            legs[k]()
            torch.cuda.synchronize()
        print("traced each sweep leg twice (warm-up + one)")
        return
    for fn in legs.values():                            # warm-up
        fn()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    r = sweep(out.top, out.score, events)
    detections = int(r.detections.sum())
    row = {
        "workload": f"TCResNet8-1.0, 4020, k = 1, default detector (suppression {supp} steps); {N} x 1 h signals ({steps} steps each), "
                    f"T = {T} thresholds at quantiles of the warm scores, {sum(len(e) for e in events)} events",
        "sweep_ms": round(med["sweep_events_ms"], 3),
        "sweep_ms_range": [round(min(res["sweep_events_ms"]), 3), round(max(res["sweep_events_ms"]), 3)],
        "sweep_no_events_ms": round(med["sweep_no_events_ms"], 3),
        "sweep_with_fired_ms": round(med["sweep_events_fired_ms"], 3),
        "sweep_1x1h_ms": round(med["sweep_1x1h_events_ms"], 3),
        "scan_ms": round(med["scan_ms"], 2),
        "sweep_over_scan": round(med["sweep_events_ms"] / med["scan_ms"], 4),
        "rescans_ms_estimate": round(med["scan_ms"] * T, 0),
        "detections_summed_over_thresholds": detections,
        "reps": args.reps,
        "raw": {k: [round(x, 4) for x in v] for k, v in res.items()},
    }
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), **row}, fh, indent=1)


GRID = dict(average_window_ms=(500, 1000, 2000), min_count=(1, 3, 5), suppression_ms=(750, 1500, 3000))


def kernel_stats(directory):
    """{kernel name (up to its arguments): (calls, average ms)} of a rocprofv3 --stats run."""
    import csv
    import glob
    rows = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows[r["Name"].split("(")[0]] = (int(r["Calls"]), float(r["AverageNs"]) / 1e6)
    return rows


def grid_leg(args, fe, net, scanner, audio, out, thr, events):
    import itertools
    N, steps = int(out.top.shape[0]), int(out.top.shape[1])
    combos = list(itertools.product(*GRID.values()))
    scanners = [KeywordScanner(net, fe, average_window_ms=w, min_count=mc, suppression_ms=sp) for w, mc, sp in combos]
    points = [(s.det.average_steps, s.det.min_count, s.det.suppression_steps) for s in scanners]
    probs = [out.probs, out.probs.clone(), out.probs.clone()]
    turn = [0]

    def next_probs():
        turn[0] = (turn[0] + 1) % len(probs)
        return probs[turn[0]]

    grid = lambda: detection_grid(next_probs(), points, thr, 12, events=events, step_seconds=HOP / SR)

    def redetect_sweeps():
        for (w, mc, sp), pt in zip(combos, points):
            r = scanner.redetect(ScanOutput(None, next_probs(), None, None, None, None), average_window_ms=w, min_count=mc, suppression_ms=sp)
            detection_sweep(r.top, r.score, thr, pt[2], 12, events=events, step_seconds=HOP / SR)

    def scan_sweeps():
        for s, pt in zip(scanners, points):
            o = s.scan(audio)
            detection_sweep(o.top, o.score, thr, pt[2], 12, events=events, step_seconds=HOP / SR)

    if args.trace_one:
        for _ in range(2):
            grid()
            torch.cuda.synchronize()
        print("traced the grid call twice (warm-up + one)")
        return
    legs = {"grid_ms": grid, "redetect_sweeps_ms": redetect_sweeps, "scan_sweeps_ms": scan_sweeps}
    res = {k: [] for k in legs}
    for k, fn in legs.items():                          # warm-up; the two paths of the same tables agree
        fn()
    d = grid()
    o = scanners[-1].scan(audio)
    want = detection_sweep(o.top, o.score, thr, points[-1][2], 12, events=events)
    assert torch.equal(d[0][-1], want.detections) and torch.equal(d[1][-1], want.hits) and torch.equal(d[2][-1], want.duplicates)
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(time_ms(fn))
    med = {k: statistics.median(v) for k, v in res.items()}
    row = {
        "workload": f"TCResNet8-1.0, 4020, k = 1; {N} x 1 h signals ({steps} steps each), C = 12, T = {len(thr)} thresholds, "
                    f"{sum(len(e) for e in events)} events; grid {GRID} = {len(points)} points in steps {sorted(set(points))[:1]} .. "
                    f"({len(set(p[:2] for p in points))} (W, min_count) pairs, {len(set(p[0] for p in points))} windows); probs rotate through "
                    f"{len(probs)} copies of {out.probs.numel() * 4 / 2 ** 20:.0f} MB",
        "grid_ms": round(med["grid_ms"], 3),
        "redetect_plus_sweep_x27_ms": round(med["redetect_sweeps_ms"], 3),
        "scan_plus_sweep_x27_ms": round(med["scan_sweeps_ms"], 1),
        "grid_over_redetect_sweeps": round(med["grid_ms"] / med["redetect_sweeps_ms"], 4),
        "grid_over_scan_sweeps": round(med["grid_ms"] / med["scan_sweeps_ms"], 5),
        "reps": args.reps,
        "raw": {k: [round(x, 4) for x in v] for k, v in res.items()},
    }
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        row["kernels_from_trace"] = {k: {"calls": c, "average_ms": round(ms, 4)} for k, (c, ms) in ks.items()
                                     if "grid_smooth_kernel" in k or "sweep_kernel" in k}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), **row}, fh, indent=1)


if __name__ == "__main__":
    main()
