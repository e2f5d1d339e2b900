"""Time of a detection sweep (KeywordScanner.sweep / detection_sweep: tcr_detect_sweep, T thresholds in one call) over the top / score
of a scan of 64 x 1-hour signals, next to the scan of the same audio.  TCResNet8-1.0 at 4020, k = 1, the default detector settings
(W = 50, min_count 3, suppression 75 steps), noise in 1 s segments of random loudness; T = 256 thresholds at quantiles of the warm scores; one labelled event per 10 s of
audio (1 s long, random labels) for the scored legs.

    python scripts/sweep_bench.py [--reps 5] [--out profiles/sweep_bench.json]
    python scripts/sweep_bench.py --trace_one         # each sweep leg twice (for rocprofv3 --kernel-trace --stats)

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

from tcresnet_amd.scanning import KeywordScanner, detection_sweep     # noqa: E402
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


if __name__ == "__main__":
    main()
