"""Time of many-step pushes (StreamingDetector.push_many: tcr_stream_scan) against the one-call scan (KeywordScanner.scan: tcr_scan)
of the same audio and against prepared pushes.  TCResNet8-1.0 at 4020, k = 1, the default detector settings, noise in 1 s segments of
random loudness.  Legs:
  chunked_64x1h  64 x 1-hour signals in 60 one-minute push_many calls (3000 steps each)  vs  scan_64x1h, one scan of the hour;
  chunked_1x1h   one 1-hour signal in 60 one-minute push_many calls                       vs  scan_1x1h;
  many_s1_50     S = 1, one push_many of 50 steps (1 s)                                   vs  prepared_s1_50, 50 prepared pushes.

    python scripts/stream_scan_bench.py [--reps 5] [--out profiles/stream_scan_bench.json]
    python scripts/stream_scan_bench.py --trace_one       # every leg once after a warm-up (for rocprofv3 --kernel-trace --stats)

Each number is the median over --reps timed calls (device events around the Python calls: output allocation included) after a
warm-up; the legs alternate within a rep.  Weights and audio are random."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd.scanning import KeywordScanner                      # noqa: E402
from tcresnet_amd.streaming import StreamingDetector                  # noqa: E402
from scripts.stream_bench import build                                # noqa: E402
from scripts.scan_bench import time_ms                                # noqa: E402

SR, HOP = 16000, 320
MINUTE = 60 * SR


def noise(n, length, dev, g):
    """Noise in 1 s segments of random loudness (0.01 or 0.5): the random net's top class moves with it."""
    loud = torch.where(torch.rand((n, length // SR), device=dev, generator=g) < 0.5, 0.01, 0.5).repeat_interleave(SR, dim=1)
    return ((torch.rand((n, length), device=dev, generator=g) - 0.5) * 2).mul_(loud).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace_one", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    fe, net = build(640, HOP, "TCResNet8", 1.0, dev)
    N, M = args.signals, args.minutes
    g = torch.Generator(device="cuda").manual_seed(0)
    chunks = [noise(N, MINUTE, dev, g) for _ in range(M)]               # [N, minute] each: what a caller reading files hands over
    whole = torch.cat(chunks, dim=1)
    one_chunks = [c[:1].contiguous() for c in chunks]
    one_whole = whole[:1].contiguous()
    scanner = KeywordScanner(net, fe)
    det_n, det_1 = StreamingDetector(net, fe, N), StreamingDetector(net, fe, 1)
    det_s1 = StreamingDetector(net, fe, 1)
    s1 = noise(1, SR, dev, g)
    buf = torch.zeros((1, HOP), device=dev)
    call = StreamingDetector(net, fe, 1).prepared(buf)
    steps_s1 = [s1[:, i * HOP:(i + 1) * HOP].contiguous() for i in range(SR // HOP)]

    def prepared_50():
        for x in steps_s1:
            buf.copy_(x)
            call()

    def chunked(det, parts):
        for c in parts:
            det.push_many(c)

    legs = {
        "chunked_64x1h_ms": lambda: time_ms(lambda: chunked(det_n, chunks)),
        "scan_64x1h_ms": lambda: time_ms(lambda: scanner.scan(whole)),
        "chunked_1x1h_ms": lambda: time_ms(lambda: chunked(det_1, one_chunks)),
        "scan_1x1h_ms": lambda: time_ms(lambda: scanner.scan(one_whole)),
        "many_s1_50_us": lambda: 1000.0 * time_ms(lambda: det_s1.push_many(s1)),
        "prepared_s1_50_us": lambda: 1000.0 * time_ms(prepared_50),
    }
    for fn in legs.values():                            # warm-up
        fn()
    if args.trace_one:
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        print("traced every leg once after a warm-up")
        return
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    rng = lambda k, d: [round(min(res[k]), d), round(max(res[k]), d)]
    row = {
        "workload": f"TCResNet8-1.0, 4020, k = 1, default detector; {N} x {M} min signals in {M} push_many calls of one minute "
                    f"({MINUTE // HOP} steps) vs one scan; S = 1: one push_many of 50 steps vs 50 prepared pushes",
        "chunked_64x1h_ms": round(med["chunked_64x1h_ms"], 2), "chunked_64x1h_ms_range": rng("chunked_64x1h_ms", 2),
        "scan_64x1h_ms": round(med["scan_64x1h_ms"], 2),
        "chunked_over_scan_64x1h": round(med["chunked_64x1h_ms"] / med["scan_64x1h_ms"], 4),
        "chunked_1x1h_ms": round(med["chunked_1x1h_ms"], 3), "chunked_1x1h_ms_range": rng("chunked_1x1h_ms", 3),
        "scan_1x1h_ms": round(med["scan_1x1h_ms"], 3),
        "chunked_over_scan_1x1h": round(med["chunked_1x1h_ms"] / med["scan_1x1h_ms"], 4),
        "many_s1_50_us": round(med["many_s1_50_us"], 1), "prepared_s1_50_us": round(med["prepared_s1_50_us"], 1),
        "prepared_over_many_s1_50": round(med["prepared_s1_50_us"] / med["many_s1_50_us"], 2),
        "targets": {"chunked_over_scan_64x1h": "<= 1.05", "chunked_over_scan_1x1h": "<= 1.3", "prepared_over_many_s1_50": ">= 10"},
        "reps": args.reps,
        "raw": {k: [round(x, 4) for x in v] for k, v in res.items()},
    }
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), **row}, fh, indent=1)


if __name__ == "__main__":
    main()
