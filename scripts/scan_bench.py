"""Time of an offline scan (KeywordScanner.scan: tcr_scan, every step of every signal in one call) per audio-hour, next to the
network alone on the same number of windows (TCResNet.forward_frozen at the scan's chunk size on pre-gathered windows) and the
prepared streaming detector at S = 1 (StreamingDetector.prepared, extrapolated from --stream_steps steps).  TCResNet8-1.0 at 4020,
k = 1, W = 50 (average_window_ms = 1000), default max_windows.  --model DSCNN-L / kws_low_latency_conv (stream_bench.build_model)
times that model instead; its network alone is the engine's forward_infer on planar windows (the 2-D graph's includes the
relayout into its planes, which the scan's gather writes directly).

    python scripts/scan_bench.py [--reps 5] [--out profiles/scan_bench.json]
    python scripts/scan_bench.py --model DSCNN-L [--out profiles/scan_bench_dscnn_l.json]
    python scripts/scan_bench.py --trace_one         # one 1-hour scan after a warm-up (for rocprofv3 --kernel-trace --stats)

Each number is the median over --reps timed calls (device events) after a warm-up call; the legs alternate within a rep.  Weights
and audio are random (timing does not depend on them)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd.scanning import DEFAULT_MAX_WINDOWS, KeywordScanner     # noqa: E402
from tcresnet_amd.streaming import StreamingDetector                       # noqa: E402
from scripts.stream_bench import MODELS, build, build_model                # noqa: E402

SR, HOP = 16000, 320
HOUR = 3600 * SR


def time_ms(fn, iters=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stream_steps", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace_one", action="store_true")
    ap.add_argument("--model", default="TCResNet8", choices=MODELS)
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.model == "TCResNet8":
        fe, net = build(640, HOP, "TCResNet8", 1.0, dev)
    else:
        _, fe, net = build_model(args.model, dev)
    scanner = KeywordScanner(net, fe, average_window_ms=1000)
    assert scanner.average_steps == 50
    g = torch.Generator(device="cuda").manual_seed(0)
    hour = ((torch.rand((1, HOUR), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    if args.trace_one:
        scanner.scan(hour)
        torch.cuda.synchronize()
        scanner.scan(hour)
        torch.cuda.synchronize()
        print("traced one 1-hour scan after a warm-up")
        return
    minutes = ((torch.rand((64, 60 * SR), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    B = DEFAULT_MAX_WINDOWS
    windows = fe(((torch.rand((B, fe.n_samples), device=dev, generator=g) - 0.5) * 0.8).contiguous())
    if args.model == "TCResNet8":
        ss = net.fold_bn()
        net_alone = lambda: net.forward_frozen(windows, ss)     # noqa: E731
    else:
        net_alone = lambda: net.forward_infer(windows)          # noqa: E731
    hour_windows = HOUR // HOP
    n_batches = hour_windows / B
    stream = StreamingDetector(net, fe, 1, average_window_ms=1000)
    step = stream.prepared(((torch.rand((1, HOP), device=dev, generator=g) - 0.5) * 0.8).contiguous())
    legs = {
        "scan_1x1h_ms": lambda: time_ms(lambda: scanner.scan(hour)),
        "scan_64x1min_ms": lambda: time_ms(lambda: scanner.scan(minutes)),
        "net_alone_batch_ms": lambda: time_ms(net_alone, 20),
        "stream_s1_step_us": lambda: 1000.0 * time_ms(step, args.stream_steps),
    }
    for fn in legs.values():                            # warm-up
        fn()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    row = {
        "workload": "%s, 4020, k = 1, W = 50, max_windows = %d" % ("TCResNet8-1.0" if args.model == "TCResNet8" else args.model, B),
        "scan_1h_ms": round(med["scan_1x1h_ms"], 3),
        "scan_1h_ms_range": [round(min(res["scan_1x1h_ms"]), 3), round(max(res["scan_1x1h_ms"]), 3)],
        "scan_64x1min_ms": round(med["scan_64x1min_ms"], 3),
        "scan_64x1min_ms_per_audio_hour": round(med["scan_64x1min_ms"] * 60 / 64, 3),
        "net_alone_batch_%d_ms" % B: round(med["net_alone_batch_ms"], 4),
        "net_alone_1h_windows_ms": round(med["net_alone_batch_ms"] * n_batches, 3),
        "scan_over_net_alone_1h": round(med["scan_1x1h_ms"] / (med["net_alone_batch_ms"] * n_batches), 3),
        "stream_s1_step_us": round(med["stream_s1_step_us"], 2),
        "stream_s1_steps_timed": args.stream_steps,
        "stream_s1_per_audio_hour_ms": round(med["stream_s1_step_us"] * hour_windows / 1000.0, 1),
        "reps": args.reps,
        "raw": {k: [round(x, 4) for x in v] for k, v in res.items()},
    }
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), **row}, fh, indent=1)


if __name__ == "__main__":
    main()
