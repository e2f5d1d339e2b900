"""Time of an offline scan (KeywordScanner.scan: tcr_scan, every step of every signal in one call) per audio-hour, next to the
network alone on the same number of windows (TCResNet.forward_frozen at the scan's chunk size on pre-gathered windows) and the
prepared streaming detector at S = 1 (StreamingDetector.prepared, extrapolated from --stream_steps steps).  TCResNet8-1.0 at 4020,
k = 1, W = 50 (average_window_ms = 1000), default max_windows.  --model DSCNN-L / kws_low_latency_conv (stream_bench.build_model)
times that model instead; its network alone is the engine's forward_infer on planar windows (the 2-D graph's includes the
relayout into its planes, which the scan's gather writes directly).

    python scripts/scan_bench.py [--reps 5] [--out profiles/scan_bench.json]
    python scripts/scan_bench.py --model DSCNN-L [--out profiles/scan_bench_dscnn_l.json]
    python scripts/scan_bench.py --trace_one         # one 1-hour scan after a warm-up (for rocprofv3 --kernel-trace --stats)
    python scripts/scan_bench.py --ragged [--out profiles/scan_ragged_bench.json]
    python scripts/scan_bench.py --ab_lib tc-resnet_amd/lib/side/libtcr_parent.so      # the dense legs against another build

--ragged: KeywordScanner.scan_ragged (tcr_scan_ragged) over a seeded corpus of 255 signals of 1 - 10 s (whole steps) and one of
10 min, next to the padded dense scan of the same corpus ([256, 10 min], what a caller without it runs) and the dense scan of 256
equal-length signals with the same total audio; the group size the call picks (the library's rule, restated here) and the ratio of
the front-end frames it computes to the live ones (steps x k) are reported with the times.  --trace_one --ragged runs the ragged
scan once after a warm-up.  --ab_lib: the 1 x 1 h and 64 x 1 min dense scans through this build and through the library given
(scripts/build_ref_lib.py), alternating in one process.

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


def ragged_group(steps, k, T, cap):
    """tcr_scan_ragged's choice (scan_ragged_chunking, csrc/scan.hip) when one row of `cap` steps fits the workspace: the G <= cap
    with the fewest front-end frames, the larger on ties; and those frames."""
    best, frames = None, None
    for G in range(min(cap, int(steps.max())), 0, -1):
        f = int(((steps + G - 1) // G).sum()) * (G * k + T - k)
        if frames is None or f < frames:
            best, frames = G, f
    return best, frames


def ragged_leg(args, fe, net, dev):
    import numpy as np
    scanner = KeywordScanner(net, fe, average_window_ms=1000)
    rng = np.random.RandomState(0)
    steps = np.concatenate([rng.randint(SR // HOP, 10 * SR // HOP + 1, 255), [600 * SR // HOP]]).astype(np.int64)
    total = int(steps.sum())
    g = torch.Generator(device="cuda").manual_seed(0)
    packed = ((torch.rand(total * HOP, device=dev, generator=g) - 0.5) * 0.8).contiguous()
    lengths = (steps * HOP).tolist()
    padded = torch.zeros((256, int(steps.max()) * HOP), device=dev)
    at = 0
    for n, m in enumerate(lengths):
        padded[n, :m] = packed[at:at + m]
        at += m
    equal = packed[:total // 256 * 256 * HOP].view(256, -1)
    ragged = lambda: scanner.scan_ragged((packed, lengths))          # noqa: E731
    if args.trace_one:
        ragged()
        torch.cuda.synchronize()
        ragged()
        torch.cuda.synchronize()
        print("traced one ragged scan after a warm-up")
        return
    legs = {"ragged_ms": lambda: time_ms(ragged), "padded_dense_ms": lambda: time_ms(lambda: scanner.scan(padded)),
            "equal_dense_ms": lambda: time_ms(lambda: scanner.scan(equal))}
    for fn in legs.values():
        fn()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    G, frames = ragged_group(steps, 1, fe.n_frames, min(1024, DEFAULT_MAX_WINDOWS))
    hours, eq_hours = total * HOP / HOUR, equal.numel() / HOUR
    row = {
        "workload": "TCResNet8-1.0, 4020, k = 1, W = 50, max_windows = %d; 255 signals of 1 - 10 s + one of 10 min (seed 0)" % DEFAULT_MAX_WINDOWS,
        "signals": 256, "total_steps": total, "audio_hours": round(hours, 5), "padded_audio_hours": round(padded.numel() / HOUR, 5),
        "group_steps": G, "frontend_frames": frames, "live_frames": total, "frame_ratio": round(frames / total, 4),
        "ragged_ms": round(med["ragged_ms"], 3), "ragged_ms_per_audio_hour": round(med["ragged_ms"] / hours, 3),
        "padded_dense_ms": round(med["padded_dense_ms"], 3), "padded_dense_ms_per_real_audio_hour": round(med["padded_dense_ms"] / hours, 3),
        "equal_dense_ms": round(med["equal_dense_ms"], 3), "equal_dense_ms_per_audio_hour": round(med["equal_dense_ms"] / eq_hours, 3),
        "ragged_over_equal_per_audio_hour": round(med["ragged_ms"] / hours / (med["equal_dense_ms"] / eq_hours), 3),
        "reps": args.reps, "raw": {k: [round(x, 4) for x in v] for k, v in res.items()},
    }
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), **row}, fh, indent=1)


def ab_leg(args, dev):
    """The dense scans through this build and through --ab_lib, alternating: medians and ranges of both."""
    import tcresnet_amd as T
    from oracle import numpy_ref as R
    libs = {"this": T._lib.get(), "other": T._lib.load_from(args.ab_lib, "hip", allow_missing=True)}
    arch = R.make_tcresnet("TCResNet8", 1.0)
    p, s = R.init_params(arch, 0)
    R.randomize_bn(arch, p, s)
    g = torch.Generator(device="cuda").manual_seed(0)
    hour = ((torch.rand((1, HOUR), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    minutes = ((torch.rand((64, 60 * SR), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    legs = {}
    for name, lib in libs.items():
        fe = T.Frontend(window_size_samples=640, window_stride_samples=HOP, device=dev, lib=lib)
        net = T.TCResNet("TCResNet8", R.tcresnet_channels("TCResNet8", 1.0), 40, fe.n_frames, 12, device=dev, lib=lib)
        net.load_state_dict({**p, **s})
        sc = KeywordScanner(net, fe, average_window_ms=1000)
        legs[name + "_scan_1x1h_ms"] = lambda sc=sc: time_ms(lambda: sc.scan(hour))
        legs[name + "_scan_64x1min_ms"] = lambda sc=sc: time_ms(lambda: sc.scan(minutes))
    for fn in legs.values():
        fn()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(fn())
    row = {"other": args.ab_lib, "reps": args.reps}
    for k, v in res.items():
        row[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), **row}, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stream_steps", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace_one", action="store_true")
    ap.add_argument("--model", default="TCResNet8", choices=MODELS)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--ab_lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.ab_lib:
        return ab_leg(args, dev)
    if args.ragged:
        return ragged_leg(args, *build(640, HOP, "TCResNet8", 1.0, dev), dev)
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
