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
    python scripts/scan_bench.py --ragged_push [--out profiles/stream_scan_ragged_bench.json]
    python scripts/scan_bench.py --cascade [--out profiles/scan_cascade_bench.json]

--ragged: KeywordScanner.scan_ragged (tcr_scan_ragged) over a seeded corpus of 255 signals of 1 - 10 s (whole steps) and one of
10 min, next to the padded dense scan of the same corpus ([256, 10 min], what a caller without it runs) and the dense scan of 256
equal-length signals with the same total audio; the group size the call picks (the library's rule, restated here) and the ratio of
the front-end frames it computes to the live ones (steps x k) are reported with the times.  --trace_one --ragged runs the ragged
scan once after a warm-up.  --ab_lib: the 1 x 1 h and 64 x 1 min dense scans through this build and through the library given
(scripts/build_ref_lib.py), alternating in one process; so do a dense push_many (256 streams x 10 s), the ragged scan of the
--ragged corpus and that corpus as one push_ragged of 256 streams: the four scan entries.

--ragged_push: StreamingDetector.push_ragged (tcr_stream_scan_ragged).  server: S = 4096 streams that advance by 0 - 3 steps each
(seed 0) in one call, next to the lockstep prepared push and push_many of 1 and 2 steps per stream (the ragged call's mean is 1.5):
device time and wall time per call -- the ragged call uploads its offset tables and waits, which device events alone do not
show -- and per advanced step.  corpus: the --ragged corpus pushed in 10 s chunks, every stream its next min(10 s, what remains),
next to the one-call scan_ragged and the lockstep push_many of the corpus zero-padded to the longest, in the same chunks.  host: the
wall time of one call of one step per stream on an idle device, push_ragged against push_many, at S = 1 and S = 4096 (the
difference is the table upload and its wait), next to a host-to-device copy of a table of that size followed by a stream wait.

--cascade: a two-stage scan (scanning.CascadeScanner) of 64 recordings of one minute: TCResNet8-1.0 first, DS-CNN-L second, both 4020
at k = 1, W = 50.  The selected share is set directly: runs of 2 x 49 + 1 steps (the default pads around one flag) at seeded places,
1 %, 5 %, 25 % and 100 % of the steps.  Timed: the first scan, the second model's full scan_ragged (what a caller without the
cascade runs), KeywordScanner.scan_steps of the second model at each share, and the whole CascadeScanner.scan_ragged at each share
(its first stage is the real scan followed by a copy that plants the flags of that share in its probs); with each share the
front-end rows staged and the windows run (KeywordScanner.steps_plan).  This arm reports the minimum over --reps.

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

from tcresnet_amd.scanning import DEFAULT_MAX_WINDOWS, CascadeScanner, KeywordScanner     # noqa: E402
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
    steps = corpus_steps()
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


def corpus_steps():
    """The --ragged corpus: 255 signals of 1 - 10 s and one of 10 min, in steps (seed 0)."""
    import numpy as np
    rng = np.random.RandomState(0)
    return np.concatenate([rng.randint(SR // HOP, 10 * SR // HOP + 1, 255), [600 * SR // HOP]]).astype(np.int64)


def wall_ms(fn, iters=1):
    """Host time of `iters` calls on an idle device, the device's work included."""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / iters


def ragged_push_leg(args, fe, net, dev):
    import numpy as np
    g = torch.Generator(device="cuda").manual_seed(0)
    noise = lambda *shape: ((torch.rand(shape, device=dev, generator=g) - 0.5) * 0.8).contiguous()      # noqa: E731
    legs = {}
    # (a) the server shape
    S = 4096
    m = np.random.RandomState(0).randint(0, 4, S).astype(np.int64)
    advanced = int(m.sum())
    srv = StreamingDetector(net, fe, S, average_window_ms=1000)
    packed, lengths = noise(advanced * HOP), (m * HOP).tolist()
    x1, x2 = noise(S, HOP), noise(S, 2 * HOP)
    step = srv.prepared(x1)
    ragged = lambda: srv.push_ragged((packed, lengths))          # noqa: E731
    legs["server_ragged_ms"] = lambda: time_ms(ragged, 20)
    legs["server_ragged_wall_ms"] = lambda: wall_ms(ragged, 20)
    legs["server_push_ms"] = lambda: time_ms(step, 200)
    legs["server_push_wall_ms"] = lambda: wall_ms(step, 200)
    legs["server_push_many_1_ms"] = lambda: time_ms(lambda: srv.push_many(x1), 20)
    legs["server_push_many_1_wall_ms"] = lambda: wall_ms(lambda: srv.push_many(x1), 20)
    legs["server_push_many_2_ms"] = lambda: time_ms(lambda: srv.push_many(x2), 20)
    legs["server_push_many_2_wall_ms"] = lambda: wall_ms(lambda: srv.push_many(x2), 20)
    # (b) the corpus shape
    steps = corpus_steps()
    N, total, chunk = len(steps), int(steps.sum()), 10 * SR // HOP
    corpus = noise(total * HOP)
    first = np.concatenate([[0], np.cumsum(steps)])[:-1] * HOP
    cor_len = (steps * HOP).tolist()
    padded = torch.zeros((N, int(steps.max()) * HOP), device=dev)
    for n in range(N):
        padded[n, :cor_len[n]] = corpus[first[n]:first[n] + cor_len[n]]
    pieces = []
    for i0 in range(0, int(steps.max()), chunk):
        ms_ = np.clip(steps - i0, 0, chunk)
        pieces.append((torch.cat([corpus[first[n] + i0 * HOP:first[n] + (i0 + ms_[n]) * HOP] for n in range(N)]), (ms_ * HOP).tolist()))
    pad_pieces = [padded[:, i0 * HOP:(i0 + chunk) * HOP].contiguous() for i0 in range(0, int(steps.max()), chunk)]
    det = StreamingDetector(net, fe, N, average_window_ms=1000)
    scanner = KeywordScanner(net, fe, average_window_ms=1000)
    everyone = np.ones(N, bool)

    def chunked():
        det.reset(everyone)
        for piece in pieces:
            det.push_ragged(piece)

    def lockstep():
        det.reset(everyone)
        for piece in pad_pieces:
            det.push_many(piece)
    legs["corpus_push_ragged_10s_ms"] = lambda: wall_ms(chunked)
    legs["corpus_scan_ragged_ms"] = lambda: wall_ms(lambda: scanner.scan_ragged((corpus, cor_len)))
    legs["corpus_padded_push_many_10s_ms"] = lambda: wall_ms(lockstep)
    # (c) the host cost of a call
    for s_ in (1, S):
        d = srv if s_ == S else StreamingDetector(net, fe, 1, average_window_ms=1000)
        xs, one = noise(s_, HOP), [HOP] * s_
        table = torch.zeros(2 * (s_ + 1), dtype=torch.int64)
        table_dev = torch.zeros(2 * (s_ + 1), dtype=torch.int64, device=dev)

        def upload(table=table, table_dev=table_dev):
            table_dev.copy_(table, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        legs["host_s%d_push_ragged_wall_us" % s_] = lambda d=d, xs=xs, one=one: 1000.0 * wall_ms(lambda: d.push_ragged((xs.view(-1), one)), 50)
        legs["host_s%d_push_many_wall_us" % s_] = lambda d=d, xs=xs: 1000.0 * wall_ms(lambda: d.push_many(xs), 50)
        legs["host_s%d_table_copy_and_wait_us" % s_] = lambda upload=upload: 1000.0 * wall_ms(upload, 200)
    for fn in legs.values():
        fn()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    rnd = lambda v: round(v, 4)                                      # noqa: E731
    row = {
        "workload": "TCResNet8-1.0, 4020, k = 1, W = 50, max_windows = %d" % DEFAULT_MAX_WINDOWS,
        "server": {"streams": S, "steps_per_stream": "0 - 3 (seed 0)", "advanced_steps": advanced,
                   "streams_without_steps": int((m == 0).sum()),
                   "push_ragged_ms": rnd(med["server_ragged_ms"]), "push_ragged_wall_ms": rnd(med["server_ragged_wall_ms"]),
                   "push_ragged_wall_us_per_step": rnd(1000.0 * med["server_ragged_wall_ms"] / advanced),
                   "push_ms": rnd(med["server_push_ms"]), "push_wall_ms": rnd(med["server_push_wall_ms"]),
                   "push_wall_us_per_step": rnd(1000.0 * med["server_push_wall_ms"] / S),
                   "push_many_1_ms": rnd(med["server_push_many_1_ms"]), "push_many_1_wall_ms": rnd(med["server_push_many_1_wall_ms"]),
                   "push_many_1_wall_us_per_step": rnd(1000.0 * med["server_push_many_1_wall_ms"] / S),
                   "push_many_2_ms": rnd(med["server_push_many_2_ms"]), "push_many_2_wall_ms": rnd(med["server_push_many_2_wall_ms"]),
                   "push_many_2_wall_us_per_step": rnd(1000.0 * med["server_push_many_2_wall_ms"] / (2 * S))},
        "corpus": {"signals": N, "total_steps": total, "chunk_steps": chunk, "chunks": len(pieces),
                   "padded_steps": N * int(steps.max()),
                   "push_ragged_10s_chunks_ms": rnd(med["corpus_push_ragged_10s_ms"]),
                   "scan_ragged_one_call_ms": rnd(med["corpus_scan_ragged_ms"]),
                   "padded_push_many_10s_chunks_ms": rnd(med["corpus_padded_push_many_10s_ms"])},
        "host": {("s%d" % s_): {"push_ragged_wall_us": rnd(med["host_s%d_push_ragged_wall_us" % s_]),
                                "push_many_wall_us": rnd(med["host_s%d_push_many_wall_us" % s_]),
                                "difference_us": rnd(med["host_s%d_push_ragged_wall_us" % s_] - med["host_s%d_push_many_wall_us" % s_]),
                                "table_copy_and_wait_us": rnd(med["host_s%d_table_copy_and_wait_us" % s_])} for s_ in (1, S)},
        "reps": args.reps, "raw": {k: [rnd(x) for x in v] for k, v in res.items()},
    }
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "command": "python scripts/scan_bench.py --ragged_push --reps %d" % args.reps,
                       **row}, fh, indent=1)


class PlantedFlags:
    """A first-stage scanner whose scan_ragged is the real scan followed by a copy of `probs` over its probs: the flags of a
    chosen share (--cascade).  Everything else is the scanner's own."""

    def __init__(self, scanner, probs):
        self._scanner, self._probs = scanner, probs

    def __getattr__(self, name):
        return getattr(self._scanner, name)

    def scan_ragged(self, signals):
        out = self._scanner.scan_ragged(signals)
        out.probs.copy_(self._probs)
        return out


def cascade_leg(args, dev):
    import numpy as np
    fe1, net1 = build(640, HOP, "TCResNet8", 1.0, dev)
    _, fe2, net2 = build_model("DSCNN-L", dev)
    first = KeywordScanner(net1, fe1, average_window_ms=1000)
    second = KeywordScanner(net2, fe2, average_window_ms=1000)
    N, steps = 64, 60 * SR // HOP
    total, pad = N * steps, second.average_steps - 1
    run = 2 * pad + 1
    g = torch.Generator(device="cuda").manual_seed(0)
    packed = ((torch.rand(total * HOP, device=dev, generator=g) - 0.5) * 0.8).contiguous()
    signals = (packed, [steps * HOP] * N)
    # the places a run may take: `run` steps apart within a signal, so that the pads never leave it
    slots = np.array([n * steps + j * run + pad for n in range(N) for j in range(steps // run)], np.int64)
    rng = np.random.RandomState(0)
    shares, legs, plans = (0.01, 0.05, 0.25, 1.0), {}, {}
    legs["first_scan_ms"] = lambda: time_ms(lambda: first.scan_ragged(signals))
    legs["second_full_scan_ms"] = lambda: time_ms(lambda: second.scan_ragged(signals))
    full = second.scan_ragged(signals)
    for share in shares:
        probs = torch.zeros((total, 12), device=dev)
        if share == 1.0:
            probs[:, 2] = 1.0
            selected = np.arange(total, dtype=np.int64)
        else:
            centres = np.sort(rng.choice(slots, int(round(share * total / run)), replace=False))
            probs[torch.from_numpy(centres).to(dev), 2] = 1.0
            selected = np.unique((centres[:, None] + np.arange(-pad, pad + 1)[None, :]).reshape(-1))
        cascade = CascadeScanner(PlantedFlags(first, probs), second, 0.5)
        out = cascade.scan_ragged(signals)
        assert np.array_equal(out.selected.cpu().numpy(), selected), share
        logits, _ = second.scan_steps(signals, selected)
        assert torch.equal(logits, full.logits[out.selected]), share          # the rows of the full scan, bitwise
        tag = "%g" % (100 * share)
        plans[tag] = {"selected_steps": int(selected.size), "share": round(selected.size / total, 5), **second.steps_plan(signals, selected)}
        legs["scan_steps_%s_ms" % tag] = lambda selected=selected: time_ms(lambda: second.scan_steps(signals, selected))
        legs["cascade_%s_ms" % tag] = lambda cascade=cascade: time_ms(lambda: cascade.scan_ragged(signals))
    for fn in legs.values():
        fn()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(fn())
    low = {k: min(v) for k, v in res.items()}
    G, frames = ragged_group(np.full(N, steps), 1, fe2.n_frames, min(1024, DEFAULT_MAX_WINDOWS))
    hours = total * HOP / HOUR
    row = {
        "workload": "TCResNet8-1.0 then DS-CNN-L, 4020, k = 1, W = 50, max_windows = %d; 64 recordings of 60 s; runs of %d steps" % (
            DEFAULT_MAX_WINDOWS, run),
        "signals": N, "total_steps": total, "audio_hours": round(hours, 5),
        "first_scan_ms": round(low["first_scan_ms"], 3), "second_full_scan_ms": round(low["second_full_scan_ms"], 3),
        "second_full_scan": {"group_steps": G, "rows": frames // (G + fe2.n_frames - 1), "row_frames": G + fe2.n_frames - 1, "windows": total},
        "shares": {tag: {**plans[tag], "scan_steps_ms": round(low["scan_steps_%s_ms" % tag], 3),
                         "cascade_ms": round(low["cascade_%s_ms" % tag], 3),
                         "scan_steps_over_full_scan": round(low["scan_steps_%s_ms" % tag] / low["second_full_scan_ms"], 4),
                         "cascade_over_full_scan": round(low["cascade_%s_ms" % tag] / low["second_full_scan_ms"], 4)} for tag in plans},
        "reps": args.reps, "statistic": "min", "raw": {k: [round(x, 4) for x in v] for k, v in res.items()},
    }
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "command": "python scripts/scan_bench.py --cascade --reps %d" % args.reps,
                       **row}, fh, indent=1)


def ab_leg(args, dev):
    """The four scan entries through this build and through --ab_lib, alternating: medians and ranges of both."""
    import tcresnet_amd as T
    from oracle import numpy_ref as R
    libs = {"this": T._lib.get(), "other": T._lib.load_from(args.ab_lib, "hip", allow_missing=True)}
    arch = R.make_tcresnet("TCResNet8", 1.0)
    p, s = R.init_params(arch, 0)
    R.randomize_bn(arch, p, s)
    g = torch.Generator(device="cuda").manual_seed(0)
    hour = ((torch.rand((1, HOUR), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    minutes = ((torch.rand((64, 60 * SR), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    ten = ((torch.rand((256, 10 * SR), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    steps = corpus_steps()
    corpus = ((torch.rand(int(steps.sum()) * HOP, device=dev, generator=g) - 0.5) * 0.8).contiguous()
    cor_len = (steps * HOP).tolist()
    legs = {}
    for name, lib in libs.items():
        fe = T.Frontend(window_size_samples=640, window_stride_samples=HOP, device=dev, lib=lib)
        net = T.TCResNet("TCResNet8", R.tcresnet_channels("TCResNet8", 1.0), 40, fe.n_frames, 12, device=dev, lib=lib)
        net.load_state_dict({**p, **s})
        sc = KeywordScanner(net, fe, average_window_ms=1000)
        legs[name + "_scan_1x1h_ms"] = lambda sc=sc: time_ms(lambda: sc.scan(hour))
        legs[name + "_scan_64x1min_ms"] = lambda sc=sc: time_ms(lambda: sc.scan(minutes))
        st = StreamingDetector(net, fe, 256, average_window_ms=1000)
        legs[name + "_push_many_256x10s_ms"] = lambda st=st: time_ms(lambda: st.push_many(ten))
        legs[name + "_scan_ragged_corpus_ms"] = lambda sc=sc: time_ms(lambda: sc.scan_ragged((corpus, cor_len)))
        legs[name + "_push_ragged_corpus_ms"] = lambda st=st: time_ms(lambda: st.push_ragged((corpus, cor_len)))
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
    ap.add_argument("--ragged_push", action="store_true")
    ap.add_argument("--cascade", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.cascade:
        return cascade_leg(args, dev)
    if args.ab_lib:
        return ab_leg(args, dev)
    if args.ragged_push:
        return ragged_push_leg(args, *build(640, HOP, "TCResNet8", 1.0, dev), dev)
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
