"""Time of phrase detection (PhraseDetector.scores / .detect: tcr_phrase_scores and tcr_detect_redetect over its posteriors) on the scan
of 64 x 1-hour signals, next to the scan that produces their input and to what a user would write in torch for the unordered score.
TCResNet8-1.0 at 4020, k = 1, the default detector, scan_bench.py's audio (noise in 1 s segments of random loudness), C = 12; four
phrases of two and three words over eight distinct classes.

    python scripts/phrase_bench.py [--reps 5] [--out profiles/phrase_bench.json] [--seconds 3600] [--windows 75,150]

Legs (each the median over --reps timed calls after a warm-up call, device events around the Python call; the legs alternate within a
rep), per window w in steps, order and combiner:
  scores_*   PhraseDetector.scores over the scan's smoothed: one kernel
  detect_*   PhraseDetector.detect: the scores and the detector rule over them
  torch_w    the unordered product in plain torch: zeros in front, unfold over the window, amax, the product of the words' columns
             (its result is compared with scores_unordered_product's, bit for bit: `torch_equal`)
  scan       the scan the phrase detector reads.

    python scripts/phrase_bench.py --stream [--reps 5] [--out profiles/phrase_stream_bench.json] [--windows 75,150]

times streaming phrase detection (StreamingPhraseDetector.push: tcr_phrase_stream_push) in its two shapes, same phrases and windows:
  (a) server  S = 4096 live streams, one step a push: `step_ms` is StreamingDetector.push (front-end, network, detector), and
              push_* the phrase push of that step's output, each the time per call over --iters calls in a row between two device
              events, after more than a window of warm-up pushes (every ring is full); ratio_* = push / step.
  (b) chunk   64 streams x 3000 rows a call (a scan's smoothed): carried_* is the push on a state whose rings are full, whole_* is
              PhraseDetector.detect (tcr_phrase_scores + tcr_detect_redetect) over the same rows; ratio_* = carried / whole.  A
              push from a fresh state is compared with `detect`, bit for bit (`chunk_equal`)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd.scanning import KeywordScanner, PhraseDetector        # noqa: E402
from scripts.stream_bench import build                                # noqa: E402
from scripts.scan_bench import time_ms                                # noqa: E402

SR, HOP = 16000, 320
PHRASES = [[2, 3], [4, 5, 6], [3, 2], [7, 8, 9]]


def torch_unordered(smoothed, phrases, w):
    """[N, steps, C] -> [N, steps, P + 1]: per word the maximum over the last w steps, per phrase their product, the background last."""
    N, steps, C = smoothed.shape
    cols = sorted({c for q in phrases for c in q})
    x = torch.cat([torch.zeros((N, w - 1, len(cols)), dtype=smoothed.dtype, device=smoothed.device), smoothed[:, :, cols]], dim=1)
    m = x.unfold(1, w, 1).amax(dim=-1)                                 # [N, steps, U]
    out = torch.empty((N, steps, len(phrases) + 1), dtype=smoothed.dtype, device=smoothed.device)
    for q, words in enumerate(phrases):
        r = m[:, :, cols.index(words[0])]
        for c in words[1:]:
            r = r * m[:, :, cols.index(c)]
        out[:, :, q] = r
    out[:, :, -1] = 1.0 - out[:, :, :-1].amax(dim=-1)
    return out


def modes(scanner, windows):
    for w in windows:
        for ordered in (True, False):
            for combine in ("product", "min"):
                ph = PhraseDetector(scanner, PHRASES, window_ms=w * scanner.step_ms, ordered=ordered, combine=combine, detection_threshold=0.05)
                assert ph.window_steps == w
                yield f"w{w}_{'ordered' if ordered else 'unordered'}_{combine}", w, ph


def run_legs(legs, reps, iters=1):
    """Median time per call of every leg over `reps` rounds (the legs alternate within a round), after one warm-up call each."""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            res[k].append(time_ms(fn, iters))
    return {k: round(statistics.median(v), 4) for k, v in res.items()}, {k: [round(x, 4) for x in v] for k, v in res.items()}


def stream_main(args, dev):
    from tcresnet_amd.streaming import StreamingDetector
    fe, net = build(640, HOP, "TCResNet8", 1.0, dev)
    windows = [int(x) for x in args.windows.split(",")]
    g = torch.Generator(device="cuda").manual_seed(0)
    # (a) the server shape
    S = args.streams
    live = StreamingDetector(net, fe, S)
    buf = ((torch.rand((S, live.step_samples), device=dev, generator=g) - 0.5) * 0.5).contiguous()
    legs = {"step_ms": lambda: live.push(buf)}
    out = live.push(buf)
    for tag, w, ph in modes(live, windows):
        sp = ph.streaming(S)
        for _ in range(w + 8):                          # every stream's ring is full from here on
            sp.push(out)
        legs[f"push_{tag}_ms"] = lambda sp=sp: sp.push(out)
    med_a, raw_a = run_legs(legs, args.reps, args.iters)
    ratio_a = {k.replace("push_", "ratio_").replace("_ms", ""): round(v / med_a["step_ms"], 4) for k, v in med_a.items() if k != "step_ms"}
    del live, legs
    # (b) the chunk shape
    N, rows = 64, 3000
    scanner = KeywordScanner(net, fe)
    L = rows * scanner.step_samples
    loud = torch.where(torch.rand((N, L // SR), device=dev, generator=g) < 0.5, 0.01, 0.5).repeat_interleave(SR, dim=1)
    audio = ((torch.rand((N, L), device=dev, generator=g) - 0.5) * 2).mul_(loud).contiguous()
    scan = scanner.scan(audio)
    assert tuple(scan.top.shape) == (N, rows)
    legs, equal = {}, {}
    for tag, w, ph in modes(scanner, windows):
        sp = ph.streaming(N)
        first, whole = sp.push(scan), ph.detect(scan)
        equal[tag] = all(bool(torch.equal(getattr(first, f), getattr(whole, f))) for f in ("probs", "top", "score", "is_new"))
        legs[f"carried_{tag}_ms"] = lambda sp=sp: sp.push(scan)
        legs[f"whole_{tag}_ms"] = lambda ph=ph: ph.detect(scan)
    med_b, raw_b = run_legs(legs, args.reps, 4)
    ratio_b = {k.replace("carried_", "ratio_").replace("_ms", ""): round(v / med_b[k.replace("carried_", "whole_")], 4)
               for k, v in med_b.items() if k.startswith("carried_")}
    row = {"device": torch.cuda.get_device_name(0),
           "workload": f"TCResNet8-1.0, 4020, k = 1, default detector, C = 12, phrases {PHRASES} (8 distinct classes), threshold 0.05",
           "server": {"streams": S, "rows_per_push": 1, "calls_per_timing": args.iters, **med_a, **ratio_a},
           "chunk": {"streams": N, "rows_per_push": rows, "calls_per_timing": 4, **med_b, **ratio_b, "chunk_equal": equal},
           "reps": args.reps, "raw": {**raw_a, **raw_b}}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stream", action="store_true", help="time streaming phrase detection (see above) instead of the whole-scan legs")
    ap.add_argument("--streams", type=int, default=4096, help="--stream: live streams of the server shape")
    ap.add_argument("--iters", type=int, default=50, help="--stream: one-step pushes per timing")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--windows", default="75,150", help="comma-separated windows in steps")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.stream:
        return stream_main(args, dev)
    fe, net = build(640, HOP, "TCResNet8", 1.0, dev)
    scanner = KeywordScanner(net, fe)
    N, L = args.signals, args.seconds * SR
    g = torch.Generator(device="cuda").manual_seed(0)
    loud = torch.where(torch.rand((N, args.seconds), device=dev, generator=g) < 0.5, 0.01, 0.5).repeat_interleave(SR, dim=1)
    audio = ((torch.rand((N, L), device=dev, generator=g) - 0.5) * 2).mul_(loud).contiguous()
    del loud
    out = scanner.scan(audio)
    steps = int(out.top.shape[1])
    legs, equal, fired = {"scan_ms": lambda: scanner.scan(audio)}, {}, {}
    for w in (int(x) for x in args.windows.split(",")):
        for ordered in (True, False):
            for combine in ("product", "min"):
                ph = PhraseDetector(scanner, PHRASES, window_ms=w * scanner.step_ms, ordered=ordered, combine=combine, detection_threshold=0.05)
                assert ph.window_steps == w
                tag = f"w{w}_{'ordered' if ordered else 'unordered'}_{combine}"
                legs[f"scores_{tag}_ms"] = lambda ph=ph: ph.scores(out)
                legs[f"detect_{tag}_ms"] = lambda ph=ph: ph.detect(out)
                fired[tag] = int(ph.detect(out).is_new.sum())
                if not ordered and combine == "product":
                    equal[f"w{w}"] = bool(torch.equal(torch_unordered(out.smoothed, PHRASES, w), ph.scores(out)))
        legs[f"torch_w{w}_ms"] = lambda w=w: torch_unordered(out.smoothed, PHRASES, w)
    for fn in legs.values():                            # warm-up
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(time_ms(fn))
    med = {k: round(statistics.median(v), 4) for k, v in res.items()}
    row = {"device": torch.cuda.get_device_name(0),
           "workload": f"TCResNet8-1.0, 4020, k = 1, default detector; {N} x {args.seconds} s signals ({steps} steps each), C = 12, phrases "
                       f"{PHRASES} (8 distinct classes), threshold 0.05",
           **med, "torch_equal": equal, "detections": fired, "reps": args.reps, "raw": {k: [round(x, 4) for x in v] for k, v in res.items()}}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
