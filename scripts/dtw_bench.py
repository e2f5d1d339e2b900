"""Time of template matching (TemplateDetector.scores / .detect: tcr_dtw_scores and tcr_detect_redetect over its posteriors;
StreamingTemplateDetector.push: tcr_dtw_stream_push), next to the stages it follows.  TCResNet8-1.0 at 4020, k = 1, the default
detector, scan_bench.py's audio (noise in 1 s segments of random loudness), C = 12; 4 and 16 templates of 50 and of 100 frames cut from
the scan itself, every template a keyword of its own (the parallelism of a call is signals x keywords).

    python scripts/dtw_bench.py [--reps 3] [--out profiles/dtw_bench.json] [--seconds 3600] [--streams 4096]

Shapes (each leg the median over --reps timed calls after a warm-up call, device events around the Python call; the legs alternate
within a rep), per template set q{Q}_l{L}:
  whole   64 x 1-hour signals: scores_* is TemplateDetector.scores over the scan's smoothed, detect_* TemplateDetector.detect, next to
          scan_ms, the scan that produces their input, and phrase_scores_w75_ms, PhraseDetector.scores at a window of 75 steps.
  server  S = 4096 live streams, one step a push: step_ms is StreamingDetector.push (front-end, network, detector) and push_* the
          template push of that step's output, the time per call over --iters calls in a row; ratio_* = push / step.
  chunk   64 streams x 3000 rows in one call: carried_* is the push, whole_* TemplateDetector.detect over the same rows; a push from
          a fresh state is compared with `detect`, bit for bit (`chunk_equal`).
The numbers are records, not gates."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd.scanning import KeywordScanner, KeywordTemplates, PhraseDetector, TemplateDetector     # noqa: E402
from scripts.phrase_bench import PHRASES, run_legs                     # noqa: E402
from scripts.stream_bench import build                                # noqa: E402

SR, HOP = 16000, 320
SETS = [(4, 50), (4, 100), (16, 50), (16, 100)]


def noise(N, seconds, dev, g):
    loud = torch.where(torch.rand((N, seconds), device=dev, generator=g) < 0.5, 0.01, 0.5).repeat_interleave(SR, dim=1)
    return ((torch.rand((N, seconds * SR), device=dev, generator=g) - 0.5) * 2).mul_(loud).contiguous()


def detectors(scanner, smoothed):
    """A TemplateDetector per template set: template q is rows 100 + 37 q .. of signal q mod N of the scan."""
    N = int(smoothed.shape[0])
    for Q, L in SETS:
        kt = KeywordTemplates()
        for q in range(Q):
            kt.add(f"k{q}", smoothed[q % N, 100 + 37 * q:100 + 37 * q + L].cpu().numpy())
        yield f"q{Q}_l{L}", TemplateDetector(scanner, kt, detection_threshold=0.9)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20, help="one-step pushes per timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    from tcresnet_amd.streaming import StreamingDetector
    fe, net = build(640, HOP, "TCResNet8", 1.0, dev)
    g = torch.Generator(device="cuda").manual_seed(0)
    scanner = KeywordScanner(net, fe)
    # whole: the scan of N signals of an hour
    audio = noise(args.signals, args.seconds, dev, g)
    out = scanner.scan(audio)
    steps = int(out.top.shape[1])
    ph = PhraseDetector(scanner, PHRASES, window_ms=75 * scanner.step_ms, detection_threshold=0.05)
    legs, fired = {"scan_ms": lambda: scanner.scan(audio), "phrase_scores_w75_ms": lambda: ph.scores(out)}, {}
    for tag, td in detectors(scanner, out.smoothed):
        legs[f"scores_{tag}_ms"] = lambda td=td: td.scores(out)
        legs[f"detect_{tag}_ms"] = lambda td=td: td.detect(out)
        fired[tag] = int(td.detect(out).is_new.sum())
    whole, raw_w = run_legs(legs, args.reps)
    chunk_src = out.smoothed[:, :3000].contiguous()
    del audio, out, legs
    # server: one step of S live streams
    S = args.streams
    live = StreamingDetector(net, fe, S)
    buf = ((torch.rand((S, live.step_samples), device=dev, generator=g) - 0.5) * 0.5).contiguous()
    step_out = live.push(buf)
    legs = {"step_ms": lambda: live.push(buf)}
    for tag, td in detectors(live, chunk_src):
        sp = td.streaming(S)
        for _ in range(8):
            sp.push(step_out)
        legs[f"push_{tag}_ms"] = lambda sp=sp: sp.push(step_out)
    server, raw_s = run_legs(legs, args.reps, args.iters)
    ratio_s = {k.replace("push_", "ratio_").replace("_ms", ""): round(v / server["step_ms"], 4) for k, v in server.items() if k != "step_ms"}
    del live, legs
    # chunk: 64 streams x 3000 rows a call
    from tcresnet_amd.scanning import ScanOutput
    rows = ScanOutput(None, chunk_src, chunk_src, None, None, None)
    legs, equal = {}, {}
    for tag, td in detectors(scanner, chunk_src):
        sp = td.streaming(int(chunk_src.shape[0]))
        first, ref = sp.push(rows), td.detect(rows)
        equal[tag] = all(bool(torch.equal(getattr(first, f), getattr(ref, f))) for f in ("probs", "top", "score", "is_new"))
        legs[f"carried_{tag}_ms"] = lambda sp=sp: sp.push(rows)
        legs[f"whole_{tag}_ms"] = lambda td=td: td.detect(rows)
    chunk, raw_c = run_legs(legs, args.reps, 4)
    row = {"device": torch.cuda.get_device_name(0),
           "workload": "TCResNet8-1.0, 4020, k = 1, default detector, C = 12; Q templates of L frames cut from the scan, one keyword each, "
                       "scale 0.5 / L, max_stretch 3, threshold 0.9",
           "whole": {"signals": args.signals, "steps": steps, **whole, "detections": fired},
           "server": {"streams": S, "rows_per_push": 1, "calls_per_timing": args.iters, **server, **ratio_s},
           "chunk": {"streams": int(chunk_src.shape[0]), "rows_per_push": 3000, "calls_per_timing": 4, **chunk, "chunk_equal": equal},
           "reps": args.reps, "raw": {**raw_w, **raw_s, **raw_c}}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
