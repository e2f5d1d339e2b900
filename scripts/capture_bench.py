"""What capturing detections' audio on live streams costs (capturing.StreamingRecorder, tcr_capture_*).

    python scripts/capture_bench.py [--streams 4096] [--iters 50] [--reps 5] [--out profiles/capture_bench.json]

Legs (each the median over --reps timings of --iters calls after a warm-up call, device events around the Python calls; the legs
alternate within a round -- scripts/phrase_bench.py's `run_legs`):
 server shape, S streams x one step of 320 samples, one-second clips (n_samples = 16000, lead 0):
  step_ms               the `StreamingDetector.push` the recorder follows;
  rec_push_{0,1,100}_ms `StreamingRecorder.push` with 0 %, 1 % and 100 % of the streams triggering (the outputs are the detector's with
                        is_new / top replaced; capacity = the streams, so every clip is gathered);
  torch_{0,1,100}_ms    the same work in plain torch with the same bits: an index_copy_ of the step into a [S, 16000] ring and, per
                        clip, the ring's two slices and the step copied into the clip's row (the triggering streams known on the host
                        beforehand: torch pays no read-back either);
  copy_ms               a device-to-device copy of the step's S x 320 floats: the bytes the append moves.  append_gbps_whole_push is
                        those bytes (read + written) over the WHOLE no-trigger push (its six launches), a lower bound of the append
                        kernel's own rate; copy_gbps the same bytes over copy_ms.
 chunk shape, 64 streams x 3000 rows:
  many_ms, many_rec_ms  `push_many`, and `push_many` followed by the recorder's push of its output.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd.capturing import StreamingRecorder                  # noqa: E402
from tcresnet_amd.streaming import StreamingDetector, StreamOutput    # noqa: E402
from scripts.phrase_bench import run_legs                             # noqa: E402
from scripts.stream_bench import build                                # noqa: E402

HOP, N_SAMPLES = 320, 16000


class TorchRing:
    """The recorder's work in torch: ring [S, n] with one write position (every stream advances together), clips by slices."""

    def __init__(self, S, step, n, dev):
        self.ring = torch.zeros((S, n), dtype=torch.float32, device=dev)
        self.clips = torch.zeros((S, n), dtype=torch.float32, device=dev)
        self.cols = torch.arange(step, device=dev)
        self.pos, self.step, self.n = 0, step, n

    def push(self, x, streams):
        pos, step, n = self.pos, self.step, self.n
        for i, s in enumerate(streams):                 # the clip: the last n - step samples of the ring, then the step
            tail = n - pos - step
            self.clips[i, :tail] = self.ring[s, pos + step:]
            self.clips[i, tail:n - step] = self.ring[s, :pos]
            self.clips[i, n - step:] = x[s]
        self.ring.index_copy_(1, self.cols + pos, x)
        self.pos = (pos + step) % n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50, help="one-step pushes per timing")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fe, net = build(640, HOP, "TCResNet8", 1.0, dev)
    g = torch.Generator(device="cuda").manual_seed(0)
    S = args.streams
    live = StreamingDetector(net, fe, S)
    step = live.step_samples
    buf = ((torch.rand((S, step), device=dev, generator=g) - 0.5) * 0.5).contiguous()
    out = live.push(buf)
    legs = {"step_ms": lambda: live.push(buf)}
    dst = torch.empty_like(buf)
    legs["copy_ms"] = lambda: dst.copy_(buf)
    rec = StreamingRecorder(live, capacity=S)
    ring = TorchRing(S, step, N_SAMPLES, dev)
    for pct in (0, 1, 100):
        k = S * pct // 100
        new = torch.zeros(S, dtype=torch.int32, device=dev)
        streams = list(range(0, S, S // k))[:k] if k else []
        new[streams] = 1
        fake = StreamOutput(out.logits, out.probs, out.smoothed, torch.full_like(out.top, 5), out.score, new)
        assert len(rec.push(buf, fake)) == k
        legs[f"rec_push_{pct}_ms"] = lambda fake=fake: rec.push(buf, fake)
        legs[f"torch_{pct}_ms"] = lambda streams=streams: ring.push(buf, streams)
    for _ in range(N_SAMPLES // step + 2):              # every ring is full from here on
        rec.push(buf, out)
    med_a, raw_a = run_legs(legs, args.reps, args.iters)
    moved = 2.0 * S * step * 4
    extra = {"append_gbps_whole_push": round(moved / (med_a["rec_push_0_ms"] * 1e6), 1), "copy_gbps": round(moved / (med_a["copy_ms"] * 1e6), 1)}
    del rec, ring, legs
    # the chunk shape
    N, rows = 64, 3000
    chunk = StreamingDetector(net, fe, N)
    crec = StreamingRecorder(chunk, capacity=256)
    audio = ((torch.rand((N, rows * step), device=dev, generator=g) - 0.5) * 0.5).contiguous()

    def many_rec():
        crec.push(audio, chunk.push_many(audio))

    med_b, raw_b = run_legs({"many_ms": lambda: chunk.push_many(audio), "many_rec_ms": many_rec}, args.reps, 2)
    row = {"device": torch.cuda.get_device_name(0),
           "workload": f"TCResNet8-1.0, 4020, k = 1, default detector; recorder: n_samples {N_SAMPLES}, lead 0, float32 clips",
           "server": {"streams": S, "rows_per_push": 1, "calls_per_timing": args.iters, **med_a, **extra},
           "chunk": {"streams": N, "rows_per_push": rows, "calls_per_timing": 2, **med_b, "captured_per_call": len(crec.push(audio, chunk.push_many(audio)))},
           "reps": args.reps, "raw": {**raw_a, **raw_b}}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
