"""Time of hard-example mining (KeywordScanner.mine and its four calls: tcr_mine_detections / _peaks / _select / _gather) over the scan of
64 x 1-hour and 64 x 1-minute signals, next to the scan itself and to what there was before for the same result.  TCResNet8-1.0 at
4020, k = 1, the default detector, scan_bench.py's audio (noise in 1 s segments of random loudness), one labelled event per 10 s.

    python scripts/mine_bench.py [--reps 5] [--out profiles/mine_bench.json] [--seconds 3600,60]

Legs per shape (each the median over --reps timed calls after a warm-up call, device events around the Python call, so the host's
table copies and the read-back of the counts are included; the legs alternate within a rep):
  detections       mine_detections over the scan's top / score / is_new and the events
  detections_old   sweep(return_fired=True) at the scanner's threshold, nonzero, the copy to the host and the rule there in NumPy
                   (searchsorted over the events, first hit per event by np.unique)
  peaks            mine_peaks over the scan's probs (classes 2 on, floor 0.2, radius = the suppression steps)
  select_K         select_top over the peaks' values;  select_old_K: the values copied to the host, torch.topk there, the indices sorted
  gather_K         gather_clips of the K picked peaks' clips (float32);  gather_old_K: one torch slice per clip into a zeroed batch
  mine_K           the whole KeywordScanner.mine(source="detections", kinds=false_accept, pcm=True);  mine_peaks_K: source="peaks"
  scan             the scan the mining reads
and one roofline figure: gather_10000's bytes (read + written: 2 x K x 16000 x 4) per second next to a torch device-to-device copy of
a tensor of K x 16000 floats (the same bytes read and written) timed the same way in the same process."""
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

from tcresnet_amd.scanning import (KeywordScanner, RaggedScanOutput, detection_sweep, gather_clips, mine_detections, mine_peaks,      # noqa: E402
                                   select_top)
from scripts.stream_bench import build                                # noqa: E402
from scripts.scan_bench import time_ms                                # noqa: E402

SR, HOP, CLIP = 16000, 320, 16000


def classify_on_host(fired, top, offsets, ev):
    """The parent commit's route: the fired steps (device) -> kinds on the host, vectorised."""
    steps = fired.nonzero().reshape(-1).cpu().numpy()
    lab = top.cpu().numpy()[steps]
    sig = np.searchsorted(offsets, steps, side="right") - 1
    first, last, label, ev_off = ev
    i = steps - offsets[sig]
    key = sig.astype(np.int64) << 40 | i                                   # events are sorted within a signal: one global sorted key
    ev_key = np.repeat(np.arange(len(ev_off) - 1, dtype=np.int64), np.diff(ev_off)) << 40 | first
    e = np.searchsorted(ev_key, key, side="right") - 1
    covered = (e >= 0) & (np.repeat(np.arange(len(ev_off) - 1), np.diff(ev_off))[np.maximum(e, 0)] == sig) & (last[np.maximum(e, 0)] >= i)
    match = covered & (label[np.maximum(e, 0)] == lab)
    kind = np.zeros(steps.size, np.uint8)
    _, firsts = np.unique(e[match], return_index=True)
    idx = np.flatnonzero(match)
    kind[idx] = 2
    kind[idx[firsts]] = 1
    return steps, kind


def slices(packed, sample_off, sig, first, n):
    out = torch.zeros((len(sig), n), dtype=torch.float32, device=packed.device)
    for j, (s, f) in enumerate(zip(sig.tolist(), first.tolist())):
        a, b = int(sample_off[s]), int(sample_off[s + 1])
        lo, hi = max(f, 0), min(f + n, b - a)
        if hi > lo:
            out[j, lo - f:hi - f] = packed[a + lo:a + hi]
    return out


def shape_row(args, fe, net, seconds, N):
    dev = torch.device("cuda")
    scanner = KeywordScanner(net, fe)
    L = seconds * SR
    g = torch.Generator(device="cuda").manual_seed(0)
    loud = torch.where(torch.rand((N, seconds), device=dev, generator=g) < 0.5, 0.01, 0.5).repeat_interleave(SR, dim=1)
    audio = ((torch.rand((N, L), device=dev, generator=g) - 0.5) * 2).mul_(loud).contiguous()
    del loud
    dense = scanner.scan(audio)
    steps = int(dense.top.shape[1])
    offsets = np.arange(N + 1, dtype=np.int64) * steps
    out = RaggedScanOutput(*(t.reshape(N * steps, *t.shape[2:]) for t in dense), offsets)
    packed, sample_off = audio.reshape(-1), offsets * HOP
    rng = np.random.RandomState(0)
    starts = np.arange(0, steps - 50, 500, dtype=np.int64)
    ev_steps = [np.stack([starts, starts + 49, rng.randint(12, size=len(starts))], axis=1) for _ in range(N)]
    ev_ms = [[(20.0 * (a + 1), 20.0 * (b + 1), int(c)) for a, b, c in e] for e in ev_steps]
    ev_host = (np.concatenate([e[:, 0] for e in ev_steps]), np.concatenate([e[:, 1] for e in ev_steps]),
               np.concatenate([e[:, 2] for e in ev_steps]), np.arange(N + 1, dtype=np.int64) * len(starts))
    thr, supp, radius = scanner.det.threshold, scanner.suppression_steps, max(1, scanner.suppression_steps)
    classes = list(range(2, 12))

    def detections_old():
        r = detection_sweep(out.top, out.score, [thr], supp, 12, events=ev_steps, return_fired=True, step_offsets=offsets)
        return classify_on_host(r.fired[0], out.top, offsets, ev_host)

    md = mine_detections(out.top, out.score, out.is_new, offsets, 12, ev_steps)
    old_steps, old_kind = detections_old()
    assert md.step.cpu().numpy().tolist() == old_steps.tolist() and md.kind.cpu().numpy().tolist() == old_kind.tolist()
    mp = mine_peaks(out.probs, offsets, 0.2, radius, classes)
    n_peaks = mp.count
    legs = {"detections_ms": lambda: mine_detections(out.top, out.score, out.is_new, offsets, 12, ev_steps),
            "detections_old_ms": detections_old,
            "peaks_ms": lambda: mine_peaks(out.probs, offsets, 0.2, radius, classes, capacity=n_peaks),
            "scan_ms": lambda: scanner.scan(audio)}
    copies = {}
    for K in args.k:
        picked = select_top(mp.value, K)
        host = mp.value.cpu().numpy()
        want = np.sort(np.lexsort((np.arange(host.size), -host))[:K])
        assert picked.cpu().numpy().tolist() == want.tolist()
        n = int(picked.numel())
        sig = (mp.step[picked] // steps).to(torch.int32)
        first = (mp.step[picked] % steps + 1) * HOP - CLIP
        clips, _ = gather_clips(packed, sample_off, sig, first, CLIP)
        sig_h, first_h = sig.cpu().numpy(), first.cpu().numpy()
        assert torch.equal(clips, slices(packed, sample_off, sig_h, first_h, CLIP))
        src, dst = torch.empty((n, CLIP), dtype=torch.float32, device=dev).normal_(), torch.empty((n, CLIP), dtype=torch.float32, device=dev)
        copies[K] = n
        legs.update({
            f"select_{K}_ms": lambda K=K: select_top(mp.value, K),
            f"select_old_{K}_ms": lambda K=K: torch.sort(torch.topk(mp.value.cpu(), min(K, n_peaks)).indices).values.to(dev),
            f"gather_{K}_ms": lambda sig=sig, first=first: gather_clips(packed, sample_off, sig, first, CLIP),
            f"gather_old_{K}_ms": lambda sig_h=sig_h, first_h=first_h: slices(packed, sample_off, sig_h, first_h, CLIP),
            f"copy_{K}_ms": lambda src=src, dst=dst: dst.copy_(src),
            f"mine_{K}_ms": lambda K=K: scanner.mine(out, (packed, [L] * N), ev_ms, k=K, pcm=True),
            f"mine_peaks_{K}_ms": lambda K=K: scanner.mine(out, (packed, [L] * N), ev_ms, k=K, source="peaks", floor=0.2, pcm=True),
        })
    for fn in legs.values():                            # warm-up
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            res[k].append(time_ms(fn))
    med = {k: round(statistics.median(v), 4) for k, v in res.items()}
    row = {"workload": f"TCResNet8-1.0, 4020, k = 1, default detector; {N} x {seconds} s signals ({steps} steps each), "
                       f"{sum(len(e) for e in ev_steps)} events, {int(md.step.numel())} detections, {n_peaks} peaks (floor 0.2, radius {radius})",
           **med, "clips": copies, "reps": args.reps, "raw": {k: [round(x, 4) for x in v] for k, v in res.items()}}
    for K, n in copies.items():
        nbytes = 2.0 * n * CLIP * 4
        row[f"gather_{K}_GBps"] = round(nbytes / med[f"gather_{K}_ms"] / 1e6, 1)
        row[f"copy_{K}_GBps"] = round(nbytes / med[f"copy_{K}_ms"] / 1e6, 1)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--seconds", default="3600,60", help="comma-separated signal lengths, one shape each")
    ap.add_argument("--k", default="1000,10000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.k = [int(x) for x in args.k.split(",")]
    fe, net = build(640, HOP, "TCResNet8", 1.0, torch.device("cuda"))
    rows = {}
    for seconds in (int(x) for x in args.seconds.split(",")):
        rows[f"{args.signals}x{seconds}s"] = shape_row(args, fe, net, seconds, args.signals)
        print(json.dumps({f"{args.signals}x{seconds}s": rows[f"{args.signals}x{seconds}s"]}), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), **rows}, fh, indent=1)


if __name__ == "__main__":
    main()
