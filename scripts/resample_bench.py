"""Time of the on-device sample-rate conversion (resampling.Resampler.resample: tcr_resample) per audio-hour of output, int16 PCM in,
for 48 kHz / 44.1 kHz / 8 kHz -> 16 kHz, next to (a) the scan of the converted audio (KeywordScanner.scan, TCResNet8-1.0 at 4020,
k = 1), the cost it sits in front of, and (b) the host path it replaces: a float32 torch-CPU polyphase filter with the same table
(one strided conv1d per phase row, --threads CPU threads) plus the upload of its float32 result.

    python scripts/resample_bench.py [--hours 64] [--reps 3] [--out profiles/resample_bench.json]
    python scripts/resample_bench.py --trace_one 44100      # two one-hour conversions after a warm-up (for rocprofv3 --kernel-trace --stats)

64 audio-hours per ratio, converted a call at a time; a call's input is >= 300 MB (one audio-hour at 48 / 44.1 kHz, six at 8 kHz) and
the calls rotate through three distinct input buffers and two output buffers, so no call finds its input in the 256 MiB Infinity
Cache.  Device events around the whole rotation on the stream, after a warm-up rotation; the median over --reps rotations.  Bytes: the
int16 read + the float32 written, against 6.29 TB/s (the measured HBM copy rate of MI355X_MICROARCH.md's table; 8 TB/s is the spec).  The
host path is timed on --host_seconds of audio (default 600) and scaled to the hour: its cost is linear in the length.  The one gate:
the device conversion of an audio-hour must take less time than (b); the script exits with an error otherwise."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd.resampling import Resampler, design_table        # noqa: E402
from tcresnet_amd.scanning import KeywordScanner                   # noqa: E402
from scripts.stream_bench import build                             # noqa: E402

OUT_RATE = 16000
HBM_BYTES_PER_S = 6.29e12


def host_polyphase(pcm: torch.Tensor, L: int, M: int, table: np.ndarray, n_out: int) -> torch.Tensor:
    """float32 [n_out] on the CPU: decode, then for every residue r of j mod L one conv1d of stride M with table row (r M) mod L."""
    P = table.shape[1]
    lead = P // 2 - 1
    x = pcm.to(torch.float32) * (1.0 / 32768.0)
    x = torch.cat([torch.zeros(lead), x, torch.zeros(P + M)])[None, None, :]
    y = torch.empty(n_out, dtype=torch.float32)
    tab = torch.from_numpy(table)
    for r in range(L):
        cnt = len(range(r, n_out, L))
        if cnt == 0:
            continue
        f0 = r * M // L
        y[r::L] = torch.nn.functional.conv1d(x[:, :, f0:f0 + (cnt - 1) * M + P], tab[(r * M) % L][None, None, :], stride=M)[0, 0, :cnt]
    return y


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hours", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host_seconds", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace_one", type=int, default=None, metavar="RATE")
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.set_num_threads(args.threads)
    g = torch.Generator(device="cuda").manual_seed(0)

    def pcm_rows(rows, n):
        return torch.randint(-32768, 32768, (rows, n), device=dev, generator=g, dtype=torch.int32).to(torch.int16)

    if args.trace_one is not None:
        rs = Resampler(args.trace_one, OUT_RATE, 1, device=dev)
        x = pcm_rows(1, 3600 * args.trace_one)
        for _ in range(3):
            rs.resample(x)
        torch.cuda.synchronize()
        print(f"traced one-hour conversions {args.trace_one} Hz -> {OUT_RATE} Hz after a warm-up")
        return

    fe, net = build(640, 320, "TCResNet8", 1.0, dev)
    scanner = KeywordScanner(net, fe, average_window_ms=1000)
    hour16 = ((torch.rand((1, 3600 * OUT_RATE), device=dev, generator=g) - 0.5) * 0.8).contiguous()
    scanner.scan(hour16)
    scans = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        scanner.scan(hour16)
        b.record()
        b.synchronize()
        scans.append(a.elapsed_time(b))
    scan_ms = statistics.median(scans)
    del hour16

    rows_out = {}
    ok = True
    for rate in (48000, 44100, 8000):
        rs = Resampler(rate, OUT_RATE, 1, device=dev)
        L, M, table = design_table(rate, OUT_RATE)
        S = max(1, -(-300_000_000 // (3600 * rate * 2)))           # audio-hours per call: >= 300 MB of int16
        calls = -(-args.hours // S)
        n_in = 3600 * rate
        n_out = rs.out_length(n_in)
        ins = [pcm_rows(S, n_in) for _ in range(3)]
        outs = [torch.empty((S, n_out), dtype=torch.float32, device=dev) for _ in range(2)]

        def rotation():
            for c in range(calls):
                rs.convert(ins[c % 3], 0, 0, n_out, out=outs[c % 2])
        rotation()                                                  # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rotation()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) / (calls * S))
        dev_ms = statistics.median(times)
        bytes_per_hour = n_in * 2 + n_out * 4
        # (b) the host path on a slice, scaled to the hour; its result against the device's on the same samples
        n_host = args.host_seconds * rate
        pcm_host = ins[0][0, :n_host].cpu()
        m_host = rs.out_length(n_host)
        host_polyphase(pcm_host[:rate], L, M, table, rs.out_length(rate))          # warm-up (thread pool, conv plans)
        t0 = time.perf_counter()
        y = host_polyphase(pcm_host, L, M, table, m_host)
        t1 = time.perf_counter()
        yd = y.to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        scale = 3600.0 / args.host_seconds
        diff = float((rs.resample(ins[0][:1, :n_host])[0] - yd).abs().max())
        assert diff < 1e-4, f"{rate}: the host polyphase differs from the device by {diff}"
        host_ms, upload_ms = 1000.0 * (t1 - t0) * scale, 1000.0 * (t2 - t1) * scale
        rows_out[f"{rate}_to_{OUT_RATE}"] = {
            "up": L, "down": M, "taps": int(table.shape[1]), "audio_hours_per_call": S, "calls": calls,
            "device_ms_per_audio_hour": round(dev_ms, 4),
            "device_ms_per_audio_hour_range": [round(min(times), 4), round(max(times), 4)],
            "bytes_per_audio_hour": bytes_per_hour,
            "achieved_bytes_per_s": round(bytes_per_hour / (dev_ms * 1e-3), 1),
            "share_of_hbm_6.29e12": round(bytes_per_hour / (dev_ms * 1e-3) / HBM_BYTES_PER_S, 4),
            "gflop_per_audio_hour": round(2.0 * n_out * table.shape[1] / 1e9, 2),
            "host_polyphase_ms_per_audio_hour": round(host_ms, 1),
            "host_upload_float32_ms_per_audio_hour": round(upload_ms, 1),
            "host_seconds_timed": args.host_seconds, "host_threads": args.threads,
            "host_vs_device_max_abs_diff": diff,
            "device_over_scan": round(dev_ms / scan_ms, 4),
            "device_faster_than_host_path": dev_ms < host_ms + upload_ms,
        }
        ok = ok and dev_ms < host_ms + upload_ms
        print(json.dumps({f"{rate}": rows_out[f"{rate}_to_{OUT_RATE}"]}), flush=True)
        del ins, outs
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "input": "int16 PCM", "hours_per_ratio": args.hours, "reps": args.reps,
           "scan_1h_ms": round(scan_ms, 3), "scan_workload": "TCResNet8-1.0, 4020, k = 1, W = 50 (tcr_scan of one audio-hour)", **rows_out}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not ok:
        sys.exit("the device conversion of an audio-hour took longer than the host path it replaces")


if __name__ == "__main__":
    main()
