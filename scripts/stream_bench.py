"""Per-step time of the streaming detector (StreamingDetector.prepared: stage / shift, k new front-end frames, network, detector in
one C-ABI call) next to the offline call on the same S windows (TCResNet.waveform_call: the whole front-end + network), in one
process, alternating the two.  k = 1; S = 1, 64, 4096; 4020 and 3010; TCResNet8-1.0 and TCResNet14-1.5.  --model DSCNN-L
(4020, 10 MFCCs) or kws_low_latency_conv (4020, 40 MFCCs) times that model alone, the offline call then being the front-end
followed by the engine's forward_infer.

    python scripts/stream_bench.py [--iters 400] [--reps 5] [--out profiles/stream_bench.json]
    python scripts/stream_bench.py --model DSCNN-L [--out profiles/stream_bench_dscnn_l.json]
    python scripts/stream_bench.py --trace_one 4096         # one config, a few steps (for rocprofv3 --kernel-trace --stats)

Each number is the median over --reps windows of --iters back-to-back calls, timed with device events after a warm-up of the
same calls.  Weights are random (timing does not depend on them)."""
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

import tcresnet_amd as T                       # noqa: E402
from tcresnet_amd.streaming import StreamingDetector    # noqa: E402
from oracle import numpy_ref as R              # noqa: E402

CONFIGS = [("4020", 640, 320, "TCResNet8", 1.0), ("4020", 640, 320, "TCResNet14", 1.5),
           ("3010", 480, 160, "TCResNet8", 1.0), ("3010", 480, 160, "TCResNet14", 1.5)]
MODELS = ("TCResNet8", "DSCNN-L", "kws_low_latency_conv")       # --model; TCResNet8 runs CONFIGS (both TC-ResNets)


def build(win, hop, name, width, dev):
    fe = T.Frontend(window_size_samples=win, window_stride_samples=hop, device=dev)
    arch = R.make_tcresnet(name, width)
    p, s = R.init_params(arch, 0)
    R.randomize_bn(arch, p, s)
    net = T.TCResNet(name, R.tcresnet_channels(name, width), 40, fe.n_frames, 12, device=dev)
    sd = dict(p)
    sd.update(s)
    net.load_state_dict(sd)
    return fe, net


def build_model(model, dev):
    """(front-end tag, front-end, net) of --model other than TCResNet8 at 4020, random weights and moving statistics."""
    import numpy as np
    fe = T.Frontend(window_size_samples=640, window_stride_samples=320, num_mfccs=10 if model == "DSCNN-L" else 40, device=dev)
    if model == "DSCNN-L":
        net = T.DSCNN("L", fe.n_frames, fe.n_coef, 12, device=dev)
        net.init_xavier(0)
    else:
        from tcresnet_amd.audio_nets import kws
        net = T.Graph2D("", fe.n_frames, fe.n_coef, 1, device=dev)
        net.finalize(kws.build_model(net, {"spectrogram_length": fe.n_frames, "fingerprint_width": fe.n_coef,
                                           "fingerprint_size": fe.n_frames * fe.n_coef, "label_count": 12, "sample_rate": 16000,
                                           "window_stride_samples": 320}, "low_latency_conv"))
    rng = np.random.RandomState(1)
    for n, ti in net.tensors.items():                   # BN: non-trivial moving statistics
        if ti.arena == 1:
            v = net._view(n)
            v.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, tuple(v.shape)).astype(np.float32)).to(dev))
    return "4020", fe, net


def time_calls(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters        # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace_one", type=int, default=0, help="S: run a few steps of 4020 TCResNet8-1.0 only (profiler run)")
    ap.add_argument("--model", default="TCResNet8", choices=MODELS)
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.trace_one:
        fe, net = build(640, 320, "TCResNet8", 1.0, dev)
        S = args.trace_one
        det = StreamingDetector(net, fe, S)
        call = det.prepared(torch.rand((S, fe.cfg.hop), device=dev) - 0.5)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        print(f"traced 20 steps at S = {S}")
        return
    rows = []
    for tag, win, hop, name, width in (CONFIGS if args.model == "TCResNet8" else [(None, 0, 0, args.model, None)]):
        if args.model == "TCResNet8":
            fe, net = build(win, hop, name, width, dev)
        else:
            tag, fe, net = build_model(args.model, dev)
        for S in (1, 64, 4096):
            det = StreamingDetector(net, fe, S)
            samples = (torch.rand((S, fe.cfg.hop), device=dev) - 0.5).contiguous()
            step = det.prepared(samples)
            wav = (torch.rand((S, fe.n_samples), device=dev) - 0.5).contiguous()
            if args.model == "TCResNet8":
                out = (torch.empty((S, 12), device=dev), torch.empty((S, 12), device=dev))
                offline = net.waveform_call(fe, wav, out)
            else:
                offline = lambda: net.forward_infer(fe(wav))            # noqa: E731
            for _ in range(args.warmup):
                step()
                offline()
            torch.cuda.synchronize()
            ts, to = [], []
            for _ in range(args.reps):                  # alternating windows
                ts.append(time_calls(step, args.iters))
                to.append(time_calls(offline, args.iters))
            row = {"frontend": tag, "net": f"{name}-{width}" if width else name, "S": S, "k": 1, "stream_step_us": round(statistics.median(ts), 2),
                   "stream_step_us_range": [round(min(ts), 2), round(max(ts), 2)], "offline_call_us": round(statistics.median(to), 2),
                   "offline_call_us_range": [round(min(to), 2), round(max(to), 2)]}
            row["ratio"] = round(row["stream_step_us"] / row["offline_call_us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del det, step, offline
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
