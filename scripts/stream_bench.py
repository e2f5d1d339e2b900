"""Per-step time of the streaming detector (StreamingDetector.prepared: stage / shift, k new front-end frames, network, detector in
one C-ABI call) next to the offline call on the same S windows (TCResNet.waveform_call: the whole front-end + network), in one
process, alternating the two.  k = 1; S = 1, 64, 4096; 4020 and 3010; TCResNet8-1.0 and TCResNet14-1.5.  --model DSCNN-L
(4020, 10 MFCCs) or kws_low_latency_conv (4020, 40 MFCCs) times that model alone, the offline call then being the front-end
followed by the engine's forward_infer.

    python scripts/stream_bench.py [--iters 400] [--reps 5] [--out profiles/stream_bench.json]
    python scripts/stream_bench.py --model DSCNN-L [--out profiles/stream_bench_dscnn_l.json]
    python scripts/stream_bench.py --trace_one 4096         # one config, a few steps (for rocprofv3 --kernel-trace --stats)
    python scripts/stream_bench.py --cascade [--out profiles/stream_cascade_bench.json]

--cascade: a streaming cascade (streaming.StreamingCascade) over S = 4096 streams, TCResNet8-1.0 at 30 / 10 ms and k = 2 in front of
DS-CNN-L at 40 / 20 ms and k = 1 (both steps are 320 samples), pad_after = 0.  The enter thresholds are quantiles of the first stage's
keyword peak over a warm-up, so that about 0 %, 1 %, 5 %, 25 % and 100 % of the streams are selected per step; per threshold the
cascade push, the same three calls without the read-back of n_selected (a fixed count: what the read-back costs), and, in the same
run, first.push alone and second.push alone.  The audio is noise at a level of its own per stream and step, cycled from 16 buffers.

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


def cascade_leg(args, dev):
    from tcresnet_amd.streaming import StreamingCascade
    S, n_buf = args.cascade_streams, 16
    fe1, net1 = build(480, 160, "TCResNet8", 1.0, dev)
    _, fe2, net2 = build_model("DSCNN-L", dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    bufs = [((torch.rand((S, 320), device=dev, generator=gen) - 0.5) * torch.rand((S, 1), device=dev, generator=gen) * 1.2).contiguous()
            for _ in range(n_buf)]
    state = {"i": 0}

    def audio():
        state["i"] = (state["i"] + 1) % n_buf
        return bufs[state["i"]]

    first, second = StreamingDetector(net1, fe1, S, frames_per_step=2), StreamingDetector(net2, fe2, S)
    peaks = []
    for i in range(args.warmup + 4 * n_buf):
        x = audio()
        out = first.push(x)
        second.push(x)
        if i >= args.warmup:
            peaks.append(out.probs[:, 2:].max(dim=1).values.cpu().numpy())
    peaks = np.concatenate(peaks)

    def median_of(fn):
        ts = [time_calls(fn, args.iters) for _ in range(args.reps)]
        return round(statistics.median(ts), 2), [round(min(ts), 2), round(max(ts), 2)]

    alone = {}
    for name, det in (("first_push_us", first), ("second_push_us", second)):
        alone[name], alone[name + "_range"] = median_of(lambda: det.push(audio()))
    print(json.dumps(alone), flush=True)
    rows = []
    for target in (0.0, 0.01, 0.05, 0.25, 1.0):
        enter = float("inf") if target == 0.0 else float("-inf") if target == 1.0 else float(np.quantile(peaks, 1.0 - target))
        cas = StreamingCascade(first, second, enter, pad_after_ms=0)
        counts, fixed = [], {"n": 0}

        def push():
            cas.push(audio())
            counts.append(cas.n_selected)

        def push_no_readback():
            x = audio()
            out1 = first.push(x)
            cas.lib.tcr_stream_select(S, 12, out1.probs.data_ptr(), cas._cmask.data_ptr(), cas.enter_threshold, cas.pad_after, None,
                                      cas._since.data_ptr(), cas._ws.data_ptr(), cas._ws.numel() * 4, cas._selected.data_ptr(),
                                      cas._count.data_ptr(), cas.mask.data_ptr(), second.net._stream())
            second.push_selected(x, cas._selected, fixed["n"], out1.logits, out1.probs)

        for _ in range(args.warmup):
            push()
        torch.cuda.synchronize()
        del counts[:]
        t_push, r_push = median_of(push)
        fixed["n"] = int(round(float(np.mean(counts))))
        t_fixed, r_fixed = median_of(push_no_readback)
        row = {"S": S, "first": "TCResNet8-1.0 3010 k=2", "second": "DSCNN-L 4020 k=1", "target_fraction": target, "enter": enter,
               "selected_fraction": round(float(np.mean(counts)) / S, 4), "cascade_push_us": t_push, "cascade_push_us_range": r_push,
               "no_readback_us": t_fixed, "no_readback_us_range": r_fixed,
               "readback_share": round(max(t_push - t_fixed, 0.0) / t_push, 3), **alone}
        row["vs_second_alone"] = round(t_push / alone["second_push_us"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "rows": rows}, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace_one", type=int, default=0, help="S: run a few steps of 4020 TCResNet8-1.0 only (profiler run)")
    ap.add_argument("--model", default="TCResNet8", choices=MODELS)
    ap.add_argument("--cascade", action="store_true", help="the streaming cascade leg (see above)")
    ap.add_argument("--cascade_streams", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.cascade:
        cascade_leg(args, dev)
        return
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
