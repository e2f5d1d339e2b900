"""Time of reverberating clip pools and recordings on the device (tcr_reverb through reverberation.reverb) next to what a user has
without it.

    python scripts/reverb_bench.py [--reps 5] [--out profiles/reverb_bench.json] [--clips 100000] [--hours 1.0] [--host_clips 4096]

Workloads:
  pool_rt60_0.3 / pool_rt60_0.6   --clips one-second int16 clips against 64 synthetic responses (RT60 0.3 s: 4800 taps, 0.6 s: 9600
                                  taps, one drawn per clip), int16 in, int16 out, the whole tail kept
  hour_f32                        --hours of float32 audio as one recording against one response of RT60 0.3 s, float32 out
Legs (medians over --reps timed calls after a warm-up call, device events around the Python call, so the table uploads are inside;
the legs alternate within a rep):
  reverb      reverberation.reverb (one tcr_reverb launch)
  torch_fft   the same convolution by torch.fft on the device where this torch build has it (rfft of clip and response at the next
              power of two, product, irfft, in batches of 2048 clips; the hour by overlap-add in blocks of 2^17); float32 out, no int16
              rounding.  "torch_fft": null and the reason in "torch_fft_note" where it does not run.
  host_fft    NumPy's FFT convolution on 16 host threads, one clip per task, and the upload of the result -- measured on the first
              --host_clips clips and scaled to the pool by the clip count (stated in the row); the hour is measured whole
MAC/s: the algorithmic multiply-adds over each output's real support (sum over outputs of the chain's terms = n L for a kept tail)
over the reverb leg's time, and that as a fraction of the 157.3 TFLOP/s (78.65 TMAC/s) f32 peak.  torch_fft and host_fft are compared
with reverb's float32 output before anything is timed (max |difference| in the row: they round differently)."""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tcresnet_amd import _lib                                         # noqa: E402
from tcresnet_amd import reverberation as Rv                          # noqa: E402
from scripts.scan_bench import time_ms                                # noqa: E402

SR, CLIP = 16000, 16000
PEAK_MACS = 157.3e12 / 2


def pow2(n):
    return 1 << (int(n) - 1).bit_length()


def torch_fft_pool(data, n_clips, bank, taps, clip_ir, batch=2048):
    """[n_clips, CLIP + max taps - 1] float32 (rows zero behind their own tail)."""
    m = CLIP + int(taps.max()) - 1
    nfft = pow2(m)
    H = torch.fft.rfft(bank, nfft)                      # bank: [R, max taps], zero padded
    out = torch.empty((n_clips, m), dtype=torch.float32, device=data.device)
    idx = torch.from_numpy(clip_ir).to(data.device)
    for a in range(0, n_clips, batch):
        b = min(a + batch, n_clips)
        x = data[a * CLIP:b * CLIP].view(b - a, CLIP).to(torch.float32).mul_(1.0 / 32768.0)
        out[a:b] = torch.fft.irfft(torch.fft.rfft(x, nfft) * H[idx[a:b]], nfft)[:, :m]
    return out


def torch_fft_long(x, h, block=1 << 17):
    """Overlap-add: x float32 [n] with h [L] -> [n] (the tail dropped)."""
    n, L = int(x.shape[0]), int(h.shape[0])
    nfft = pow2(block + L - 1)
    H = torch.fft.rfft(h, nfft)
    rows = -(-n // block)
    xp = torch.zeros(rows * block, dtype=torch.float32, device=x.device)
    xp[:n] = x
    y = torch.fft.irfft(torch.fft.rfft(xp.view(rows, block), nfft) * H, nfft)[:, :block + L - 1]
    out = torch.zeros(rows * block + L - 1, dtype=torch.float32, device=x.device)
    out[:rows * block].view(rows, block).add_(y[:, :block])
    out[block:block + (rows - 1) * block].view(rows - 1, block)[:, :L - 1].add_(y[:-1, block:])
    out[rows * block:].add_(y[-1, block:])
    return out[:n]


def host_fft_pool(pcm, n_clips, hs, clip_ir, dev, threads=16):
    m = CLIP + max(len(h) for h in hs) - 1
    nfft = pow2(m)
    H = [np.fft.rfft(h.astype(np.float64), nfft) for h in hs]
    out = np.zeros((n_clips, m), np.float32)

    def one(j):
        x = pcm[j * CLIP:(j + 1) * CLIP].astype(np.float64) / 32768.0
        out[j] = np.fft.irfft(np.fft.rfft(x, nfft) * H[clip_ir[j]], nfft)[:m]

    with cf.ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(n_clips)))
    return torch.from_numpy(out).to(dev)


def host_fft_long(x, h, dev, threads=16, block=1 << 17):
    n, L = x.size, h.size
    nfft = pow2(block + L - 1)
    H = np.fft.rfft(h.astype(np.float64), nfft)
    rows = -(-n // block)
    parts = [None] * rows

    def one(r):
        parts[r] = np.fft.irfft(np.fft.rfft(x[r * block:(r + 1) * block].astype(np.float64), nfft) * H, nfft)[:block + L - 1]

    with cf.ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(rows)))
    out = np.zeros(rows * block + L - 1)
    for r in range(rows):
        out[r * block:r * block + block + L - 1] += parts[r]
    return torch.from_numpy(out[:n].astype(np.float32)).to(dev)


def timed(legs, reps):
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            res[k].append(time_ms(fn))
    return {k: round(statistics.median(v), 4) for k, v in res.items()}, {k: [round(x, 4) for x in v] for k, v in res.items()}


def have_torch_fft(dev):
    try:
        torch.fft.irfft(torch.fft.rfft(torch.ones(64, device=dev), 64), 64)
        torch.cuda.synchronize()
        return None
    except Exception as e:      # noqa: BLE001
        return f"torch.fft does not run in this torch build: {type(e).__name__}: {str(e)[:200]}"


def pool_row(args, lib, data, rt60, no_fft):
    dev = data.device
    n = args.clips
    irs = Rv.ImpulseResponses.synthetic(64, rt60, SR, seed=1, device=dev, lib=lib)
    hs = irs.numpy()
    taps = irs.lengths
    clip_ir = np.random.default_rng(2).integers(0, 64, n).astype(np.int64)
    off, lens = np.arange(n, dtype=np.int64) * CLIP, np.full(n, CLIP, np.int64)
    out_len = lens + taps[clip_ir] - 1
    macs = float((lens * taps[clip_ir]).sum())
    run = lambda: Rv.reverb(lib, data, off, lens, irs, clip_ir, out_len, floats=False, pcm=True)
    # the float32 output of the first --host_clips clips against both references
    k = min(args.host_clips, n)
    got, _, out_off = Rv.reverb(lib, data, off[:k], lens[:k], irs, clip_ir[:k], out_len[:k], floats=True, pcm=False)
    got = got.cpu().numpy()
    pcm_host = data[:k * CLIP].cpu().numpy()
    want = host_fft_pool(pcm_host, k, hs, clip_ir, dev).cpu().numpy()
    diff_host = max(float(np.abs(got[out_off[j]:out_off[j + 1]] - want[j, :out_len[j]]).max()) for j in range(k))
    row = {"workload": f"{n} clips of {CLIP} int16 samples, 64 synthetic responses of RT60 {rt60} s ({int(taps[0])} taps), int16 out, whole tail",
           "algorithmic_MACs": macs, "max_abs_diff_host_fft": diff_host}
    bank = torch.zeros((64, int(taps.max())), dtype=torch.float32, device=dev)
    for r, h in enumerate(hs):
        bank[r, :len(h)] = torch.from_numpy(h).to(dev)
    legs = {"reverb_ms": run}
    if no_fft is None:
        tf = torch_fft_pool(data, k, bank, taps, clip_ir).cpu().numpy()
        row["max_abs_diff_torch_fft"] = max(float(np.abs(got[out_off[j]:out_off[j + 1]] - tf[j, :out_len[j]]).max()) for j in range(k))
        legs["torch_fft_ms"] = lambda: torch_fft_pool(data, n, bank, taps, clip_ir)
    else:
        row.update(torch_fft_ms=None, torch_fft_note=no_fft)
    med, raw = timed(legs, args.reps)
    host = [time_ms(lambda: host_fft_pool(pcm_host, k, hs, clip_ir, dev)) for _ in range(2)]
    med["host_fft_ms"] = round(min(host) * n / k, 1)
    row.update(med, host_fft_note=f"measured on {k} clips ({[round(x, 1) for x in host]} ms, the smaller taken) and scaled by {n}/{k}", reps=args.reps, raw=raw)
    row.update(reverb_TMACps=round(macs / med["reverb_ms"] / 1e9, 2), reverb_fraction_of_f32_peak=round(macs / (med["reverb_ms"] * 1e-3) / PEAK_MACS, 4),
               speedup_over_host_fft=round(med["host_fft_ms"] / med["reverb_ms"], 1))
    if no_fft is None:
        row["speedup_over_torch_fft"] = round(med["torch_fft_ms"] / med["reverb_ms"], 2)
    return row


def hour_row(args, lib, no_fft):
    dev = torch.device("cuda")
    n = int(args.hours * 3600 * SR)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(n, device=dev, generator=g).mul_(2.0).sub_(1.0)
    irs = Rv.ImpulseResponses.synthetic(1, 0.3, SR, seed=1, device=dev, lib=lib)
    h = irs.numpy()[0]
    macs = float(n) * len(h) - len(h) * (len(h) - 1) / 2.0          # the tail is dropped: outputs 0 .. n - 1
    run = lambda: Rv.reverb(lib, x, [0], [n], irs, [0], [n], floats=True, pcm=False)
    got = run()[0]
    xh = x.cpu().numpy()
    row = {"workload": f"{args.hours} h of float32 audio ({n} samples) as one recording, one response of RT60 0.3 s ({len(h)} taps), float32 out, length kept",
           "algorithmic_MACs": macs, "max_abs_diff_host_fft": float((got - host_fft_long(xh, h, dev)).abs().max())}
    legs = {"reverb_ms": run}
    if no_fft is None:
        hd = torch.from_numpy(h).to(dev)
        row["max_abs_diff_torch_fft"] = float((got - torch_fft_long(x, hd)).abs().max())
        legs["torch_fft_ms"] = lambda: torch_fft_long(x, hd)
    else:
        row.update(torch_fft_ms=None, torch_fft_note=no_fft)
    med, raw = timed(legs, args.reps)
    med["host_fft_ms"] = round(min(time_ms(lambda: host_fft_long(xh, h, dev)) for _ in range(2)), 1)
    row.update(med, reps=args.reps, raw=raw)
    row.update(reverb_TMACps=round(macs / med["reverb_ms"] / 1e9, 2), reverb_fraction_of_f32_peak=round(macs / (med["reverb_ms"] * 1e-3) / PEAK_MACS, 4),
               speedup_over_host_fft=round(med["host_fft_ms"] / med["reverb_ms"], 1))
    if no_fft is None:
        row["speedup_over_torch_fft"] = round(med["torch_fft_ms"] / med["reverb_ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clips", type=int, default=100000)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--host_clips", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reverb_bench.py measures on the GPU: none is visible")
    dev, lib = torch.device("cuda"), _lib.get()
    no_fft = have_torch_fft(dev)
    g = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(-20000, 20000, (args.clips * CLIP,), device=dev, generator=g, dtype=torch.int32).to(torch.int16)
    rows = {}
    for rt60 in (0.3, 0.6):
        rows[f"pool_rt60_{rt60}"] = pool_row(args, lib, data, rt60, no_fft)
        print(json.dumps({f"pool_rt60_{rt60}": {k: v for k, v in rows[f"pool_rt60_{rt60}"].items() if k != "raw"}}), flush=True)
        torch.cuda.empty_cache()
    del data
    torch.cuda.empty_cache()
    rows["hour_f32"] = hour_row(args, lib, no_fft)
    print(json.dumps({"hour_f32": {k: v for k, v in rows["hour_f32"].items() if k != "raw"}}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "tile": _lib.REVERB_TILE, "stage": _lib.REVERB_STAGE, "f32_peak_TFLOPs": 157.3, **rows},
                      fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
