"""TEST INFRASTRUCTURE ONLY -- generates the committed fixtures under tests/golden/.

    python -m oracle.make_golden

The reference holds no golden vectors and cannot be executed here (TF 1.13.1), so these fixtures are
produced by the float64 NumPy restatement (oracle/numpy_ref.py) after cross-checking it against the
independent PyTorch implementation (oracle/torch_ref.py); "parity unpinned" applies (oracle/__init__.py).
Every fixture stores inputs AND expected outputs, so tests never need /root/reference.
"""
from __future__ import annotations

import os

import numpy as np

from . import numpy_ref as R
from . import torch_ref as TR

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def dropout_uniform(seed: int, index: np.ndarray) -> np.ndarray:
    """Bit-exact NumPy mirror of tcr::uniform01 (tc-resnet_amd/csrc/tcr_common.h)."""
    def mix32(x):
        x = x.astype(np.uint32)
        x ^= x >> np.uint32(16)
        x = (x.astype(np.uint64) * np.uint64(0x7feb352d) & np.uint64(0xffffffff)).astype(np.uint32)
        x ^= x >> np.uint32(15)
        x = (x.astype(np.uint64) * np.uint64(0x846ca68b) & np.uint64(0xffffffff)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        return x
    index = np.asarray(index, np.uint64)
    lo = (index & np.uint64(0xffffffff)).astype(np.uint32)
    hi = (index >> np.uint64(32)).astype(np.uint32)
    s0 = np.array([seed & 0xffffffff], np.uint32)
    s1 = np.array([(seed >> 32) & 0xffffffff], np.uint32)
    s1c = ((s1.astype(np.uint64) + np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)).astype(np.uint32)
    h = mix32(lo ^ mix32(hi ^ mix32(s0 ^ mix32(s1c))))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def dropout_mask(seed: int, sample_offset: int, batch: int, channels: int, keep_prob: float) -> np.ndarray:
    idx = (sample_offset + np.arange(batch, dtype=np.uint64)[:, None]) * np.uint64(channels) + np.arange(channels, dtype=np.uint64)[None, :]
    return (dropout_uniform(seed, idx) < np.float32(keep_prob)).astype(np.float64)


FRONTENDS = {"3010": R.FRONTEND_3010, "4020": R.FRONTEND_4020}


def make_frontend():
    for tag, cfg in FRONTENDS.items():
        wav = R.synth_waveforms(2, seed=1234)
        # edge rows: digital silence and a full-scale square-ish signal
        wav = np.concatenate([wav, np.zeros((1, 16000), np.float32), np.sign(np.sin(np.arange(16000) * 0.05)).astype(np.float32)[None] * 0.99])
        m64 = R.mfcc(wav, cfg)
        mt = TR.mfcc(__import__("torch").tensor(wav, dtype=__import__("torch").float64), cfg).numpy()
        assert np.abs(m64 - mt).max() < 1e-9
        lm = R.log_mel_spectrogram(wav, cfg, magnitude_squared=False)
        np.savez_compressed(os.path.join(OUT, f"frontend_{tag}.npz"), wav=wav, mfcc=m64, log_mel_magnitude=lm,
                            win=cfg.win, hop=cfg.hop)


def edge_waveforms(n_samples: int = 16000) -> np.ndarray:
    """The reference's low-amplitude workload and two spectral extremes, where log(mel + 1e-6) amplifies error most:
    rows 0-2: a SILENT clip (label `_silence_`: empty file -> zeros, datasets/audio_data_wrapper.py:164-174) mixed with a
              background recording at volume 0.01 / 0.05 / 0.1 (augmentation_factory.py:92-97: clip(bg * volume + fg); the
              reference draws the volume from U(0, 0.1), :30-101) -- the "recording" is int16 noise like a decoded WAV;
    row 3:    white noise at amplitude 1e-4 (mel energies around the 1e-6 log offset);
    row 4:    a pure full-scale 1 kHz sine (one spectral line, 90 dB above its neighbours);
    row 5:    a 30 Hz sine at 0.5 (energy only BELOW the first mel filter: every band near the log offset)."""
    from . import augment_ref as A
    rng = np.random.RandomState(77)
    bg = rng.randint(-32768, 32768, 3 * n_samples).astype(np.int16)
    rows = []
    for i, vol in enumerate((0.01, 0.05, 0.1)):
        crop = bg[i * n_samples:(i + 1) * n_samples].astype(np.float32) * np.float32(1.0 / 32768.0)
        rows.append(A.mix_background(np.zeros(n_samples, np.float32), crop, vol))
    rows.append((rng.uniform(-1.0, 1.0, n_samples) * 1e-4).astype(np.float32))
    t = np.arange(n_samples, dtype=np.float64) / 16000.0
    rows.append(np.sin(2.0 * np.pi * 1000.0 * t).astype(np.float32))
    rows.append((0.5 * np.sin(2.0 * np.pi * 30.0 * t)).astype(np.float32))
    return np.stack(rows)


def make_frontend_edges():
    import torch
    wav = edge_waveforms()
    for tag, cfg in FRONTENDS.items():
        m64 = R.mfcc(wav, cfg)
        mt = TR.mfcc(torch.tensor(wav, dtype=torch.float64), cfg).numpy()
        assert np.abs(m64 - mt).max() < 1e-9
        np.savez_compressed(os.path.join(OUT, f"frontend_edge_{tag}.npz"), wav=wav, mfcc=m64, mfcc_deploy=R.mfcc_deploy(wav, cfg),
                            win=cfg.win, hop=cfg.hop)


def _keep(name: str, full: bool, key: str) -> bool:
    """Large nets store only the small tensors + a few weight tensors (weights are regenerated from the seeds)."""
    if full:
        return True
    return ("BatchNorm" in key) or key.endswith("conv0/weights") or key.endswith("fc/weights") or ("block5/" in key) or ("block2/down" in key)


def make_net(name: str, width: float, tag: str, batch: int = 4, seed: int = 0, full: bool = True):
    cfg = FRONTENDS[tag]
    arch = R.make_tcresnet(name, width)
    p, s = R.init_params(arch, seed)
    R.randomize_bn(arch, p, s, seed + 1)
    wav = R.synth_waveforms(batch, seed=4321)
    labels = R.synth_labels(batch).astype(np.float64)
    x = R.mfcc(wav, cfg)
    ev = R.forward(arch, p, s, x, False)
    # cross-check eval against torch
    import torch
    tev = TR.forward(arch, {k: torch.tensor(v) for k, v in p.items()}, {k: torch.tensor(v) for k, v in s.items()}, torch.tensor(x), False)
    assert np.abs(tev["logits"].numpy() - ev["logits"]).max() < 1e-10
    out = {"wav": wav, "labels": labels, "mfcc": x, "eval_logits": ev["logits"], "eval_probs": ev["probs"], "eval_ranges": ev["ranges"],
           "width": width, "win": cfg.win, "hop": cfg.hop}
    out.update(init_seed=seed, bn_seed=seed + 1, full=full)
    if full:        # otherwise: R.init_params(arch, init_seed) + R.randomize_bn(arch, p, s, bn_seed)
        for k, v in p.items():
            out["param:" + k] = v
        for k, v in s.items():
            out["stat:" + k] = v
    # training: 3 momentum steps, keep_prob 0.5 with the kernel's own counter-based mask
    keep, wd, lr, mu, dseed, off = 0.5, 0.001, 0.1, 0.9, 99, 5
    pp, ss = dict(p), dict(s)
    mm = {k: np.zeros_like(v) for k, v in p.items()}
    for step in range(3):
        mask = dropout_mask(dseed + step, off, batch, arch.fc.cin, keep)
        if step == 0:
            tg, ttot, tmodel, tns = TR.grads(arch, pp, ss, x, labels, wd, keep, mask)
        pp, ss, mm, info = R.train_step(arch, pp, ss, mm, x, labels, lr, wd, mu, keep, mask)
        if step == 0:
            assert max(np.abs(info["grads"][k] - tg[k]).max() for k in tg) < 1e-9
            out["train_logits"] = info["logits"]
            out["train_model_loss"] = info["model_loss"]
            out["train_l2_loss"] = info["l2_loss"]
            for k, v in info["grads"].items():
                if _keep(name, full, k):
                    out["grad:" + k] = v            # includes the L2 term wd * w
            for k, v in ss.items():
                out["stat1:" + k] = v
            for k, v in pp.items():
                if _keep(name, full, k) and full:
                    out["param1:" + k] = v
    for k, v in pp.items():
        if _keep(name, full, k):
            out["param3:" + k] = v
    for k, v in ss.items():
        out["stat3:" + k] = v
    out.update(train_keep_prob=keep, train_weight_decay=wd, train_lr=lr, train_momentum=mu, train_seed=dseed, train_sample_offset=off)
    np.savez_compressed(os.path.join(OUT, f"{name.lower()}_{width}_{tag}.npz"), **out)


def make_dscnn():
    """DS-CNN S/M/L eval logits; weights are regenerated from the seed (dscnn_ref.init_params(net_def(size), seed=0))."""
    import dataclasses
    from . import dscnn_ref as D
    cfg = dataclasses.replace(R.FRONTEND_4020, num_mfccs=10)
    wav = R.synth_waveforms(3, seed=2468)
    x = R.mfcc(wav, cfg)
    out = {"wav": wav, "mfcc": x, "win": cfg.win, "hop": cfg.hop, "init_seed": 0}
    for size in ("S", "M", "L"):
        p, s = D.init_params(D.net_def(size), seed=0)
        r = D.forward(D.net_def(size), p, s, x, False)
        out[f"logits_{size}"] = r["logits"]
        out[f"probs_{size}"] = r["probs"]
        out[f"n_params_{size}"] = sum(v.size for v in p.values())
    np.savez_compressed(os.path.join(OUT, "dscnn_4020.npz"), **out)
    # training: 3 Adam steps (lr 5e-4, the reference's DS-CNN schedule).  S is stored in full; L keeps the small tensors.
    # The waveform seed is the one (of 40 candidates) whose BN pre-activations stay farthest from the ReLU kink in the first
    # step: an f32 implementation cannot be expected to land on the same side of an input within round-off (~1e-6) of 0,
    # and one flipped mask changes that channel's gradient by O(1 / elements per channel).
    labels = R.synth_labels(3).astype(np.float64)
    tr = {"labels": labels, "train_lr": 5e-4, "init_seed": 0}
    for size in ("S", "L"):
        blocks = D.net_def(size)
        margin, wav_seed = -1.0, None
        for cand in range(2468, 2508):
            p, s = D.init_params(blocks, seed=0)
            f = D.forward(blocks, p, s, R.mfcc(R.synth_waveforms(3, seed=cand), cfg), True)
            mg = min(np.abs(c["xhat"] + p[k + "/beta"]).min() for k, c in f["cache"].items() if isinstance(c, dict))
            if mg > margin:
                margin, wav_seed = mg, cand
        assert margin > 5e-6, margin
        x = R.mfcc(R.synth_waveforms(3, seed=wav_seed), cfg)
        tr[f"{size}:wav_seed"] = wav_seed
        tr[f"{size}:relu_margin"] = margin
        m = {k: np.zeros_like(v) for k, v in p.items()}
        v = {k: np.zeros_like(w) for k, w in p.items()}
        keep = (lambda k: True) if size == "S" else (lambda k: ("pointwise_conv/weights" not in k) or k.startswith("DSCNN/conv_ds_3/"))
        keep_w = (lambda k: True) if size == "S" else (lambda k: "pointwise_conv/weights" not in k)
        for step in range(3):
            p, s, m, v, info = D.train_step(blocks, p, s, m, v, x, labels, 5e-4, step + 1)
            if step == 0:
                tr[f"{size}:train_logits"] = info["logits"]
                tr[f"{size}:train_model_loss"] = info["model_loss"]
                for k, g in info["grads"].items():
                    if keep(k):
                        tr[f"{size}:grad:" + k] = g
                for k, w in s.items():
                    tr[f"{size}:stat1:" + k] = w
                for k, w in p.items():
                    if keep_w(k):
                        tr[f"{size}:param1:" + k] = w
        for k, w in p.items():
            if keep_w(k):
                tr[f"{size}:param3:" + k] = w
        for k, w in s.items():
            tr[f"{size}:stat3:" + k] = w
    np.savez_compressed(os.path.join(OUT, "dscnn_train_4020.npz"), **tr)


def main():
    os.makedirs(OUT, exist_ok=True)
    import sys
    if "--edges-only" in sys.argv:          # (adds frontend_edge_*.npz without rewriting the other fixtures)
        make_frontend_edges()
        return
    if "--tcresnet14-3010-only" in sys.argv:        # (round 6: adds the configs[3] fixture at the reference's own setting without rewriting the others)
        make_net("TCResNet14", 1.5, "3010", batch=2, full=False)
        return
    make_dscnn()
    make_frontend()
    make_frontend_edges()
    make_net("TCResNet8", 1.0, "4020")
    make_net("TCResNet8", 1.0, "3010", batch=3)
    make_net("TCResNet14", 1.5, "4020", batch=3, full=False)
    # BASELINE configs[3] at the reference's own front-end setting: its only TCResNet14-1.5 script is 30 / 10 ms -> 98 frames
    # (scripts/commands/TCResNet14Model-1.5_mfcc_40_3010_0.001_mom_l1.sh:3): the asymmetric SAME pads (3, 4) of the stride-2 convs at T = 98
    make_net("TCResNet14", 1.5, "3010", batch=2, full=False)
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)) // 1024, "KiB")


if __name__ == "__main__":
    main()
