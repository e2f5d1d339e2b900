"""The cases of tests/test_frontend_trim.py and the writer of its fixture, tests/golden/frontend_trim_digests.json: a sha256 of the float32
feature tensor (and of each of its rows) per case, per library kind ("emu": the host emulator build, "hip": the gfx950 library on an
MI355X -- the two differ in their logarithm).  The fixture is written ONCE, from a build of the commit BEFORE a change that must keep
the front-end's bits, and the test then holds the changed kernels to it:

    python tests/frontend_trim_digests.py --emu                    # the emulator build of this tree (tests/emu/_build)
    python tests/frontend_trim_digests.py --hip                    # the gfx950 library of this tree, on the GPU
    python tests/frontend_trim_digests.py --hip --root <tree>      # ... of another checkout (the parent's), written into this tree's fixture

Each call replaces its own kind's digests in the fixture and keeps the other's."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "frontend_trim_digests.json")
BATCH = 3
SAMPLE_RATE = 16000
N_SAMPLES = 16000
# name -> (window, stride, num_mfccs, method): 49 frames per clip at 640 / 320 (147 frames at batch 3: two 56-frame chunks and a partial
# one at the maximum of 8 rounds, utterance boundaries inside a round of 8 frames), 98 at 480 / 160
CASES = {
    "4020_c40": (640, 320, 40, "mfcc"),
    "4020_c10": (640, 320, 10, "mfcc"),
    "3010_c40": (480, 160, 40, "mfcc"),
    "4020_logmel": (640, 320, 40, "log_mel_spectrogram"),
}


def inputs():
    """One row each: seeded uniform noise, a full-scale 1 kHz sine, one impulse at sample 0 (every other product of the window
    multiply is a zero: the signs of zeros through the FFT)."""
    x = np.zeros((BATCH, N_SAMPLES), np.float32)
    x[0] = np.random.RandomState(20261).uniform(-1.0, 1.0, N_SAMPLES).astype(np.float32)
    x[1] = np.sin(2.0 * np.pi * 1000.0 * np.arange(N_SAMPLES, dtype=np.float64) / SAMPLE_RATE).astype(np.float32)
    x[2, 0] = 1.0
    return x


def digest(t):
    """sha256 of a float32 tensor's bytes (C order)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def case_digests(feat):
    return {"all": digest(feat), "rows": [digest(feat[i]) for i in range(feat.shape[0])]}


def make_frontend(T, lib, name):
    import torch
    win, hop, coef, method = CASES[name]
    dev = torch.device("cuda" if lib.kind == "hip" else "cpu")
    fe = T.Frontend(sample_rate=SAMPLE_RATE, clip_duration_ms=1000, window_size_samples=win, window_stride_samples=hop, num_mfccs=coef,
                    method=method, lib=lib, device=dev)
    assert fe.n_samples == N_SAMPLES
    return fe, dev


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--hip", action="store_true")
    ap.add_argument("--root", default=ROOT, help="checkout whose package and built libraries are measured")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import tcresnet_amd as T
    fx = json.load(open(args.out)) if os.path.exists(args.out) else {}
    kinds = []
    if args.emu:
        kinds.append(("emu", T._lib.load_from(os.path.join(os.path.abspath(args.root), "tests", "emu", "_build", "libtcr_emu.so"), "emu")))
    if args.hip:
        kinds.append(("hip", T._lib.get()))
    for kind, lib in kinds:
        fx[kind] = {}
        for name in CASES:
            fe, dev = make_frontend(T, lib, name)
            fx[kind][name] = case_digests(fe(torch.from_numpy(inputs()).to(dev)))
            print(kind, name, fx[kind][name]["all"])
    with open(args.out, "w") as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
