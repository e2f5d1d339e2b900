"""Enroll keywords the model was not trained on from recorded examples, for scan_audio.py / sweep_audio.py / stream_audio.py --templates:

    python enroll_audio.py --frozen MODEL.npz --out TEMPLATES.npz NAME=FILE.wav[:START_MS-END_MS] [NAME=FILE.wav ...]
                           [--frames_per_step k] [--average_window_ms MS] [--on smoothed|probs] [--max_frames N] [--append]

Every example is one 16-bit PCM WAV file, read as the other tools read theirs (`audio_input.Recordings`: converted to the model's
sample rate on the device when it differs; samples that do not fill a whole step are dropped) and longer than the model's clip.  It is
scanned with MODEL, and the smoothed posteriors (--on probs: the raw ones) of the steps whose windows end in START_MS .. END_MS (default:
the whole file) become one template of keyword NAME (`scanning.KeywordTemplates.enroll`); of more than --max_frames rows (default: the
largest template the library takes) every r-th is kept.  Several examples under one NAME are that keyword's templates.  --append adds to
an existing TEMPLATES.npz.  Give --frames_per_step and --average_window_ms the values the detecting tool will run with: the templates are
rows of that scan.  One line per template on stdout: name,file,frames,first_ms,last_ms."""
from __future__ import annotations

import argparse
import os
import re
import sys
from typing import List, Optional

if __package__ in (None, ""):           # run as a script: import the package through the repository's shim
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tcresnet_amd.audio_input import Recordings
    from tcresnet_amd.deploy import FrozenModel
    from tcresnet_amd.templates import KeywordTemplates
else:
    from .audio_input import Recordings
    from .deploy import FrozenModel
    from .templates import KeywordTemplates

EXAMPLE = re.compile(r"^([^=]+)=(.+?)(?::(\d+(?:\.\d*)?)-(\d+(?:\.\d*)?))?$")


def parse_arguments(arguments: Optional[List[str]] = None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frozen", required=True, help="frozen artifact (.npz) of any model family exported with include_preprocess")
    p.add_argument("--out", required=True, help="the templates file to write (.npz)")
    p.add_argument("examples", nargs="+", metavar="NAME=FILE.wav[:START_MS-END_MS]")
    p.add_argument("--frames_per_step", type=int, default=1, help="new front-end frames per step (k): the detecting tool's")
    p.add_argument("--average_window_ms", type=float, default=1000.0, help="the smoothing window: the detecting tool's")
    p.add_argument("--on", choices=("smoothed", "probs"), default="smoothed", help="the rows kept (the detecting tools read smoothed)")
    p.add_argument("--max_frames", type=int, default=None, help="frames per template at most (default: the library's limit)")
    p.add_argument("--append", action="store_true", help="add to an existing --out file")
    return p.parse_args(arguments)


def main(args) -> int:
    examples = []
    for spec in args.examples:
        m = EXAMPLE.match(spec)
        if m is None:
            raise SystemExit(f"{spec!r} is not NAME=FILE.wav[:START_MS-END_MS]")
        name, path, a, b = m.groups()
        examples.append((name, path, None if a is None else float(a), None if b is None else float(b)))
    scanner = FrozenModel.load(args.frozen).scanner(frames_per_step=args.frames_per_step, average_window_ms=args.average_window_ms)
    templates = KeywordTemplates.load(args.out) if args.append else KeywordTemplates()
    step_ms = scanner.step_ms
    for name, path, a, b in examples:
        rec = Recordings([path], scanner)
        signal, _ = rec.packed()
        t = templates.enroll(scanner, name, signal, a, b, on=args.on, max_frames=args.max_frames)
        print(f"{name},{path},{t.shape[0]},{'' if a is None else format(a, 'g')},{'' if b is None else format(b, 'g')}")
    templates.save(args.out)
    print(f"{args.out}: {len(templates)} templates of {len(templates.names)} keywords at {step_ms:g} ms a step", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
