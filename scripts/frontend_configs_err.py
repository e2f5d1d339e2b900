"""Worst error per row and kernel arm of the front-end configuration sweep (tests/test_frontend_configs.py) against the float64
oracle, as JSON: the record later front-end work is compared with.

    python scripts/frontend_configs_err.py --lib hip --out profiles/frontend_configs_err.json      (on the MI355X)
    python scripts/frontend_configs_err.py --lib emu --out profiles/frontend_configs_err.json      (emulator build; merged into the file)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", choices=("hip", "emu"), required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import tcresnet_amd as T
    from tests import test_frontend_configs as F
    lib = T._lib.get() if a.lib == "hip" else T._lib.load_from(os.path.join(ROOT, "tests", "emu", "_build", "libtcr_emu.so"), "emu")
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.setdefault("bounds", {"mfcc / log-mel": F.Cm.MFCC_TOL, "deploy float64": F.DEPLOY_TOL, "matrices": F.MATRIX_TOL})
    rows = doc.setdefault("rows", {})
    for row in F.ROWS:
        e = F.check_config_row(lib, row)
        r = rows.setdefault(row[0], {"config": dict(zip(("sample_rate", "clip_ms", "win", "hop", "lower_hz", "upper_hz", "num_mfccs", "method",
                                                        "kernel"), row[1:]))})
        r[a.lib] = {k: float("%.3e" % v) for k, v in e.items()}
        r[a.lib + "_batch"] = F.batch_for(lib, F.build(lib, row)[0].n_frames)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
