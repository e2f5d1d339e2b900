"""Merge the per-row worst errors tests/test_g2d_configs.py prints (pytest -s: lines `G2D_CONFIGS_ERR {json}`) into
profiles/g2d_configs_err.json, the format of profiles/dscnn_configs_err.json.

    pytest tests/test_g2d_configs.py -m "not gpu" -s -n 0 > emu.log;  pytest tests/test_g2d_configs.py -m gpu -s > hip.log
    python scripts/g2d_configs_err.py emu.log hip.log --out profiles/g2d_configs_err.json
"""
import argparse
import json
import os

BOUNDS = {"logits": 1e-4, "probs": 1e-5, "loss": 1e-4, "grads (relative to max(|ref|, 1e-3))": 3e-4, "stats (x max(1, |ref|))": 1e-5, "adam": 1e-6}
KINDS = ("rows", "unaligned", "shards", "knob")
WHAT = ("worst errors of tests/test_g2d_configs.py per row against the float64 oracle (oracle/net2d_ref.py::graph_forward), as printed by the "
        "tests (pytest -s): emu = the emulator build, hip = an MI355X; unaligned = the C-ABI rows with every pointer one float off; shards = "
        "the whole batch and the sum of two shards; knob = chan_reduce4_kernel behind TCR_TUNE_BWD_MASK = 4; relu_near = ReLU inputs within "
        "1e-5 of zero, where the oracle takes the kernels' side")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logs", nargs="+")
    ap.add_argument("--out", default="profiles/g2d_configs_err.json")
    a = ap.parse_args()
    doc = {"what": WHAT, "bounds": BOUNDS}
    doc.update({k: {} for k in KINDS})
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc.update(json.load(f))
    for path in a.logs:
        with open(path) as f:
            for line in f:
                at = line.find("G2D_CONFIGS_ERR ")
                if at < 0:
                    continue
                rec = json.loads(line[at + len("G2D_CONFIGS_ERR "):])
                doc[rec["kind"]].setdefault(rec["row"], {})[rec["lib"]] = rec["errs"]
    doc["what"], doc["bounds"] = WHAT, BOUNDS
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, {k: len(doc[k]) for k in KINDS})


if __name__ == "__main__":
    main()
