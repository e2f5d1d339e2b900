"""Merge the per-row worst errors tests/test_g2d_dw.py prints (pytest -s: lines `G2D_DW_CONFIGS_ERR {json}`) into
profiles/g2d_dw_configs_err.json, the format of profiles/g2d_configs_err.json.

    pytest tests/test_g2d_dw.py -m "not gpu" -s -n 0 > emu.log;  pytest tests/test_g2d_dw.py -m gpu -s > hip.log
    python scripts/g2d_dw_configs_err.py emu.log hip.log --out profiles/g2d_dw_configs_err.json
"""
import argparse
import json
import os

TAG = "G2D_DW_CONFIGS_ERR "
BOUNDS = {"logits": 1e-4, "probs": 1e-5, "loss": 1e-4, "grads (relative to max(|ref|, 1e-3))": 3e-4, "stats (x max(1, |ref|))": 1e-5, "adam": 1e-6}
WHAT = ("worst errors of tests/test_g2d_dw.py per row against the float64 reference (tests/g2d_dw_ref.py::graph_forward), as printed by the "
        "tests (pytest -s): emu = the emulator build, hip = an MI355X; abi_* = the same passes through the C ABI with every pointer one float "
        "behind a 16-byte boundary; relu_near = ReLU inputs within 1e-5 of zero, where the reference takes the kernels' side")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logs", nargs="+")
    ap.add_argument("--out", default="profiles/g2d_dw_configs_err.json")
    a = ap.parse_args()
    doc = {"rows": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc.update(json.load(f))
    for path in a.logs:
        with open(path) as f:
            for line in f:
                at = line.find(TAG)
                if at < 0:
                    continue
                rec = json.loads(line[at + len(TAG):])
                doc["rows"].setdefault(rec["row"], {})[rec["lib"]] = rec["errs"]
    doc["what"], doc["bounds"] = WHAT, BOUNDS
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, len(doc["rows"]), "rows")


if __name__ == "__main__":
    main()
