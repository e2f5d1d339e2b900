"""Merge the per-row worst error / bound tests/test_reverb.py prints (pytest -s: lines `REVERB_CONFIGS_ERR {json}`) into
profiles/reverb_configs_err.json.

    pytest tests/test_reverb.py -m "not gpu" -s -n 0 > emu.log;  pytest tests/test_reverb.py -m gpu -s > hip.log
    python scripts/reverb_configs_err.py emu.log hip.log --out profiles/reverb_configs_err.json
"""
import argparse
import json
import os

WHAT = ("worst |error| / bound of tests/test_reverb.py's noise rows, as printed by the tests (pytest -s): synthetic responses off the "
        "fixed-point grid, every output of every clip against the float64 dot product over the same float32 taps and samples, bound "
        "(terms + 1) 2^-24 sum |h x| (an fmaf chain of `terms` products); emu = the emulator build, hip = an MI355X.  The grid, integer, "
        "invariance and identity checks of the same file are bitwise and have no figure.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logs", nargs="+")
    ap.add_argument("--out", default="profiles/reverb_configs_err.json")
    a = ap.parse_args()
    doc = {"what": WHAT, "bound": "err / bound <= 1", "rows": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc.update(json.load(f))
    for path in a.logs:
        with open(path) as f:
            for line in f:
                at = line.find("REVERB_CONFIGS_ERR ")
                if at < 0:
                    continue
                rec = json.loads(line[at + len("REVERB_CONFIGS_ERR "):])
                row = doc["rows"].setdefault(rec["row"], {"taps": rec["taps"], "lengths": rec["lengths"]})
                row[rec["lib"]] = rec["worst_err_over_bound"]
    doc["what"] = WHAT
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, len(doc["rows"]), "rows")


if __name__ == "__main__":
    main()
