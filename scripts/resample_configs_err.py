"""Merge the per-row worst error / bound tests/test_resample_configs.py prints (pytest -s: lines `RESAMPLE_CONFIGS_ERR {json}`) into
profiles/resample_configs_err.json.

    pytest tests/test_resample_configs.py -m "not gpu" -s -n 0 > emu.log;  pytest tests/test_resample_configs.py -m gpu -s > hip.log
    python scripts/resample_configs_err.py emu.log hip.log --out profiles/resample_configs_err.json
"""
import argparse
import json
import os

WHAT = ("worst |error| / bound of tests/test_resample_configs.py's noise check per row of tests/resample_configs.py, as printed by the "
        "tests (pytest -s): every output against the float64 dot product over the same float32 table, bound (P + 1) 2^-24 sum |c x| "
        "(a length-P fmaf chain), whole conversions of int16 and float32 input and a range from a negative out_first; emu = the "
        "emulator build, hip = an MI355X.  The exact, probe and position checks of the same rows are bitwise and have no figure.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logs", nargs="+")
    ap.add_argument("--out", default="profiles/resample_configs_err.json")
    a = ap.parse_args()
    doc = {"what": WHAT, "bound": "err / bound < 1", "rows": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc.update(json.load(f))
    for path in a.logs:
        with open(path) as f:
            for line in f:
                at = line.find("RESAMPLE_CONFIGS_ERR ")
                if at < 0:
                    continue
                rec = json.loads(line[at + len("RESAMPLE_CONFIGS_ERR "):])
                row = doc["rows"].setdefault(rec["row"], {"lmp": rec["lmp"]})
                row[rec["lib"]] = rec["worst_err_over_bound"]
    doc["what"] = WHAT
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, len(doc["rows"]), "rows")


if __name__ == "__main__":
    main()
