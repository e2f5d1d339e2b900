#!/bin/bash
# one gpurun call: the pipeline parity tests + bench.py with the driver's flags and with its defaults (headline only)
cd "$(dirname "$0")/.."; OUT=${OUT:-results/quick}; mkdir -p $OUT
timeout 600 python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "pipeline" > $OUT/pytest.log 2>&1; echo "pytest rc=$?"; tail -3 $OUT/pytest.log
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --legs ${LEGS:-none} > $OUT/bench_driver.json 2> $OUT/bench_driver.err; echo "rc=$?"
OUT=$OUT python - <<'PY'
import json, os
for f in (os.path.join(os.environ["OUT"], "bench_driver.json"),):
    o = json.loads(open(f).read().strip().splitlines()[-1])
    print(f, o["ms_per_step"], o["value"], "seq", o["sequential"]["ms_per_step"], "pair", o["pair_roofline"]["frac"], "fe", o["roofline"]["frac"], o.get("bitwise_equal_to_sequential"),
          {k: o[k]["ms_per_step"] for k in o if isinstance(o[k], dict) and "ms_per_step" in o[k] and k != "sequential"})
PY
timeout 300 python bench.py --full --no-cpu-baseline --legs ${LEGS:-none} > $OUT/bench_default.json 2> $OUT/bench_default.err; echo "rc=$?"
OUT=$OUT python - <<'PY'
import json, os
for f in (os.path.join(os.environ["OUT"], "bench_default.json"),):
    o = json.loads(open(f).read().strip().splitlines()[-1])
    print(f, o["ms_per_step"], o["value"], "seq", o["sequential"]["ms_per_step"], "pair", o["pair_roofline"]["frac"], "fe", o["roofline"]["frac"], o.get("bitwise_equal_to_sequential"),
          {k: o[k]["ms_per_step"] for k in o if isinstance(o[k], dict) and "ms_per_step" in o[k] and k != "sequential"})
PY
