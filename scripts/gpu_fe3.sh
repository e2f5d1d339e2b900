#!/bin/bash
# one gpurun call: front-end parity tests, the three-waves vs two-waves A/B (with sweeps), a quick headline bench
cd "$(dirname "$0")/.."; OUT=${OUT:-results/fe3}; mkdir -p $OUT
timeout 900 python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "frontend" > $OUT/pytest.log 2>&1; echo "pytest rc=$?"; tail -5 $OUT/pytest.log
timeout 600 python scripts/ab_fe_kernel.py --sweep > $OUT/ab.log 2>&1; echo "ab rc=$?"; cat $OUT/ab.log
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --legs ${LEGS:-train} > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"
OUT=$OUT python - <<'PY'
import json, os
o = json.loads(open(os.path.join(os.environ["OUT"], "bench.json")).read().strip().splitlines()[-1])
print(o["ms_per_step"], o["value"], "seq", o["sequential"]["ms_per_step"], "pair", o["pair_roofline"]["frac"], "fe", o["roofline"]["frac"], o["roofline"]["kernel"], o["roofline"]["kernel_ms"], o.get("bitwise_equal_to_sequential"),
      {k: o[k]["ms_per_step"] for k in o if isinstance(o[k], dict) and "ms_per_step" in o[k] and k != "sequential"})
PY
