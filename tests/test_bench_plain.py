"""A plain `bench.py` run times the headline alone; --full adds the figures that take runs of their own (CPU rehearsal on the
emulator build: control flow and the JSON line, not a measurement)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "_build", "libtcr_emu.so")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "phases_ms", "sequential", "bitwise_equal_to_sequential", "cold_ms_per_step", "cpu_baseline", "train", "latency_batch_1")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["TCR_BENCH_EMU"] = EMU
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--prewarm", "0", "--batch", "8", *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)


def _line(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_carries_the_headline_alone(emu_lib):
    out = _line(_bench())
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert not [k for k in FULL_ONLY if k in out], sorted(out)


def test_full_run_adds_what_takes_runs_of_its_own(emu_lib):
    out = _line(_bench("--full", "--legs", "none", "--no-cpu-baseline"))
    assert all(k in out for k in HEADLINE + ("roofline", "phases_ms", "sequential", "cold_ms_per_step")), sorted(out)


def test_legs_ask_for_full():
    r = _bench("--legs", "train")
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]
