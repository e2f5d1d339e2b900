"""bench.py --dump-outputs: the last timed step's (logits, probs) as float32 .npy, the same from run to run (CPU rehearsal on the
emulator build), and the fixed, seeded row sample that keeps a large batch under the size limit."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "_build", "libtcr_emu.so")


def _bench_dump(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["TCR_BENCH_EMU"] = EMU
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--prewarm", "0", "--batch", "8",
           "--legs", "none", "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return {n: np.load(out_dir / f"{n}.npy") for n in ("logits", "probs")}


def test_bench_dumps_the_last_step_outputs(emu_lib, tmp_path):
    a = _bench_dump(tmp_path / "a")
    b = _bench_dump(tmp_path / "b")
    for n in ("logits", "probs"):
        assert a[n].dtype == np.float32 and a[n].shape == (8, 12), (n, a[n].dtype, a[n].shape)
        assert np.array_equal(a[n], b[n]), n
    assert np.abs(a["probs"] - torch.softmax(torch.from_numpy(a["logits"]).double(), 1).numpy()).max() < 1e-6
    assert np.all(np.isfinite(a["logits"])) and np.ptp(a["logits"]) > 0


def test_bench_dump_samples_rows_over_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 2 * 12 * 4)        # ten rows of (logits, probs)
    logits = torch.arange(100 * 12, dtype=torch.float32).reshape(100, 12)
    bench.dump_outputs(str(tmp_path / "a"), {"logits": logits, "probs": logits + 0.5}, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), {"logits": logits, "probs": logits + 0.5}, 0, 1)
    la, pa = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "a" / "probs.npy")
    assert la.shape == (10, 12) and la.dtype == np.float32
    rows = la[:, 0].astype(np.int64) // 12
    assert np.all(np.diff(rows) > 0) and np.array_equal(pa, la + 0.5)               # the same rows of every array, in order
    assert np.array_equal(la, np.load(tmp_path / "b" / "logits.npy"))              # a fixed sample
    bench.dump_outputs(str(tmp_path / "c"), {"logits": logits}, 1, 2)
    assert os.path.exists(tmp_path / "c" / "logits_rank1.npy")
