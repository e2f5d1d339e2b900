"""The default front-end kernel's LDS reads stay unpaired (no GPU needed): frontend_pk3.hip compiled to gfx950 assembly with the
library's flags, the body of frontend_pk3_kernel<512, 10, false, false> (the bench's 4020 front-end) has no ds_read2_b64 -- the pair
costs 8 LDS-array cycles where two ds_read_b64 take 2 + 2 (lds_read_unpaired in frontend_pk3.hip) -- and the kernel keeps three waves per
SIMD without scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tc-resnet_amd", "csrc")
KERNEL = "_ZN3tcr19frontend_pk3_kernelILi512ELi10ELb0ELb0EEEvNS_12FrontendArgsE"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("pk3_isa") / "frontend_pk3.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           "--cuda-device-only", "-S", os.path.join(CSRC, "frontend_pk3.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    start = re.search(r"^" + KERNEL + r":", text, re.M).start()
    end = text.index("\n.Lfunc_end", start)
    body = text[start:end]
    tail = text[end:]
    meta = {}
    for key in ("NumVgprs", "ScratchSize", "Occupancy"):
        m = re.search(r"^; " + key + r": (\d+)", tail, re.M)
        assert m, key
        meta[key] = int(m.group(1))
    return body, meta


def test_default_frontend_kernel_has_no_paired_b64_reads(kernel_asm):
    body, _ = kernel_asm
    ops = re.findall(r"^\s+(ds_read\w*)", body, re.M)
    assert "ds_read_b64" in ops
    assert "ds_read2_b64" not in ops and "ds_read2st64_b64" not in ops, sorted(set(ops))


def test_default_frontend_kernel_keeps_three_waves_without_scratch(kernel_asm):
    _, meta = kernel_asm
    assert meta["NumVgprs"] <= 168, meta
    assert meta["ScratchSize"] == 0, meta
    assert meta["Occupancy"] == 3, meta
