#!/usr/bin/env python3
"""Static instruction mix of one kernel, per basic block, from the gfx950 assembly of one source file:

    python scripts/isa_loop_counts.py fused.hip net_fused_tc8_kernelILi8ELi49ELi0ELi6E [-D...] [--asm-out FILE] [--min-insts N]

Compiles tc-resnet_amd/csrc/<file> to device assembly with the library's flags (those of scripts/kernel_regs.sh; no GPU needed), takes the
first kernel whose mangled name contains the substring, and prints per basic block its loop depth (the assembler's own loop comments) and
the counts of MFMA / other VALU / SALU / DS / VMEM / s_waitcnt instructions with the six most frequent VALU opcodes; then the same summed
per loop depth and for the kernel, and every v_readlane / v_writelane count by depth.  Counts are STATIC (per pass through a block):
multiply by trip counts yourself.  Block labels move from build to build; the depth and the mix identify a block."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tc-resnet_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLASSES = ("mfma", "valu", "salu", "ds", "vmem", "wait")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "mfma"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"           # (scalar ALU, scalar memory, branches and s_nop alike: everything the scalar unit issues)
    return None


def assemble(src, extra):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
               "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out] + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("hipcc failed:\n" + r.stderr[-3000:])
        with open(out) as fh:
            return fh.read()


def kernel_text(asm, pat):
    """lines of the first function whose label contains `pat` (from its label to its .Lfunc_end)"""
    lines = asm.splitlines()
    for i, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m and pat in m.group(1) and not m.group(1).startswith(".L"):
            for j in range(i + 1, len(lines)):
                if lines[j].startswith(".Lfunc_end"):
                    return m.group(1), lines[i + 1:j]
    sys.exit(f"no kernel matching {pat!r}")


def blocks_of(lines):
    """[(label, depth, Counter of classes, Counter of valu opcodes)] in layout order"""
    out = []
    cur = ["entry", 0, collections.Counter(), collections.Counter(), False]
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            out.append(cur)
            cur = [m.group(1), 0, collections.Counter(), collections.Counter(), False]
        s = ln.strip()
        if not cur[4]:          # loop comments between a label and the block's first instruction
            d = re.search(r";.*(?:This (?:Inner )?Loop Header|in Loop: Header=\S+).*Depth=(\d+)", ln)
            if d:
                cur[1] = max(cur[1], int(d.group(1)))
        body = s.split(";")[0].strip()
        if not body or body.endswith(":") or body.startswith("."):
            continue
        op = body.split()[0]
        cls = classify(op)
        if cls is None:
            continue
        cur[4] = True
        cur[2][cls] += 1
        if cls == "valu":
            cur[3][op] += 1
    out.append(cur)
    return [(b[0], b[1], b[2], b[3]) for b in out if sum(b[2].values())]


def row(name, depth, cls, ops):
    top = ", ".join(f"{o} x{n}" for o, n in ops.most_common(6))
    return f"{name:<12} {depth:>5} " + " ".join(f"{cls.get(c, 0):>6}" for c in CLASSES) + "  " + top


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source")
    ap.add_argument("kernel", help="substring of the kernel's (mangled) name")
    ap.add_argument("--asm-out", help="also keep the whole assembly in this file")
    ap.add_argument("--min-insts", type=int, default=12, help="blocks with fewer instructions are only counted in the sums")
    args, extra = ap.parse_known_args()
    asm = assemble(args.source, extra)
    if args.asm_out:
        with open(args.asm_out, "w") as fh:
            fh.write(asm)
    name, lines = kernel_text(asm, args.kernel)
    blocks = blocks_of(lines)
    print(f"kernel {name}: {len(blocks)} basic blocks")
    head = f"{'block':<12} {'depth':>5} " + " ".join(f"{c:>6}" for c in CLASSES) + "  most frequent VALU opcodes"
    print(head)
    by_depth = collections.defaultdict(lambda: (collections.Counter(), collections.Counter()))
    lanes = collections.defaultdict(collections.Counter)
    for label, depth, cls, ops in blocks:
        if sum(cls.values()) >= args.min_insts:
            print(row(label, depth, cls, ops))
        by_depth[depth][0].update(cls)
        by_depth[depth][1].update(ops)
        for o in ("v_readlane_b32", "v_writelane_b32"):
            if ops[o]:
                lanes[o][depth] += ops[o]
    print("-- summed per loop depth --")
    total = (collections.Counter(), collections.Counter())
    for depth in sorted(by_depth):
        print(row("all blocks", depth, *by_depth[depth]))
        total[0].update(by_depth[depth][0])
        total[1].update(by_depth[depth][1])
    print(row("kernel", max(by_depth), *total))
    for o in ("v_readlane_b32", "v_writelane_b32"):
        print(f"{o} by loop depth: " + (", ".join(f"depth {d}: {n}" for d, n in sorted(lanes[o].items())) or "none"))


if __name__ == "__main__":
    main()
