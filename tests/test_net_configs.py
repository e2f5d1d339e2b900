"""The TC-ResNet engine across its configuration space: widths, explicit channel lists, coefficient counts, frame counts, label sets
and batches away from the flagship shapes, so that every fallback and generic kernel form is compared with the float64 oracle
(oracle/numpy_ref.py) at a shape where it is what runs BY DEFAULT -- eval logits / probabilities / ranges / argmax, train-mode logits /
loss / every gradient / moving statistics, the optimiser steps, run-to-run reproducibility, the staged sync-BN API; which kernel
families ran, from the emulator's launch log; writes outside what the C ABI declares; the detection stack on a non-flagship net.
Emulator (`-m "not gpu"`) and MI355X (`-m gpu`): the same rows, shapes and batches (the dispatch is host code)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from oracle.make_golden import dropout_mask
from tests import common as Cm

PROB_TOL = 1e-5            # probabilities and ranges
GRAD_RTOL = 2e-4           # every gradient tensor, relative to max(|ref|, 1e-3)
STAT_TOL = 1e-5            # moving statistics, x max(1, |ref|)
STEP_TOL = 2e-5            # parameters after one momentum step
# One Adam / RMSProp / EMA step in float32 against the float64 formulas on the SAME (kernel-produced) gradient: a handful of float32
# operations whose result is a parameter of magnitude < 2, i.e. half an ulp (6e-8) from the final rounding plus the update's own
# rounding (|update| <= ~3.2 lr = 3.2e-3, a few ulps of that: < 1e-9).  1e-6 is eight ulps of the largest parameter.
OPT_TOL = 1e-6
MIN_BN_POSITIONS = 8       # batch x T' of the last BN layer: train-mode BN over fewer positions is ill-conditioned (T = 1 at batch 2: 6.6e-5)

# (id, net, width or explicit channel list, in_channels, t_in, num_classes, batch, expected paths)
# Expected paths, one token per group (asserted from the emulator's launch log; a group left out of a row is not asserted):
#   eval:   small / static / generic = the whole-network kernel's three forms (fused.hip), layers = the per-layer kernels
#   conv0:  mfma / valu  = the first conv of the per-layer forward (launch_conv_mfma returns 1 for cin % 4 != 0)
#   convs:  mfma / mixed / valu = all per-layer forward convs on the matrix cores / some / none ("valu": knob 0 changes no bit)
#   fwd:    phases-static / phases / chain = training forward by compile-time phases, generic phases, the per-layer chain
#   ks:     4 / 2 / 1 = the K-split of the first conv's raw-epilogue launch in the per-layer training forward (chain rows with an
#           MFMA first conv).  The split by GROUP count needs batch x T >= 131072 positions, outside what a test may run: the rows
#           take the three values through the chunk count (K * ceil(cin / 16): 40, 20 and 16 coefficients).
#   bwd:    lazy / chain = bwd_lazy.hip / the per-layer backward
#   wgrad0: lds / 16b    = the first conv's filter gradient by the LDS-staged kernel / the 16-byte-load kernel
#   wide:   yes / no     = a layer of more than 80 output channels: its filter gradient reduced at once (not deferrable)
#   down:   fused / mixed / separate = the per-layer forward's conv_a + 1x1 shortcut pairs in one launch (needs cin % 4 == 0) or apart
#   dgrad:  mfma / mixed / valu / lazy = the per-layer backward's data gradients (conv_dgrad_mfma_covers: cout % 4); lazy: bwd_lazy.hip's own
#   shortcut: early / late / lazy = the per-layer backward's shortcut data gradient ahead of conv_a's (down_dgrad_first) or behind it
FLAG = "conv0:mfma convs:mfma bwd:lazy wgrad0:lds wide:no"
ROWS = [
    # ---- TCResNet8-1.0 on 40 coefficients: the flagship net at and away from its two frame counts
    ("tc8_w1_t49_small",   "TCResNet8", 1.0, 40, 49, 12, 3, "eval:small fwd:phases-static down:fused dgrad:lazy shortcut:lazy " + FLAG),
    ("tc8_w1_t98",         "TCResNet8", 1.0, 40, 98, 12, 2, "eval:static fwd:phases-static down:fused dgrad:lazy shortcut:lazy " + FLAG),
    ("tc8_w1_t65_generic", "TCResNet8", 1.0, 40, 65, 12, 3, "eval:generic fwd:phases down:fused dgrad:lazy shortcut:lazy " + FLAG),      # neither 49 nor 98: the generic walk
    # fewer frames than taps.  A stride-2 data gradient over ONE input frame has an empty odd phase: configure_lazy declines (block 0 at
    # one frame, block 1 at two), so the per-layer backward runs on a net of <= 48 channels
    ("tc8_w1_t1",          "TCResNet8", 1.0, 40, 1, 12, 9, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:lds wide:no down:fused dgrad:mfma shortcut:early"),
    ("tc8_w1_t2",          "TCResNet8", 1.0, 40, 2, 12, 9, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:lds wide:no down:fused dgrad:mfma shortcut:early"),
    ("tc8_w1_t31",         "TCResNet8", 1.0, 40, 31, 12, 3, "eval:generic fwd:phases down:fused dgrad:lazy shortcut:lazy " + FLAG),       # one short of a 32-position wave group
    # 40 x 308 floats per utterance: beyond the LDS-staged filter gradient's 8 x 576 cap
    ("tc8_w1_t300",        "TCResNet8", 1.0, 40, 300, 12, 2, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:lazy wgrad0:16b wide:no down:fused dgrad:lazy shortcut:lazy"),
    # ---- widths and channel lists
    ("tc8_w05_t15",        "TCResNet8", 0.5, 40, 15, 12, 5, "eval:generic fwd:phases down:fused dgrad:lazy shortcut:lazy " + FLAG),       # 8/12/16/24; one short of a 16-position unit
    # 12/18/24/36: cin 18 inside block 1 -> eval off the fused kernel, no phases, no lazy backward
    ("tc8_w075_t49",       "TCResNet8", 0.75, 40, 49, 12, 3, "eval:layers conv0:mfma convs:mixed fwd:chain ks:4 bwd:chain wgrad0:lds wide:no down:mixed dgrad:mixed shortcut:early"),
    # odd everywhere, 13 coefficients: the VALU conv throughout
    ("tc8_odd_f13_t31",    "TCResNet8", [7, 10, 14, 21], 13, 31, 12, 3, "eval:layers conv0:valu convs:valu fwd:chain bwd:chain wgrad0:16b wide:no down:separate dgrad:valu shortcut:late"),
    # odd channels behind 40 coefficients (even T: pads (3, 4)); 7 x 58 floats per row: the LDS-staged filter gradient's (cout*tpo) % 4
    ("tc8_odd_f40_t50",    "TCResNet8", [7, 10, 14, 21], 40, 50, 12, 2, "eval:layers conv0:mfma convs:mixed fwd:chain ks:4 bwd:chain wgrad0:16b wide:no down:separate dgrad:valu shortcut:late"),
    # 32/48/64/96: lazy off (> 48), 96 > 80 not deferrable; the early-shortcut policy's 64-frame edge
    ("tc8_w2_t63",         "TCResNet8", 2.0, 40, 63, 12, 2, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:lds wide:yes down:fused dgrad:mfma shortcut:late"),
    ("tc8_w2_t64",         "TCResNet8", 2.0, 40, 64, 12, 2, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:lds wide:yes down:fused dgrad:mfma shortcut:early"),
    ("tc8_w2_t65",         "TCResNet8", 2.0, 40, 65, 12, 2, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:lds wide:yes down:fused dgrad:mfma shortcut:early"),
    # 48/72/96/144: three output tiles in the first conv (no LDS-staged instance)
    ("tc8_w3_t33",         "TCResNet8", 3.0, 40, 33, 12, 2, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:16b wide:yes down:fused dgrad:mfma shortcut:late"),
    # ---- in_channels
    # 4/7/9/14 on ONE coefficient, the largest head
    ("tc8_w03_f1_c46",     "TCResNet8", 0.3, 1, 49, 46, 3, "eval:layers conv0:valu convs:mixed fwd:chain bwd:chain wgrad0:16b wide:no down:mixed dgrad:valu shortcut:late"),
    # 10 coefficients, flagship channels: per-layer forward (conv0 on the VALU conv) but the LAZY backward (it never reads conv0's input width)
    ("tc8_w1_f10_c2",      "TCResNet8", 1.0, 10, 49, 2, 3, "eval:layers conv0:valu convs:mixed fwd:chain bwd:lazy wgrad0:16b wide:no down:fused dgrad:lazy shortcut:lazy"),
    ("tc8_w1_f13_c35",     "TCResNet8", 1.0, 13, 49, 35, 3, "eval:layers conv0:valu convs:mixed fwd:chain bwd:lazy wgrad0:16b wide:no down:fused dgrad:lazy shortcut:lazy"),
    ("tc8_w1_f20_t17",     "TCResNet8", 1.0, 20, 17, 12, 4, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:lazy wgrad0:16b wide:no down:fused dgrad:lazy shortcut:lazy"),   # two input tiles
    ("tc8_w1_f64_t16",     "TCResNet8", 1.0, 64, 16, 12, 4, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:lazy wgrad0:16b wide:no down:fused dgrad:lazy shortcut:lazy"),   # four input tiles
    # 37 coefficients: three input tiles, so the LDS-staged filter gradient has an instance -- and (37 x 33) % 4 != 0 sends it back
    ("tc8_w1_f37_t25",     "TCResNet8", 1.0, 37, 25, 12, 3, "eval:layers conv0:valu convs:mixed fwd:chain bwd:lazy wgrad0:16b wide:no down:fused dgrad:lazy shortcut:lazy"),
    # first conv's K-split by chunk count in the per-layer training forward: 20 coefficients -> 2, 16 -> 1 (40: tc8_w075_t49 -> 4)
    ("tc8_w075_f20_t32",   "TCResNet8", 0.75, 20, 32, 12, 3, "eval:layers conv0:mfma convs:mixed fwd:chain ks:2 bwd:chain wgrad0:16b wide:no down:mixed dgrad:mixed shortcut:early"),
    ("tc8_w075_f16_t33",   "TCResNet8", 0.75, 16, 33, 12, 3, "eval:layers conv0:mfma convs:mixed fwd:chain ks:1 bwd:chain wgrad0:16b wide:no down:mixed dgrad:mixed shortcut:early"),
    # ---- TCResNet14: identity shortcuts
    ("tc14_w1_t32",        "TCResNet14", 1.0, 40, 32, 12, 3, "eval:generic fwd:phases down:fused dgrad:lazy shortcut:lazy " + FLAG),
    # 12/18/18/24/24/36/36 on 13 coefficients, 35 words, 1.5 s clips at 30 / 20 ms: identity shortcuts at an odd channel count
    ("tc14_w075_f13_c35",  "TCResNet14", 0.75, 13, 74, 35, 2, "eval:layers conv0:valu convs:mixed fwd:chain bwd:chain wgrad0:16b wide:no down:mixed dgrad:mixed shortcut:early"),
    # (eval: the compile-time TCResNet14-1.5 instances exist for 8 and 16 waves, i.e. for groups of several utterances; a batch this
    #  small runs one utterance per group on 4 waves -- the generic walk.  EXTRA_EVAL reaches the instance with a group of 8.)
    ("tc14_w15_t49",       "TCResNet14", 1.5, 40, 49, 12, 2, "eval:generic fwd:phases-static conv0:mfma convs:mfma bwd:chain wgrad0:lds wide:no down:fused dgrad:mfma shortcut:late"),
    ("tc14_w15_t60",       "TCResNet14", 1.5, 40, 60, 12, 2, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:lds wide:no down:fused dgrad:mfma shortcut:late"),
    # Long clip.  forward_infer_fused: sz = {36 x 107, 24 x 206, 36 x 107} + bank pads ~ 12.7 K floats = 51 KB per utterance: the group
    # of 8 the policy starts from no longer fits 160 KB (3 do); the fused generic walk still runs.  40 x 206 > 8 x 576: wgrad0 16b.
    ("tc14_w15_t198_long", "TCResNet14", 1.5, 40, 198, 12, 2, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:16b wide:no down:fused dgrad:mfma shortcut:early"),
    # Does not fit at all: a 200-channel first conv at 200 frames is 200 x 208 floats = 166 400 B for ONE utterance's conv0 output
    # (> 160 KB), so eval takes the per-layer kernels although every cin % 4 == 0; the training phase staging that tensor does not fit
    # either.  (A plain width multiplier gets there only at sizes the emulator cannot afford: width 6 at 200 frames.)
    ("tc8_c200_t200_nolds", "TCResNet8", [200, 8, 12, 16], 40, 200, 12, 2, "eval:layers conv0:mfma convs:mfma fwd:chain ks:4 bwd:chain wgrad0:16b wide:yes down:fused dgrad:mfma shortcut:early"),
    ("tc14_w2_f64_t31",    "TCResNet14", 2.0, 64, 31, 12, 3, "eval:generic fwd:phases conv0:mfma convs:mfma bwd:chain wgrad0:16b wide:yes down:fused dgrad:mfma shortcut:late"),
    # 16 blocks, 35 BN units (two widenings, fourteen identity blocks): more than kFusedMaxLayers = 32, so eval leaves the fused kernel
    # although every cin % 4 == 0 and 5 KB per utterance would fit; the phases and the lazy backward run at that depth
    ("tc_deep_35_units",   "TCResNet14", [16] + [24] * 8 + [32] * 8, 40, 33, 12, 2, "eval:layers conv0:mfma convs:mfma fwd:phases bwd:lazy wgrad0:lds wide:no down:fused dgrad:lazy shortcut:lazy"),
]
ROW_IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}

# eval at further batches (utterances cycled from the row's own).  (batch, TCR_TUNE_FUSED_GROUP, eval path, bitwise): bitwise the same
# utterances at the row's batch -- the 64-utterance edge of the small-batch kernel, ragged batches at one utterance per group (what
# the policy picks below 512 groups) and at groups of 8 (a last group of 3) -- or, where the other batch reaches ANOTHER kernel form
# that is not documented bitwise (the static TCResNet14-1.5 instance against the generic walk), against the oracle.
EXTRA_EVAL = {"tc8_w1_t49_small": ((1, 0, "small", True), (64, 0, "small", True), (67, 0, "static", True), (67, 8, "static", True)),
              "tc8_w1_t65_generic": ((1, 0, "generic", True), (131, 0, "generic", True), (131, 8, "generic", True)),
              "tc14_w15_t49": ((67, 8, "static", False),)}
DROPOUT_ROWS = ["tc8_w1_t49_small", "tc8_w1_f10_c2", "tc14_w15_t49", "tc8_w075_t49", "tc8_w2_t64"]     # keep_prob 0.5 + label smoothing
OPTIM_ROWS = ["tc8_w1_t49_small", "tc8_w075_t49"]                                                      # Adam / RMSProp / EMA
STAGED_ROWS = ["tc8_odd_f13_t31", "tc8_w2_t64", "tc14_w1_t32"]                                         # sync-BN hand-off, identity hook
GUARD_ROWS = ["tc8_odd_f13_t31", "tc8_w1_t1", "tc14_w15_t198_long"]                                    # writes outside the declared buffers
# C-ABI calls whose every pointer starts one float behind a 16-byte boundary: {row: paths that differ from the row's aligned ones}
UNALIGNED_ROWS = {"tc8_w1_t49_small": {"eval": "static", "wgrad0": "16b"}, "tc8_w075_t49": {"wgrad0": "16b"}, "tc_deep_35_units": {"wgrad0": "16b"}}


def paths_of(row):
    return dict(tok.split(":") for tok in row[7].split())


def channels_of(row):
    return Cm.net_channels(row[1], row[2])


def last_frames(row):
    t = row[4]
    ch = channels_of(row)
    for a, b in zip(ch[:-1], ch[1:]):
        t = -(-t // 2) if a != b else t
    return t


# ---- the launch log of the emulator build --------------------------------------------------------------------------------------------
def launch_log(lib):
    """Kernel launches since the last clear (tests/emu/hip/hip_runtime.h): one text per launch, in order."""
    dll = lib._dll
    dll.tcr_emu_launch_log_read.restype, dll.tcr_emu_launch_log_read.argtypes = C.c_long, [C.c_char_p, C.c_long]
    n = dll.tcr_emu_launch_log_read(None, 0)
    buf = C.create_string_buffer(n)
    dll.tcr_emu_launch_log_read(buf, n)
    lines = buf.value.decode().split("\n")[:-1]
    assert not any(ln.startswith("!dropped") for ln in lines), lines[-1]
    return lines


def clear_log(lib):
    lib._dll.tcr_emu_launch_log_clear.restype = None
    lib._dll.tcr_emu_launch_log_clear()


class Log:
    """`with Log(lib) as g:` -> g.entries, the launches of the block (emulator; empty on the GPU library)."""

    def __init__(self, lib):
        self.lib, self.entries = lib, []

    def __enter__(self):
        if self.lib.kind == "emu":
            clear_log(self.lib)
        return self

    def __exit__(self, *exc):
        if self.lib.kind == "emu":
            self.entries = launch_log(self.lib)
        return False

    def has(self, name):
        return any(name in e for e in self.entries)


# Template parameters of the kernels whose instance the checks below read, in declaration order (conv.hip, mfma.hip).  The log holds
# the DEMANGLED instance ("void tcr::conv_mfma_ksplit_kernel<3, 1, 1, false, 4>(tcr::ConvArgs, ...)"); a kernel whose parameter list
# changes fails `targs` with that message instead of a wrong token.
TEMPLATE_ARGS = {"conv_fwd_kernel": ("K", "S", "CT", "P", "EPI", "KS"), "conv_mfma_kernel": ("K", "S", "MT", "EPI", "DOWN", "LB"),
                 "conv_mfma_ksplit_kernel": ("K", "S", "MT", "DOWN", "KS"), "conv_dgrad_kernel": ("K", "S", "CT")}


def kernel_of(entry):
    """The kernel's plain name: of the demangled instance where the log has one, else of the launch expression."""
    text = entry.split(" = ", 1)[1] if " = " in entry else entry
    head = text.split("(")[0] if "<" not in text.split("(")[0] else text.split("<")[0]
    return head.replace("void ", "").strip().strip("()").split("::")[-1]


def targs(entry):
    """{template parameter: text} of a logged instance of one of TEMPLATE_ARGS' kernels."""
    name = kernel_of(entry)
    assert " = " in entry, ("the launch log has no demangled instance for", entry)
    inst = entry.split(" = ", 1)[1]
    body, depth = inst[inst.index("<") + 1:], 1
    for i, ch in enumerate(body):
        depth += (ch == "<") - (ch == ">")
        if depth == 0:
            body = body[:i]
            break
    vals = [v.strip() for v in body.split(",")]
    assert len(vals) == len(TEMPLATE_ARGS[name]), ("tests/test_net_configs.py::TEMPLATE_ARGS is out of date for", name, "logged:", inst)
    return dict(zip(TEMPLATE_ARGS[name], vals))


def eval_family(g):
    names = {kernel_of(e) for e in g.entries}
    fam = [k for k, ks in (("small", {"net_small_tc8_kernel"}), ("static", {"net_fused_tc8_kernel", "net_fused_tc14w_kernel"}),
                           ("generic", {"net_fused_kernel"})) if names & ks]
    assert len(fam) <= 1, fam
    return fam[0] if fam else "layers"


def conv_entries(g):
    """The implicit-GEMM / VALU conv launches of a pass, in order (a forward's 1x1 shortcut alone has kernels of its own: conv1x1_*)."""
    return [e for e in g.entries if kernel_of(e) in ("conv_fwd_kernel", "conv_mfma_kernel", "conv_mfma_ksplit_kernel")]


def three_way(flags, names):
    return names[0] if all(flags) else (names[2] if not any(flags) else names[1])


def layer_families(g):
    """A per-layer eval forward: the first conv and all convs on the matrix cores or not; the blocks' conv_a + `down` pairs in one launch
    (DOWN instances of the matrix-core conv) or apart (a conv1x1_* launch)."""
    ce = conv_entries(g)
    assert ce, "no per-layer conv launch in the log"
    valu = [kernel_of(e) == "conv_fwd_kernel" for e in ce]
    fused = sum(targs(e)["DOWN"] == "true" for e in ce if kernel_of(e) != "conv_fwd_kernel")
    apart = sum(kernel_of(e).startswith("conv1x1_") for e in g.entries)
    return {"conv0": "valu" if valu[0] else "mfma", "convs": three_way(valu, ("valu", "mixed", "mfma")),
            "down": "none" if fused + apart == 0 else ("fused" if apart == 0 else ("separate" if fused == 0 else "mixed"))}


def train_fwd_families(g):
    names = {kernel_of(e) for e in g.entries}
    out = {"fwd": "phases-static" if "train_phase_s_kernel" in names else ("phases" if "train_phase_kernel" in names else "chain")}
    ce = conv_entries(g)
    if out["fwd"] == "chain" and ce and kernel_of(ce[0]) != "conv_fwd_kernel":
        out["ks"] = targs(ce[0])["KS"] if kernel_of(ce[0]) == "conv_mfma_ksplit_kernel" else "1"
    return out


def bwd_families(g):
    """A backward pass.  The per-layer chain's data gradients are the matrix-core conv over dy (one launch per output phase: 9 taps for
    conv_b, 5 and 4 for a stride-2 conv_a, 1 for the stride-2 1x1 shortcut; launch_conv_dgrad_mfma) or conv_dgrad_kernel<K, S>.
    shortcut: of the first block with a shortcut conv the backward meets, whether that conv's data gradient is launched BEFORE conv_a's
    (net.cpp::down_dgrad_first) or behind it."""
    names = [kernel_of(e) for e in g.entries]
    out = {"bwd": "lazy" if "bwd_lazy_kernel" in names else "chain", "wgrad0": "lds" if "conv_wgrad_lds_kernel" in names else "16b",
           "wide": "yes" if "wgrad_reduce_kernel" in names else "no"}
    if out["bwd"] == "lazy":
        out.update(dgrad="lazy", shortcut="lazy")
        return out
    dg = [(kernel_of(e) != "conv_dgrad_kernel", int(targs(e)["K"]), int(targs(e)["S"])) for e in g.entries
          if kernel_of(e) in ("conv_dgrad_kernel", "conv_mfma_kernel", "conv_mfma_ksplit_kernel")]
    assert dg, "no data-gradient launch in the log"
    out["dgrad"] = three_way([m for m, _, _ in dg], ("mfma", "mixed", "valu"))
    is_down = [(m and k == 1) or (not m and (k, st) == (1, 2)) for m, k, st in dg]
    is_a = [(m and k in (4, 5)) or (not m and (k, st) == (9, 2)) for m, k, st in dg]
    assert any(is_down) and any(is_a), dg
    out["shortcut"] = "early" if is_down.index(True) < is_a.index(True) else "late"
    return out


def assert_paths(lib, row, got):
    """The families the row was written for ran, the others of each group did not (each group has exactly one token)."""
    if lib.kind != "emu":
        return
    want = paths_of(row)
    for k, v in got.items():
        if k in want:
            assert want[k] == v, (row[0], k, "expected", want[k], "ran", v)


# ---- one row ------------------------------------------------------------------------------------------------------------------------
_SETUP = {}


def row_setup(row):
    """Oracle side of a row: the architecture, float32-rounded parameters / statistics as float64, the input batch whose train-mode ReLU
    inputs stay farthest from zero (of 12 candidates), its eval / train forwards and gradients."""
    name = row[0]
    if name in _SETUP:
        return _SETUP[name]
    _, net, width, f, t, nc, batch, _ = row
    arch = Cm.make_arch(net, width, f, nc)
    p, s = R.init_params(arch, 5)
    R.randomize_bn(arch, p, s, 6)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    s = {k: v.astype(np.float32).astype(np.float64) for k, v in s.items()}
    best = None
    for seed in range(300, 312):
        x = np.random.RandomState(seed).uniform(-2.0, 2.0, (batch, t, f)).astype(np.float32)
        tr = R.forward(arch, p, s, x.astype(np.float64), True)
        mg = Cm.relu_margin(arch, tr)
        if best is None or mg > best[0]:
            best = (mg, x, tr)
    margin, x, tr = best
    labels = R.synth_labels(batch, nc).astype(np.float64)
    x64 = x.astype(np.float64)
    st = dict(arch=arch, p=p, s=s, x=x, x64=x64, labels=labels, margin=margin, tr=tr, ev=R.forward(arch, p, s, x64, False),
              grads=R.backward(arch, p, tr, labels, 0.0), loss=R.loss(tr["logits"], labels, p, 0.0)[1])
    _SETUP.clear()                      # (one row at a time: a worker runs the emulator and the GPU test of a row back to back at most)
    _SETUP[name] = st
    return st


def make_row_net(lib, row, st):
    _, net, width, f, t, nc, _, _ = row
    return Cm.make_net(lib, net, width, t, st["p"], st["s"], in_channels=f, num_classes=nc)


def planar(lib, x):
    return T.features_to_planar(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(Cm.device_of(lib)), lib=lib)


def grad_errors(net, grads, what):
    worst = 0.0
    for k, ref in grads.items():
        got = net.grad_view(k).cpu().numpy().reshape(ref.shape).astype(np.float64)
        e = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-3))
        worst = max(worst, e)
        assert e < GRAD_RTOL, f"{what}: {k}: grad rel err {e}"
    return worst


def stat_errors(net, new_stats, what):
    worst = 0.0
    for k, ref in new_stats.items():
        e = float(np.abs(net._view(k).cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max()))
        worst = max(worst, e)
        assert e < STAT_TOL, f"{what}: {k}: moving statistic err {e}"
    return worst


def reload(net, st):
    sd = dict(st["p"])
    sd.update(st["s"])
    net.load_state_dict(sd)


def check_eval(lib, row, st, net, feat, errs):
    name, batch = row[0], row[6]
    ev = st["ev"]
    with Log(lib) as g:
        logits, probs, ranges = [v.clone() for v in net.forward_infer(feat, want_ranges=True)]
    fam = {"eval": eval_family(g)} if lib.kind == "emu" else {}
    if fam.get("eval") == "layers":
        fam.update(layer_families(g))
    lg = logits.cpu().numpy()
    errs["eval_logits"] = float(np.abs(lg - ev["logits"]).max())
    errs["eval_probs"] = float(np.abs(probs.cpu().numpy() - ev["probs"]).max())
    errs["eval_ranges"] = float(np.abs(ranges.cpu().numpy() - ev["ranges"]).max())
    print(name, "eval", {k: v for k, v in errs.items() if k.startswith("eval")}, fam)
    assert errs["eval_logits"] < Cm.LOGIT_TOL and errs["eval_probs"] < PROB_TOL and errs["eval_ranges"] < PROB_TOL, (name, errs)
    assert np.array_equal(lg.argmax(1), ev["logits"].argmax(1)), name
    # the frozen export's forward: bitwise; the per-layer kernels (what runs where the fused kernel does not apply): against the oracle
    frozen = net.forward_frozen(feat, net.fold_bn(), want_ranges=True)
    for a, b, what in zip(frozen, (logits, probs, ranges), ("logits", "probs", "ranges")):
        assert torch.equal(a, b), (name, "forward_frozen", what)
    try:
        lib.tcr_tune(3, 1)
        with Log(lib) as g:
            layered = [v.clone() for v in net.forward_infer(feat, want_ranges=True)]
    finally:
        lib.tcr_tune(3, 0)
    if lib.kind == "emu":
        assert eval_family(g) == "layers"
        fam.update(layer_families(g))
    for a, what, tol in zip(layered, ("logits", "probs", "ranges"), (Cm.LOGIT_TOL, PROB_TOL, PROB_TOL)):
        e = float(np.abs(a.cpu().numpy() - ev[what]).max())
        errs["eval_layers_" + what] = e
        assert e < tol, (name, "per-layer eval", what, e)
    assert_paths(lib, row, fam)
    # further batches: the same utterances, the same bits
    for b2, grp, want, bitwise in EXTRA_EVAL.get(name, ()):
        idx = np.arange(b2) % batch
        tidx = torch.as_tensor(idx, device=feat.device)
        try:
            lib.tcr_tune(4, grp)
            with Log(lib) as g:
                outs = net.forward_infer(feat[tidx].contiguous(), want_ranges=True)
        finally:
            lib.tcr_tune(4, 0)
        if lib.kind == "emu":
            assert eval_family(g) == want, (name, b2, grp, eval_family(g))
        for a, b, what, tol in zip(outs, (logits, probs, ranges), ("logits", "probs", "ranges"), (Cm.LOGIT_TOL, PROB_TOL, PROB_TOL)):
            if bitwise:
                assert torch.equal(a, b[tidx]), (name, "batch", b2, "group", grp, what)
            else:
                e = float(np.abs(a.cpu().numpy() - ev[what][idx]).max())
                errs[f"eval_b{b2}_g{grp}_{what}"] = e
                assert e < tol, (name, "batch", b2, "group", grp, what, e)
    return logits


def check_train(lib, row, st, net, feat, errs):
    name, nc, batch = row[0], row[5], row[6]
    tr, labels = st["tr"], st["labels"]
    lab = Cm.to_dev(lib, labels)
    stats0 = net.stats.clone()
    with Log(lib) as gf:
        tl, tp, loss = net.forward_train(feat, lab, keep_prob=1.0)
        tl, tp, loss = tl.clone(), tp.clone(), loss.clone()
    with Log(lib) as gb:
        g1 = net.backward().clone()
    if lib.kind == "emu":
        fam = train_fwd_families(gf)
        fam.update(bwd_families(gb))
        assert_paths(lib, row, fam)
        print(name, "train paths", fam)
    errs["train_logits"] = float(np.abs(tl.cpu().numpy() - tr["logits"]).max())
    errs["train_probs"] = float(np.abs(tp.cpu().numpy() - tr["probs"]).max())
    errs["loss"] = abs(float(loss) / batch - st["loss"])
    assert errs["train_logits"] < Cm.LOGIT_TOL and errs["train_probs"] < PROB_TOL and errs["loss"] < 1e-4, (name, errs)
    errs["grads"] = grad_errors(net, st["grads"], name)
    errs["stats"] = stat_errors(net, tr["new_stats"], name)
    pads = torch.ones(net.n_param, dtype=torch.bool)
    for ti in net.tensors.values():
        if ti.arena == 0:
            pads[ti.offset:ti.offset + ti.size] = False
    assert not bool(g1.cpu()[pads].any()), (name, "gradient arena not zero between its tensors")
    print(name, "train", {k: errs[k] for k in ("train_logits", "loss", "grads", "stats")})
    # run-to-run: bitwise (no float atomics, whatever the streams do)
    net.stats.copy_(stats0)
    tl2, _, loss2 = net.forward_train(feat, lab, keep_prob=1.0)
    assert torch.equal(tl, tl2) and float(loss) == float(loss2), (name, "second forward_train differs")
    assert torch.equal(g1, net.backward()), (name, "second backward differs")
    # one momentum step against the closed form
    lr, wd = 0.1, 0.001
    net.sgd_momentum_step(lr, 0.9, wd)
    worst = 0.0
    for k, ref in st["grads"].items():
        w1 = st["p"][k] - lr * (ref + (wd * st["p"][k] if R.is_l2_param(k) else 0.0))
        worst = max(worst, float(np.abs(net._view(k).cpu().numpy().reshape(w1.shape) - w1).max()))
    errs["momentum_step"] = worst
    assert worst < STEP_TOL, (name, "momentum step", worst)
    reload(net, st)
    return tl, g1


def check_dropout_smoothing(lib, row, st, net, feat, errs):
    """keep_prob 0.5 (the kernels' own generator, restated by oracle.make_golden.dropout_mask) and label smoothing 0.1."""
    name, nc, batch = row[0], row[5], row[6]
    arch, p, s, labels = st["arch"], st["p"], st["s"], st["labels"]
    seed, off, keep, smooth = 17, 5, 0.5, 0.1
    mask = dropout_mask(seed, off, batch, channels_of(row)[-1], keep)
    tr = R.forward(arch, p, s, st["x64"], True, keep_prob=keep, dropout_mask=mask)
    assert Cm.relu_margin(arch, tr) == st["margin"]               # (dropout sits behind the last ReLU: the same conditioning)
    grads = R.backward(arch, p, tr, labels, 0.0, label_smoothing=smooth)
    tl, _, loss = net.forward_train(feat, Cm.to_dev(lib, labels), keep_prob=keep, seed=seed, sample_offset=off, label_smoothing=smooth)
    net.backward()
    e = {"train_logits": float(np.abs(tl.cpu().numpy() - tr["logits"]).max()),
         "loss": abs(float(loss) / batch - R.loss(tr["logits"], labels, p, 0.0, label_smoothing=smooth)[1])}
    assert e["train_logits"] < Cm.LOGIT_TOL and e["loss"] < 1e-4, (name, "dropout + smoothing", e)
    e["grads"] = grad_errors(net, grads, name + " (dropout + smoothing)")
    e["stats"] = stat_errors(net, tr["new_stats"], name + " (dropout + smoothing)")
    print(name, "dropout 0.5 + label smoothing 0.1", e)
    errs.update({"drop_" + k: v for k, v in e.items()})
    reload(net, st)


def check_optimisers(lib, row, st, net, feat, errs):
    """One step each of Adam, RMSProp (with momentum) and the EMA behind it: float64 restatements of optim.hip's formulas on the
    gradient arena the kernels produced (a ReLU-sign difference from the oracle's gradient cannot enter)."""
    name = row[0]
    lab = Cm.to_dev(lib, st["labels"])
    nd = net.n_decay
    lr, wd = 1e-3, 0.001

    def fresh():
        reload(net, st)
        net.slots.clear()
        net.forward_train(feat, lab, keep_prob=1.0)
        g = net.backward().cpu().numpy().astype(np.float64)
        w = net.params.cpu().numpy().astype(np.float64)
        gv = g.copy()
        gv[:nd] += wd * w[:nd]
        return w, gv

    # tf.train.AdamOptimizer, t = 1: lr_t = lr sqrt(1 - b2) / (1 - b1); m = (1 - b1) g; v = (1 - b2) g^2; w -= lr_t m / (sqrt(v) + eps)
    w, gv = fresh()
    b1, b2, eps = 0.9, 0.999, 1e-8
    net.adam_step(lr, 1, b1, b2, eps, weight_decay=wd)
    m, v = (1 - b1) * gv, (1 - b2) * gv * gv
    want = w - lr * np.sqrt(1 - b2) / (1 - b1) * m / (np.sqrt(v) + eps)
    errs["adam"] = float(np.abs(net.params.cpu().numpy() - want).max())
    assert errs["adam"] < OPT_TOL, (name, "adam", errs["adam"])
    assert float(np.abs(net.slots["Adam"].cpu().numpy() - m).max()) < OPT_TOL and float(np.abs(net.slots["Adam_1"].cpu().numpy() - v).max()) < OPT_TOL
    # tf.train.RMSPropOptimizer: ms = ms + (1 - decay)(g^2 - ms), ms0 = 1; mom = momentum mom + lr g / sqrt(ms + eps); w -= mom
    # then tf.train.ExponentialMovingAverage: shadow -= (1 - d)(shadow - w), shadow0 = the variables' initial values
    w, gv = fresh()
    net.ema_init()
    decay, mom, reps, d = 0.9, 0.9, 1e-10, 0.99
    net.rmsprop_step(lr, decay, mom, reps, weight_decay=wd)
    ms = 1.0 + (1 - decay) * (gv * gv - 1.0)
    mv = lr * gv / np.sqrt(ms + reps)
    errs["rmsprop"] = float(np.abs(net.params.cpu().numpy() - (w - mv)).max())
    assert errs["rmsprop"] < OPT_TOL, (name, "rmsprop", errs["rmsprop"])
    net.ema_step(d)
    shadow = w - (1 - d) * (w - (w - mv))
    errs["ema"] = float(np.abs(net.slots["ExponentialMovingAverage"].cpu().numpy() - shadow).max())
    assert errs["ema"] < OPT_TOL, (name, "ema", errs["ema"])
    print(name, "optimisers", {k: errs[k] for k in ("adam", "rmsprop", "ema")})
    net.slots.clear()
    reload(net, st)


def check_valu_knob(lib, row, st, net, feat, eval_logits, train_logits, grads):
    """Visible from outside (asserted on the GPU too): with the scalar-fed VALU convs selected (tcr_tune(0, 1); eval also off the fused
    kernel, tcr_tune(3, 1)) a row expected on the matrix cores gives OTHER bits and the same results within the tolerances; a row
    expected on the VALU conv throughout gives the same bits."""
    name = row[0]
    lab = Cm.to_dev(lib, st["labels"])
    try:
        lib.tcr_tune(0, 1)
        lib.tcr_tune(3, 1)
        ev = net.forward_infer(feat)[0].clone()
        lib.tcr_tune(3, 0)
        tl = net.forward_train(feat, lab, keep_prob=1.0)[0].clone()
        g = net.backward().clone()
    finally:
        lib.tcr_tune(0, 0)
        lib.tcr_tune(3, 0)
    if paths_of(row)["convs"] == "valu":
        assert torch.equal(ev, eval_logits) and torch.equal(tl, train_logits) and torch.equal(g, grads), (name, "the VALU knob changed bits")
    else:
        assert not torch.equal(ev, eval_logits) and not torch.equal(tl, train_logits) and not torch.equal(g, grads), \
            (name, "the default's bits are the VALU convs': the matrix-core kernels were expected to run")
        assert float(np.abs(ev.cpu().numpy() - st["ev"]["logits"]).max()) < Cm.LOGIT_TOL
        assert float(np.abs(tl.cpu().numpy() - st["tr"]["logits"]).max()) < Cm.LOGIT_TOL
        grad_errors(net, st["grads"], name + " (VALU convs)")
    reload(net, st)


def check_net_row(lib, row):
    """One row against the oracle.  Returns its worst errors."""
    name, netname, width, f, t, nc, batch, _ = row
    st = row_setup(row)
    # conditions of the inputs, judged on the oracle alone
    assert st["margin"] > 1e-6, (name, "ReLU margin", st["margin"])
    assert batch * last_frames(row) >= MIN_BN_POSITIONS, (name, batch, last_frames(row))
    net = make_row_net(lib, row, st)
    feat = planar(lib, st["x"])
    errs = {"relu_margin": st["margin"]}
    ev = check_eval(lib, row, st, net, feat, errs)
    tl, g = check_train(lib, row, st, net, feat, errs)
    if name in DROPOUT_ROWS:
        check_dropout_smoothing(lib, row, st, net, feat, errs)
    if name in OPTIM_ROWS:
        check_optimisers(lib, row, st, net, feat, errs)
    check_valu_knob(lib, row, st, net, feat, ev, tl, g)
    if name in STAGED_ROWS:
        Cm.check_staged_equals_unstaged(lib, netname, width, batch, keep_prob=0.5, in_channels=f, num_classes=nc, t_in=t)
    print(name, "worst", errs)
    return errs


def test_rows_take_every_listed_branch():
    """The table itself: both sides of every dispatch predicate (a row that leaves takes its branch with it)."""
    assert len(set(ROW_IDS)) == len(ROWS)
    P = [paths_of(r) for r in ROWS]
    have = lambda **kv: any(all(p.get(k) == v for k, v in kv.items()) for p in P)
    # eval: the three forms of the fused kernel and the per-layer path -- for cin % 4 != 0 and for LDS alone
    assert all(have(eval=e) for e in ("small", "static", "generic", "layers"))
    assert have(eval="layers", convs="mfma") and have(eval="layers", convs="mixed") and have(eval="layers", convs="valu")
    flag = [r for r in ROWS if (r[1], r[2], r[3]) in (("TCResNet8", 1.0, 40), ("TCResNet14", 1.5, 40))]
    assert {(r[1], paths_of(r)["eval"]) for r in flag} >= {("TCResNet8", "static"), ("TCResNet8", "generic"), ("TCResNet14", "generic")}
    assert {b for v in EXTRA_EVAL.values() for b, _, _, _ in v} >= {1, 64, 67, 131}
    assert {(ROW[n][1], w) for n, v in EXTRA_EVAL.items() for _, _, w, _ in v} >= {("TCResNet8", "small"), ("TCResNet8", "static"), ("TCResNet14", "static")}
    # launch_conv_mfma's cin % 4; the 1x1 kernel against the fused conv_a + down launch (needs cin % 4 == 0)
    assert have(conv0="mfma") and have(conv0="valu") and all(have(down=v) for v in ("fused", "mixed", "separate"))
    # training forward: static / generic phases / chain; the first conv's K-split
    assert all(have(fwd=v) for v in ("phases-static", "phases", "chain")) and all(have(ks=v) for v in ("4", "2", "1"))
    # backward: lazy x phases, lazy x chain forward, chain x phases, chain x chain; in the rows with dropout + label smoothing too
    combos = {(p["fwd"].split("-")[0], p["bwd"]) for p in P}
    assert combos == {("phases", "lazy"), ("chain", "lazy"), ("phases", "chain"), ("chain", "chain")}
    assert {(paths_of(ROW[n])["fwd"].split("-")[0], paths_of(ROW[n])["bwd"]) for n in DROPOUT_ROWS} == combos
    # lazy off by width (> 48 channels), by a channel count that is no multiple of 4, and where configure_lazy declines a flagship net
    assert any(channels_of(r)[-1] > 48 for r in ROWS) and any(channels_of(r)[-1] <= 48 and paths_of(r)["bwd"] == "chain" for r in ROWS)
    assert any(channels_of(r) == [16, 24, 32, 48] and paths_of(r)["bwd"] == "chain" for r in ROWS)
    # the MFMA data gradient (conv_dgrad_mfma_covers), the filter gradient of > 80 channels, the first conv's LDS-staged form and each way out
    assert all(have(dgrad=v) for v in ("mfma", "mixed", "valu", "lazy")) and have(wide="yes") and have(wide="no")
    assert have(wgrad0="lds") and have(wgrad0="16b")
    out = [r for r in ROWS if paths_of(r)["wgrad0"] == "16b"]
    assert any(-(-r[3] // 16) != 3 for r in out)                                                   # no instance: input tiles
    assert any(-(-r[3] // 16) == 3 and channels_of(r)[0] > 32 for r in out)                        # no instance: output tiles
    assert any(-(-r[3] // 16) == 3 and (r[3] * (r[4] + 8)) % 4 for r in out)                       # (cin * tpi) % 4
    assert any(-(-r[3] // 16) == 3 and channels_of(r)[0] <= 32 and (channels_of(r)[0] * (r[4] + 8)) % 4 for r in out)      # (cout * tpo) % 4
    assert any(r[3] == 40 and channels_of(r)[0] <= 32 and r[3] * (r[4] + 8) > 8 * 576 for r in out)   # the 8 x 576 cap
    # ... and its 16-byte alignment gates (params: the small-batch eval kernel; x / dy / raw: the LDS-staged filter gradient; the phases'
    # and the lazy backward's 16-byte staging; the 1x1 conv's weight DMA): C-ABI rows one float off, leaving exactly those forms
    assert UNALIGNED_ROWS["tc8_w1_t49_small"] == {"eval": "static", "wgrad0": "16b"} and paths_of(ROW["tc8_w1_t49_small"])["eval"] == "small"
    assert all(paths_of(ROW[n])["wgrad0"] == "lds" for n in UNALIGNED_ROWS)
    assert {(paths_of(ROW[n])["fwd"].split("-")[0], paths_of(ROW[n])["bwd"]) for n in UNALIGNED_ROWS} >= {("phases", "lazy"), ("chain", "chain")}
    # the fused eval kernel's unit count: more than kFusedMaxLayers = 32 BN units with nothing else in the way
    deep = [r for r in ROWS if 1 + sum(3 if a != b else 2 for a, b in zip(channels_of(r)[:-1], channels_of(r)[1:])) > 32]
    assert deep and all(paths_of(r)["eval"] == "layers" and paths_of(r)["convs"] == "mfma" for r in deep) and deep[0][0] in UNALIGNED_ROWS
    # the early shortcut data gradient of the per-layer backward (as launched): wide nets on either side of 64 frames, a narrow net, and
    # a shortcut the matrix-core data gradient does not cover
    chain = [r for r in ROWS if paths_of(r)["bwd"] == "chain"]
    assert {(channels_of(r)[-1] > 48, paths_of(r)["shortcut"]) for r in chain} == {(True, "late"), (True, "early"), (False, "early"), (False, "late")}
    wide = {r[4]: paths_of(r)["shortcut"] for r in chain if channels_of(r) == [32, 48, 64, 96]}
    assert wide == {63: "late", 64: "early", 65: "early"}
    # shapes: coefficient counts, frame counts around the 16-position units and 32-position wave groups, pads (4,4) / (3,4), heads
    assert {1, 10, 13, 20, 64} <= {r[3] for r in ROWS} and {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 198, 300} <= {r[4] for r in ROWS}
    assert {2, 35, 46} <= {r[5] for r in ROWS}
    assert any(r[1] == "TCResNet14" and r[2] not in (1.5,) and any(c % 4 for c in channels_of(r)) for r in ROWS)
    assert all(2 <= r[6] <= 9 for r in ROWS) and all(r[4] <= 200 or (r[1], r[2], r[6]) == ("TCResNet8", 1.0, 2) for r in ROWS)
    assert all(r[6] * last_frames(r) >= MIN_BN_POSITIONS for r in ROWS)
    for rows, need in ((STAGED_ROWS, 3), (GUARD_ROWS, 3), (OPTIM_ROWS, 2), (DROPOUT_ROWS, 4)):
        assert len(rows) >= need and all(n in ROW for n in rows)
    assert any(c % 2 for c in channels_of(ROW[STAGED_ROWS[0]])) and channels_of(ROW[STAGED_ROWS[1]])[-1] > 48 and ROW[STAGED_ROWS[2]][1] == "TCResNet14"


@pytest.mark.parametrize("name", ROW_IDS)
def test_config_row(emu_lib, name):
    check_net_row(emu_lib, ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_IDS)
def test_gpu_config_row(hip_lib, name):
    check_net_row(hip_lib, ROW[name])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    for nc in (47, 100):
        with pytest.raises(T.TcrError) as e:
            T.TCResNet("TCResNet8", R.tcresnet_channels("TCResNet8", 1.0), 40, 49, nc, lib=lib, device=Cm.device_of(lib))
        assert "46-class head" in str(e.value) and str(nc) in str(e.value), str(e.value)
    T.TCResNet("TCResNet8", R.tcresnet_channels("TCResNet8", 1.0), 40, 49, 46, lib=lib, device=Cm.device_of(lib))
    for bad in (dict(in_channels=0), dict(t_in=0), dict(channels=[16, 0, 32, 48])):
        kw = dict(channels=[16, 24, 32, 48], in_channels=40, t_in=49)
        kw.update(bad)
        with pytest.raises(T.TcrError):
            T.TCResNet("TCResNet8", kw["channels"], kw["in_channels"], kw["t_in"], 12, lib=lib, device=Cm.device_of(lib))


def test_refusals(emu_lib):
    check_refusals(emu_lib)


# ---- writes stay inside what the API declares ------------------------------------------------------------------------------------------
GUARD = 4096                # floats on either side of every buffer a call writes (a multiple of 64: the alignment stays)
PATTERN = 0x5A5AA5A5        # as a float ~ 1.5e16: finite, so a value READ from a guard would also wreck the parity below


class Guarded:
    """A device buffer of n floats between two guard regions filled with PATTERN."""

    def __init__(self, lib, n, shift=0):
        self.n, self.lo = int(n), GUARD + int(shift)            # shift: floats the body starts behind the aligned position
        self.buf = torch.full((self.n + 2 * GUARD + 4,), PATTERN, dtype=torch.int32, device=Cm.device_of(lib))
        assert self.buf.data_ptr() % 64 == 0
        self.body = self.buf.view(torch.float32)[self.lo:self.lo + self.n]

    def ptr(self):
        return self.body.data_ptr()

    def intact(self):
        return bool((self.buf[:self.lo] == PATTERN).all()) and bool((self.buf[self.lo + self.n:] == PATTERN).all())


def check_guards(lib, row):
    """tcr_net_forward_infer / _forward_train / _backward called through the C ABI with every written buffer exactly as large as
    declared (the workspace: tcr_net_workspace_bytes, passed as its size) and guard regions around each: the guards keep their pattern,
    the results are bitwise the engine's own (whose workspaces the allocator pads), and the gradient arena -- handed over full of the
    pattern -- comes back exactly zero outside the tensors tcr_net_tensor_info lists (the backward's first launch zero-fills the whole
    arena: net.cpp, BwdPrologueArgs::zero)."""
    name, _, _, _, _, nc, batch, _ = row
    st = row_setup(row)
    net = make_row_net(lib, row, st)
    feat = planar(lib, st["x"])
    lab = Cm.to_dev(lib, st["labels"])
    want_eval = [v.clone() for v in net.forward_infer(feat, want_ranges=True)]
    stats0 = net.stats.clone()
    want_train = [v.clone() for v in net.forward_train(feat, lab, keep_prob=1.0)]
    want_grads = net.backward().clone()
    want_stats = net.stats.clone()
    net.stats.copy_(stats0)
    h, stream = net._h, net._stream()
    bufs = {}
    for train in (0, 1):
        nbytes = lib.tcr_net_workspace_bytes(h, batch, train)
        assert nbytes % 4 == 0 and nbytes > 0
        bufs["ws%d" % train] = Guarded(lib, nbytes // 4)
    for k, n in (("logits", batch * nc), ("probs", batch * nc), ("ranges", batch * 2), ("loss", 1), ("grads", net.n_param), ("stats", net.n_stat)):
        bufs[k] = Guarded(lib, n)
    bufs["stats"].body.copy_(stats0)

    def intact(what):
        bad = [k for k, b in bufs.items() if not b.intact()]
        assert not bad, (name, what, "wrote outside", bad)

    ws = bufs["ws0"]
    lib.check(lib.tcr_net_forward_infer(h, net.params.data_ptr(), bufs["stats"].ptr(), feat.data_ptr(), batch, ws.ptr(), ws.n * 4,
                                        bufs["logits"].ptr(), bufs["probs"].ptr(), bufs["ranges"].ptr(), stream), "tcr_net_forward_infer")
    intact("tcr_net_forward_infer")
    for k, w in zip(("logits", "probs", "ranges"), want_eval):
        assert torch.equal(bufs[k].body.view(w.shape), w), (name, "tcr_net_forward_infer", k)
    # A DECLARED size one float short is refused before anything is launched.  (Only the number passed changes: the allocation keeps
    # its full size and its guards, so even a launch could not leave the buffer.)
    rc = lib.tcr_net_forward_infer(h, net.params.data_ptr(), bufs["stats"].ptr(), feat.data_ptr(), batch, ws.ptr(), ws.n * 4 - 4,
                                   bufs["logits"].ptr(), bufs["probs"].ptr(), bufs["ranges"].ptr(), stream)
    assert rc != 0 and b"workspace" in lib.tcr_last_error()
    ws = bufs["ws1"]
    lib.check(lib.tcr_net_forward_train(h, net.params.data_ptr(), bufs["stats"].ptr(), feat.data_ptr(), lab.data_ptr(), batch, batch, 1.0, 0, 0,
                                        0.0, ws.ptr(), ws.n * 4, bufs["logits"].ptr(), bufs["probs"].ptr(), bufs["loss"].ptr(), stream),
              "tcr_net_forward_train")
    intact("tcr_net_forward_train")
    assert torch.equal(bufs["logits"].body.view(batch, nc), want_train[0]) and torch.equal(bufs["probs"].body.view(batch, nc), want_train[1])
    assert float(bufs["loss"].body[0]) == float(want_train[2]) and torch.equal(bufs["stats"].body, want_stats), (name, "tcr_net_forward_train")
    lib.check(lib.tcr_net_backward(h, net.params.data_ptr(), feat.data_ptr(), batch, ws.ptr(), ws.n * 4, bufs["grads"].ptr(), stream),
              "tcr_net_backward")
    intact("tcr_net_backward")
    got = bufs["grads"].body
    assert torch.equal(got, want_grads), (name, "tcr_net_backward", float((got - want_grads).abs().max()))
    pads = torch.ones(net.n_param, dtype=torch.bool)
    for ti in net.tensors.values():
        if ti.arena == 0:
            pads[ti.offset:ti.offset + ti.size] = False
    assert int(pads.sum()) >= 64 and not bool(got.cpu()[pads].any()), (name, "gradient arena not zero outside its tensors")


@pytest.mark.parametrize("name", GUARD_ROWS)
def test_writes_stay_inside_declared_buffers(emu_lib, name):
    check_guards(emu_lib, ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GUARD_ROWS)
def test_gpu_writes_stay_inside_declared_buffers(hip_lib, name):
    check_guards(hip_lib, ROW[name])


def check_unaligned(lib, name):
    """Every pointer of tcr_net_forward_infer / _forward_train / _backward -- parameters, statistics, features, labels, workspace,
    outputs, gradients -- one float behind a 16-byte boundary (a C-ABI caller owes the library 4-byte alignment only): against the
    oracle with the row's tolerances, guards intact, and on the emulator the forms that need 16-byte operands not launched (the
    small-batch eval kernel's weight DMA, the LDS-staged first filter gradient); everything else takes the row's paths."""
    row = ROW[name]
    _, _, _, _, _, nc, batch, _ = row
    st = row_setup(row)
    net = make_row_net(lib, row, st)
    h, stream = net._h, net._stream()
    bufs = {k: Guarded(lib, n, 1) for k, n in (("params", net.n_param), ("stats", net.n_stat), ("grads", net.n_param), ("logits", batch * nc),
                                               ("probs", batch * nc), ("ranges", batch * 2), ("loss", 1), ("labels", batch * nc),
                                               ("ws0", lib.tcr_net_workspace_bytes(h, batch, 0) // 4), ("ws1", lib.tcr_net_workspace_bytes(h, batch, 1) // 4))}
    feat0 = planar(lib, st["x"])
    bufs["feat"] = Guarded(lib, feat0.numel(), 1)
    for k, src in (("params", net.params), ("stats", net.stats), ("feat", feat0.reshape(-1)), ("labels", Cm.to_dev(lib, st["labels"]).reshape(-1))):
        bufs[k].body.copy_(src)
    assert all(b.ptr() % 16 == 4 for b in bufs.values())
    P = {k: b.ptr() for k, b in bufs.items()}

    def intact(what):
        bad = [k for k, b in bufs.items() if not b.intact()]
        assert not bad, (name, what, "wrote outside", bad)

    want = dict(paths_of(row))
    want.update(UNALIGNED_ROWS[name])
    errs = {}
    with Log(lib) as g:
        lib.check(lib.tcr_net_forward_infer(h, P["params"], P["stats"], P["feat"], batch, P["ws0"], bufs["ws0"].n * 4, P["logits"], P["probs"],
                                            P["ranges"], stream), "tcr_net_forward_infer")
    intact("tcr_net_forward_infer")
    if lib.kind == "emu":
        assert eval_family(g) == want["eval"], (name, "eval ran", eval_family(g))
    for k, tol, shape in (("logits", Cm.LOGIT_TOL, (batch, nc)), ("probs", PROB_TOL, (batch, nc)), ("ranges", PROB_TOL, (batch, 2))):
        errs["eval_" + k] = float(np.abs(bufs[k].body.view(shape).cpu().numpy() - st["ev"][k]).max())
        assert errs["eval_" + k] < tol, (name, "unaligned eval", k, errs)
    with Log(lib) as gf:
        lib.check(lib.tcr_net_forward_train(h, P["params"], P["stats"], P["feat"], P["labels"], batch, batch, 1.0, 0, 0, 0.0, P["ws1"],
                                            bufs["ws1"].n * 4, P["logits"], P["probs"], P["loss"], stream), "tcr_net_forward_train")
    intact("tcr_net_forward_train")
    with Log(lib) as gb:
        lib.check(lib.tcr_net_backward(h, P["params"], P["feat"], batch, P["ws1"], bufs["ws1"].n * 4, P["grads"], stream), "tcr_net_backward")
    intact("tcr_net_backward")
    if lib.kind == "emu":
        fam = train_fwd_families(gf)
        fam.update(bwd_families(gb))
        for k, v in fam.items():
            assert want.get(k, v) == v, (name, "unaligned", k, "expected", want[k], "ran", v)
    errs["train_logits"] = float(np.abs(bufs["logits"].body.view(batch, nc).cpu().numpy() - st["tr"]["logits"]).max())
    errs["loss"] = abs(float(bufs["loss"].body[0]) / batch - st["loss"])
    assert errs["train_logits"] < Cm.LOGIT_TOL and errs["loss"] < 1e-4, (name, "unaligned train", errs)
    got, worst = bufs["grads"].body.cpu().numpy().astype(np.float64), 0.0
    for k, ref in st["grads"].items():
        ti = net.tensors[k]
        e = float(np.abs(got[ti.offset:ti.offset + ti.size].reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-3))
        worst = max(worst, e)
        assert e < GRAD_RTOL, (name, "unaligned", k, e)
    errs["grads"] = worst
    stats = bufs["stats"].body.cpu().numpy()
    for k, ref in st["tr"]["new_stats"].items():
        ti = net.tensors[k]
        assert float(np.abs(stats[ti.offset:ti.offset + ti.size] - ref).max()) < STAT_TOL * max(1.0, np.abs(ref).max()), (name, "unaligned", k)
    print(name, "unaligned", errs)
    return errs


@pytest.mark.parametrize("name", list(UNALIGNED_ROWS))
def test_pointers_one_float_off(emu_lib, name):
    check_unaligned(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNALIGNED_ROWS))
def test_gpu_pointers_one_float_off(hip_lib, name):
    check_unaligned(hip_lib, name)


# ---- the detection stack on a non-flagship net -------------------------------------------------------------------------------------------
def check_detection_stack(lib, n_streams, tmp_path):
    """TCResNet8 at width 0.75 on 13 coefficients behind a 30 ms / 20 ms front-end over 1.5 s clips (74 frames; the per-layer eval
    kernels, VALU first conv): a frozen artifact's streaming pushes are bitwise forward_infer of the same windows, its scan bitwise
    the pushes (stream.hip and scan.hip had met TCResNet8-1.0 only among the TC-ResNets)."""
    from tcresnet_amd import deploy
    from tests import test_scan as TSc
    from tests import test_streaming as TSt
    fe = Cm.make_frontend(lib, 480, 320, num_mfccs=13, clip_ms=1500)
    assert (fe.n_frames, fe.n_coef) == (74, 13)
    arch = R.make_tcresnet("TCResNet8", 0.75, in_channels=13)
    p, s = R.init_params(arch, 0)
    R.randomize_bn(arch, p, s, 1)
    net = Cm.make_net(lib, "TCResNet8", 0.75, fe.n_frames, p, s, in_channels=13)
    meta = {"format": deploy.FORMAT, "model": "TCResNet8Model", "family": "tcresnet", "scope": net.scope, "channels": net.channels,
            "num_classes": net.num_classes, "include_preprocess": True, "height": net.t_in, "width": net.in_channels, "channels_in": 1,
            "bn_decay": float(net.cfg.bn_decay), "bn_eps": float(net.cfg.bn_eps),
            "inputs": [{"name": "input/audio/before_preprocessing", "shape": [1, fe.n_samples, 1]}],
            "output": {"name": "output/softmax", "shape": [1, net.num_classes]},
            "frontend": {"sample_rate": 16000, "clip_duration_ms": 1500, "window_size_samples": 480, "window_stride_samples": 320,
                         "num_mel_bins": 64, "num_mfccs": 13, "lower_edge_hertz": 80.0, "upper_edge_hertz": 7600.0, "method": "mfcc"}}
    consts = {k: v for k, v in net.state_dict().items() if k.endswith("/weights")}
    consts["__folded_batch_norm__"] = net.fold_bn().cpu().numpy()
    path = deploy.FrozenModel(meta, consts, lib=lib, device=Cm.device_of(lib)).save(str(tmp_path / "kws13.npz"))
    model = deploy.FrozenModel.load(path, lib=lib, device=Cm.device_of(lib))
    assert model.frontend.n_frames == 74 and model.engine.channels == [12, 18, 24, 36]
    k, steps = 3, 5
    det = model.streaming(n_streams, frames_per_step=k, min_count=1)
    clips = TSt.Clips(lib, n_streams, fe.n_samples)
    rng = np.random.RandomState(4)
    for i in range(steps):
        x = Cm.to_dev(lib, rng.uniform(-1, 1, (n_streams, k * fe.cfg.hop)) * rng.uniform(0.01, 0.6, (n_streams, 1)))
        idx = [1] if i == 3 else ()
        if idx:
            det.reset(idx)
        out = det.push(x)
        feat = fe(clips.step(x, idx))
        assert torch.equal(det.window(), feat), (i, "window != the offline front-end")
        lo, pr = net.forward_infer(feat)
        assert torch.equal(out.logits, lo) and torch.equal(out.probs, pr), (i, float((out.logits - lo).abs().max()))
    want = R.forward(arch, p, s, fe.reference_view(feat)[..., 0].cpu().numpy().astype(np.float64), False)["logits"]
    assert float(np.abs(out.logits.cpu().numpy() - want).max()) < Cm.LOGIT_TOL
    step_ms = 1000.0 * k * fe.cfg.hop / 16000
    dkw = dict(average_window_ms=3 * step_ms, min_count=2, detection_threshold=0.0, suppression_ms=4 * step_ms)
    audio = Cm.to_dev(lib, TSt.segment_audio(n_streams, 11 * k * fe.cfg.hop, 11))
    pushes = TSc.pushed(model.streaming(n_streams, frames_per_step=k, **dkw), audio)
    TSc.assert_bitwise(model.scanner(frames_per_step=k, **dkw).scan(audio), pushes)
    TSc.assert_bitwise(model.scanner(frames_per_step=k, max_windows=4, **dkw).scan(audio), pushes)


def test_detection_stack_on_a_non_flagship_net(emu_lib, tmp_path):
    check_detection_stack(emu_lib, 2, tmp_path)


@pytest.mark.gpu
def test_gpu_detection_stack_on_a_non_flagship_net(hip_lib, tmp_path):
    check_detection_stack(hip_lib, 96, tmp_path)
