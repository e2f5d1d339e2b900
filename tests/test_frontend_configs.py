"""The MFCC front-end across its configuration space: sample rates, clip lengths, windows, hops, filterbanks, coefficient counts and
methods away from the two reference framings, every kernel family per row, against the float64 oracle (oracle/numpy_ref.py); the plan
tables' invariants on the host; streaming / scanning at other framings; the launchers' batch and pointer edges.
Emulator (`-m "not gpu"`) and MI355X (`-m gpu`, the same rows at batches that fill the persistent grid more than once)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from tests import common as Cm

DEPLOY_TOL = 2e-5          # the float64 deploy kernel: float32 rounding on the way out (tests/common.py::check_frontend_edges)
MATRIX_TOL = 1e-6          # mel / DCT matrices read back from the plan
# (the log_mel_spectrogram preprocessor takes the MAGNITUDE spectrum, datasets/preprocessors.py:161-169 of the reference)
METHODS = {"mfcc": R.mfcc, "log_mel_spectrogram": lambda w, c: R.log_mel_spectrogram(w, c, False), "mfcc_deploy": R.mfcc_deploy}

# (id, sample_rate, clip_ms, win, hop, lower_hz, upper_hz, num_mfccs, method, kernel expected to run)
#   pk3: frontend_pk3_kernel (three waves per SIMD; the default where it applies)      pk: frontend_pk_kernel (two waves; what a
#   filterbank of more than mel_items_fast = 96 items, or at nfft 1024 of more than three items in a segment, falls through to)
#   general: frontend_kernel (any even window, any hop / clip parity)                   f64/<k>: the float64 deploy kernel, and <k> with
#   TCR_TUNE_DEPLOY_F32 set.  Item counts come from the plan (test_plan_tables_*); clip_ms are exact in binary where fractional.
ROWS = [
    # ---- the six packed instances (NC, QV) of both packed kernels
    ("pk3_512_10_ref4020",   16000, 1000, 640, 320, 80.0, 7600.0, 40, "mfcc", "pk3"),
    ("pk3_256_15_ref3010",   16000, 1000, 480, 160, 80.0, 7600.0, 40, "mfcc", "pk3"),
    ("pk3_256_10_8k_nyq_c1", 8000, 1000, 320, 160, 0.0, 4000.0, 1, "mfcc", "pk3"),
    ("pk3_256_16_tel_c17",   16000, 1000, 512, 256, 300.0, 3400.0, 17, "mfcc", "pk3"),            # (16000 - 512) % 256 = 128
    ("pk3_512_16_lo_c16",    16000, 1000, 1024, 512, 20.0, 4000.0, 16, "mfcc", "pk3"),            # (16000 - 1024) % 512 = 128
    ("pk3_512_15_32k_c64",   32000, 1000, 960, 480, 2000.0, 8000.0, 64, "mfcc", "pk3"),           # 65 frames, (32000 - 960) % 480 = 320
    ("pk3_512_15_logmel",    16000, 1000, 960, 320, 80.0, 7600.0, 40, "log_mel_spectrogram", "pk3"),
    ("pk3_256_16_logmel",    16000, 1000, 512, 128, 20.0, 4000.0, 40, "log_mel_spectrogram", "pk3"),
    ("pk3_256_10_8k_logmel", 8000, 1000, 320, 160, 20.0, 4000.0, 40, "log_mel_spectrogram", "pk3"),
    ("pk3_512_10_96_items",  16000, 1000, 640, 320, 0.0, 8000.0, 40, "mfcc", "pk3"),              # exactly mel_items_fast items: no empty slot
    ("pk3_256_16_44k_4seg",  44100, 500, 512, 256, 0.0, 22050.0, 40, "mfcc", "pk3"),              # nfft 512, a segment of four items (log phase loop)
    ("pk3_512_10_hi_band",   16000, 1000, 640, 320, 2000.0, 8000.0, 40, "mfcc", "pk3"),
    # ---- packed windows whose filterbank pk3 declines
    ("pk_512_15_99_items",   32000, 1000, 960, 480, 0.0, 16000.0, 40, "mfcc", "pk"),              # 99 items, four in a segment: slow-path items
    ("pk_512_16_97_items",   32000, 500, 1024, 512, 80.0, 16000.0, 17, "log_mel_spectrogram", "pk"),  # 97 items, <= 3 per segment
    ("pk_512_10_4_per_seg",  48000, 250, 640, 320, 80.0, 22800.0, 40, "mfcc", "pk"),              # 96 items, but four in a segment
    # ---- the general kernel: windows outside the instances, odd hop, odd clip
    ("gen_400_160",          16000, 1000, 400, 160, 80.0, 7600.0, 40, "mfcc", "general"),
    ("gen_258_100_c16",      16000, 1000, 258, 100, 20.0, 4000.0, 16, "mfcc", "general"),         # (16000 - 258) % 100 = 42
    ("gen_800_200_logmel",   16000, 1000, 800, 200, 0.0, 8000.0, 40, "log_mel_spectrogram", "general"),
    ("gen_odd_hop",          16000, 1000, 640, 321, 80.0, 7600.0, 40, "mfcc", "general"),
    ("gen_odd_clip",         16000, 1000.0625, 640, 320, 80.0, 7600.0, 40, "mfcc", "general"),     # 16001 samples
    ("gen_22k_442_221_c64",  22050, 1000, 442, 221, 20.0, 4000.0, 64, "mfcc", "general"),
    # ---- clip lengths: 1 frame; 63 / 64 / 65 frames per utterance
    ("pk3_512_1_frame",      16000, 40, 640, 320, 80.0, 7600.0, 40, "mfcc", "pk3"),
    ("pk3_256_1_frame",      16000, 30, 480, 160, 300.0, 3400.0, 17, "mfcc", "pk3"),
    ("gen_1_frame",          16000, 25, 400, 160, 80.0, 7600.0, 40, "mfcc", "general"),
    ("pk3_512_63_frames",    16000, 1280, 640, 320, 80.0, 7600.0, 40, "mfcc", "pk3"),
    ("pk3_512_64_frames",    16000, 1300, 640, 320, 20.0, 4000.0, 16, "mfcc", "pk3"),
    ("pk3_512_65_frames",    16000, 1320, 640, 320, 80.0, 7600.0, 1, "mfcc", "pk3"),
    ("pk3_256_63_frames",    16000, 650, 480, 160, 80.0, 7600.0, 64, "mfcc", "pk3"),
    ("pk3_256_64_frames",    16000, 660, 480, 160, 0.0, 8000.0, 40, "log_mel_spectrogram", "pk3"),
    ("pk3_256_65_frames",    16000, 675, 480, 160, 80.0, 7600.0, 40, "mfcc", "pk3"),              # 10800 samples: (10800 - 480) % 160 = 80
    ("gen_64_frames",        16000, 655, 400, 160, 2000.0, 8000.0, 17, "mfcc", "general"),
    # ---- the deploy path: the float64 kernel, and the float32 kernels behind TCR_TUNE_DEPLOY_F32
    ("f64_ref4020",          16000, 1000, 640, 320, 80.0, 7600.0, 40, "mfcc_deploy", "f64/pk3"),
    ("f64_8k_c16",           8000, 1000, 320, 160, 20.0, 4000.0, 16, "mfcc_deploy", "f64/pk3"),
    ("f64_400_tel_c17",      16000, 1000, 400, 160, 300.0, 3400.0, 17, "mfcc_deploy", "f64/general"),
    ("f64_32k_nyq_c64",      32000, 1000, 960, 480, 0.0, 16000.0, 64, "mfcc_deploy", "f64/pk"),
    ("f64_512_hi_c1",        16000, 1000, 512, 256, 2000.0, 8000.0, 1, "mfcc_deploy", "f64/pk3"),
    ("f64_odd_hop_1_frame",  16000, 64, 1024, 333, 80.0, 7600.0, 40, "mfcc_deploy", "f64/general"),
]
ROW_IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}
PACKED_FRAMES = 3 * 64          # frames of one persistent workgroup slot set per CU (pk3: three workgroups per CU, chunks of <= 64 frames)


def build(lib, row):
    _, sr, clip_ms, win, hop, lo, hi, nm, method, _ = row
    fe = Cm.make_frontend(lib, win, hop, num_mfccs=nm, method=method, sample_rate=sr, clip_ms=clip_ms, lower_hz=lo, upper_hz=hi)
    ocfg = Cm.oracle_frontend_cfg(sr, clip_ms, win, hop, lo, hi, nm)
    assert (fe.n_samples, fe.n_frames, fe.cfg.nfft) == (ocfg.n_samples, ocfg.n_frames, ocfg.nfft), row
    return fe, ocfg


def device_cus(lib):
    """Compute units the launchers size their persistent grids by: the device's, or what the emulator's runtime stub reports."""
    if lib.kind == "hip":
        return torch.cuda.get_device_properties(0).multi_processor_count
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "hip", "hip_runtime.h")).read()
    m = re.search(r"hipDeviceGetAttribute\(int\* v[^{]*\{ \*v = (\d+);", src)
    assert m, "the emulator's hipDeviceGetAttribute stub no longer states its compute-unit count"
    return int(m.group(1))


def batch_for(lib, n_frames):
    """Emulator: two ordinary rows + the five quiet ones.  GPU: enough utterances for more chunks than the persistent grid has slots."""
    if lib.kind != "hip":
        return 7
    return -(-(PACKED_FRAMES * device_cus(lib) * 5 // 4) // n_frames) + 3


def tiled(lib, base, batch):
    """`batch` utterances on the device cycling through the rows of `base`, and the row index of each."""
    idx = np.arange(batch) % base.shape[0]
    return Cm.to_dev(lib, base)[torch.as_tensor(idx, device=Cm.device_of(lib))].contiguous(), idx


def run_arms(lib, fe, wav, knobs=()):
    """The features by the default dispatch, with the two-waves kernel selected (tcr_tune(23, 1)) and with the scalar kernel selected
    (tcr_tune(1, 4)); `knobs`: (id, value) pairs held over all three."""
    out = {}
    try:
        for k, v in knobs:
            lib.tcr_tune(k, v)
        out["default"] = fe(wav).clone()
        try:
            lib.tcr_tune(23, 1)
            out["two_wave"] = fe(wav).clone()
        finally:
            lib.tcr_tune(23, 0)
        try:
            lib.tcr_tune(1, 4)
            out["scalar"] = fe(wav).clone()
        finally:
            lib.tcr_tune(1, 0)
    finally:
        for k, _ in knobs:
            lib.tcr_tune(k, 0)
    return out


def worst_errors(fe, feat, ref, idx):
    """Halo exactly zero; worst |feature - oracle| over the ordinary + quiet rows."""
    f = feat.cpu().numpy()
    h = T._lib.HALO
    assert np.all(f[:, :, :h] == 0) and np.all(f[:, :, h + fe.n_frames:] == 0), "halo not zero"
    got = f[:, :, h:h + fe.n_frames].transpose(0, 2, 1)
    assert got.shape == (len(idx),) + ref.shape[1:], (got.shape, ref.shape)
    assert np.all(np.isfinite(got))
    return float(np.abs(got - ref[idx]).max())


def check_dispatch(arms, kernel, what):
    """Pins the kernel family from the outside: the packed kernels are bitwise each other and order their sums unlike the scalar
    kernel; where the general kernel is what runs, selecting either changes nothing."""
    d, w, s = arms["default"], arms["two_wave"], arms["scalar"]
    assert torch.equal(d, w), (what, "default != two-wave", float((d - w).abs().max()))
    if kernel in ("pk3", "pk"):
        assert not torch.equal(d, s), (what, "the default's bits are the scalar kernel's: a packed kernel was expected to run")
    else:
        assert torch.equal(d, s), (what, "default != scalar on a row of the general kernel", float((d - s).abs().max()))


def check_matrices(fe, ocfg, method):
    mel = fe.mel_matrix().astype(np.float64)
    if method == "mfcc_deploy":
        want = R.deploy_mel_weight_matrix(ocfg)                # (tied to oracle.mfcc_deploy by test_deploy_matrix_is_the_oracles_filterbank)
        dct = np.sqrt(2.0 / 64) * np.cos(np.pi / 64 * np.outer(np.arange(64) + 0.5, np.arange(ocfg.num_mfccs)))
    else:
        want = R.linear_to_mel_weight_matrix(64, ocfg.n_bins, ocfg.sample_rate, ocfg.lower_edge_hertz, ocfg.upper_edge_hertz)
        dct = R.dct2_matrix(64, fe.n_coef)
    e_mel = float(np.abs(mel - want).max())
    assert mel.shape == want.shape and e_mel < MATRIX_TOL, ("mel matrix", e_mel)
    e_dct = float(np.abs(fe.dct_matrix() - dct).max())
    assert e_dct < MATRIX_TOL, ("dct matrix", e_dct)
    return e_mel, e_dct


def check_config_row(lib, row):
    """One row: every arm against the oracle, the dispatch pinned, matrices read back.  Returns {arm: worst error}."""
    name, method, kernel = row[0], row[8], row[9]
    fe, ocfg = build(lib, row)
    base = Cm.config_waveforms(fe.n_samples, 7 if lib.kind != "hip" else 37)
    ref = METHODS[method](base, ocfg)
    if method == "log_mel_spectrogram":
        assert fe.n_coef == 64
    wav, idx = tiled(lib, base, batch_for(lib, fe.n_frames))
    errs = {}
    if method == "mfcc_deploy":
        arms = run_arms(lib, fe, wav)                       # all three: the float64 kernel
        for k, v in arms.items():
            errs["f64_" + k] = worst_errors(fe, v, ref, idx)
        print(name, errs)
        assert max(errs.values()) < DEPLOY_TOL, (name, errs)
        assert torch.equal(arms["default"], arms["two_wave"]) and torch.equal(arms["default"], arms["scalar"]), name
        f32 = run_arms(lib, fe, wav, knobs=((26, 1),))      # the float32 kernels' variant of the deploy filterbank / log floor
        e32 = {"f32_" + k: worst_errors(fe, v, ref, idx) for k, v in f32.items()}
        print(name, e32)
        errs.update(e32)
        assert max(e32.values()) < Cm.MFCC_TOL, (name, e32)
        check_dispatch(f32, kernel.split("/")[1], name)
        assert not torch.equal(f32["default"], arms["default"]), name
    else:
        arms = run_arms(lib, fe, wav)
        for k, v in arms.items():
            errs[k] = worst_errors(fe, v, ref, idx)
        print(name, errs)
        assert max(errs.values()) < Cm.MFCC_TOL, (name, errs)
        check_dispatch(arms, kernel, name)
    errs["mel_matrix"], errs["dct_matrix"] = check_matrices(fe, ocfg, method)
    return errs


def test_deploy_matrix_is_the_oracles_filterbank():
    """oracle.deploy_mel_weight_matrix is what oracle.mfcc_deploy applies: magnitude spectrum @ matrix, log floor, DCT give its features."""
    for name in ("f64_ref4020", "f64_8k_c16", "f64_32k_nyq_c64"):
        _, sr, clip_ms, win, hop, lo, hi, nm, _, _ = ROW[name]
        cfg = Cm.oracle_frontend_cfg(sr, clip_ms, win, hop, lo, hi, nm)
        wav = R.synth_waveforms(2, cfg.n_samples, seed=3)
        mag = np.abs(np.fft.rfft(R.frame_signal(wav.astype(np.float64), win, hop) * R.hann_periodic(win), n=cfg.nfft, axis=-1))
        dct = np.sqrt(2.0 / 64) * np.cos(np.pi / 64 * np.outer(np.arange(64) + 0.5, np.arange(nm)))
        got = np.log(np.maximum(mag @ R.deploy_mel_weight_matrix(cfg), 1e-12)) @ dct
        assert np.abs(got - R.mfcc_deploy(wav, cfg)).max() < 1e-9


def test_rows_take_every_listed_branch():
    """The table covers what the issue lists (a row that leaves would take its branch with it)."""
    wins = {(r[3], r[9].split("/")[-1]) for r in ROWS}
    for w in (640, 480, 960, 1024, 512, 320):
        assert (w, "pk3") in wins
    assert {(960, "pk"), (1024, "pk"), (640, "pk"), (400, "general"), (258, "general"), (800, "general")} <= wins
    assert {8000, 32000} <= {r[1] for r in ROWS} and any(r[4] % 2 for r in ROWS)
    assert {(20.0, 4000.0), (300.0, 3400.0), (2000.0, 8000.0), (0.0, 8000.0), (0.0, 4000.0), (0.0, 16000.0)} <= {(r[5], r[6]) for r in ROWS}
    assert {1, 16, 17, 64} <= {r[7] for r in ROWS} and {r[8] for r in ROWS} == set(METHODS)
    frames = {1 + (int(r[1] * r[2] / 1000) - r[3]) // r[4] for r in ROWS}
    assert {1, 63, 64, 65} <= frames
    assert any((int(r[1] * r[2] / 1000) - r[3]) % r[4] for r in ROWS) and any(int(r[1] * r[2] / 1000) % 2 for r in ROWS)
    assert len(set(ROW_IDS)) == len(ROWS)


# ---- 1 + 2: the sweep, every kernel family per row ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_IDS)
def test_config_row(emu_lib, name):
    check_config_row(emu_lib, ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_IDS)
def test_gpu_config_row(hip_lib, name):
    check_config_row(hip_lib, ROW[name])


# ---- 3: plan tables, host only --------------------------------------------------------------------------------------------------------
K_MEL_ITEMS_MAX = 192


def plan_layout(win, nfft, n_mel=64):
    """frontend_plan.h::frontend_plan_layout restated: word offsets of the tables, each rounded up to 16 words."""
    nc, nbins, nseg = nfft // 2, nfft // 2 + 1, n_mel + 1
    item_bins, trips = (8, 3) if nc == 512 else (4, 6)
    nfast = trips * (nc // 16)
    off, o = {}, 0
    for key, words in (("window", win), ("tw256", 512), ("tw_combine", 512), ("tw_real", 2 * (nc // 2 + 1)), ("seg_start", nseg + 1),
                       ("wud", 2 * nbins), ("dcth", n_mel * (n_mel // 2)), ("mel_items", K_MEL_ITEMS_MAX), ("mel_ifirst", nseg + 2),
                       ("mel_wit", 2 * item_bins * nfast), ("window_sgn", win), ("dct_tab", (n_mel // 16) * (n_mel // 4) * 64)):
        off[key] = o
        o += (words + 15) // 16 * 16
    off.update(words=o, nc=nc, nbins=nbins, nseg=nseg, item_bins=item_bins, nfast=nfast)
    return off


def host_plan(lib, sr, win, lo, hi, method=0, n_mel=64, nfft=None):
    """(cfg, plan words as float32, layout) or (None, message) when the library refuses the configuration."""
    cfg = T._lib.FrontendCfg(int(sr), int(sr), int(win), int(win) // 2, 0, 0, n_mel, min(40, n_mel), float(lo), float(hi), method)
    if nfft is None:
        if lib.tcr_frontend_resolve(C.byref(cfg)) != 0:
            return None, lib.tcr_last_error().decode()
    else:
        cfg.nfft, cfg.n_frames = nfft, 1 + (cfg.n_samples - cfg.win) // cfg.hop      # (what resolve would fill in, without its checks)
    L = plan_layout(win, cfg.nfft, n_mel)
    nbytes = lib.tcr_frontend_plan_bytes(C.byref(cfg))
    assert nbytes == 4 * L["words"], (nbytes, L["words"])
    plan = np.zeros(nbytes // 4, np.float32)
    if lib.tcr_frontend_plan_init(C.byref(cfg), plan.ctypes.data) != 0:
        return None, lib.tcr_last_error().decode()
    return (cfg, plan, L), ""


def check_plan_tables(cfg, plan, L):
    """The invariants the packed kernels rely on.  Returns (number of items, most items in a segment, number of fast slots that share
    their trip and start class -- read base mod 32, mod 16 at 16 lanes per frame -- with an earlier slot: zero when the matching of
    frontend_plan.cpp placed every item, positive when items were left over and took a free slot at their natural base)."""
    pi = plan.view(np.int32)
    nseg, nbins, ib, nfast = L["nseg"], L["nbins"], L["item_bins"], L["nfast"]
    seg = pi[L["seg_start"]:L["seg_start"] + nseg + 1].astype(np.int64)
    ifirst = pi[L["mel_ifirst"]:L["mel_ifirst"] + nseg + 2].astype(np.int64)
    items = pi[L["mel_items"]:L["mel_items"] + K_MEL_ITEMS_MAX].astype(np.int64)
    wud = plan[L["wud"]:L["wud"] + 2 * nbins].reshape(nbins, 2)
    wit = plan[L["mel_wit"]:L["mel_wit"] + 2 * ib * nfast].reshape(ib, nfast, 2)
    assert np.all(np.diff(seg) >= 0) and 0 <= seg[0] and seg[nseg] <= nbins
    # the segments' items in logical order: what ifirst promises
    n = int(ifirst[nseg])
    assert ifirst[0] == 0 and ifirst[nseg + 1] == n and np.all(np.diff(ifirst) >= 0) and n <= K_MEL_ITEMS_MAX
    want = []                                               # logical item -> (first bin, bins, segment)
    for j in range(nseg):
        ks = list(range(int(seg[j]), int(seg[j + 1]), ib))
        assert ifirst[j + 1] - ifirst[j] == len(ks), (j, ifirst[j], ifirst[j + 1], ks)
        want += [(k, min(ib, int(seg[j + 1]) - k), j) for k in ks]
    assert len(want) == n
    cover = np.zeros(nbins, np.int64)
    lpf = L["nc"] // 16                                     # lanes per frame = slots per trip
    classes, taken, shared = (32 if lpf >= 32 else 16), set(), 0
    dummy = (nfast if n <= nfast else K_MEL_ITEMS_MAX)
    seen = []
    for slot in range(nfast):
        d = int(items[slot])
        base, nb, sg, logical = d & 1023, (d >> 10) & 15, (d >> 14) & 127, (d >> 21) & 255
        if nb == 0:                                         # an empty slot: the dummy cell, all-zero slopes
            assert d == dummy << 21, (slot, hex(d), dummy)
            assert np.all(wit[:, slot] == 0)
            continue
        assert logical < min(n, nfast), (slot, logical, n)
        k0, nb_want, j = want[logical]
        assert (nb, sg) == (nb_want, j), (slot, logical, nb, sg, want[logical])
        assert 0 <= base <= k0 and k0 + nb <= base + ib, (slot, "read base", base, k0, nb)      # the item lies inside the trip's reads
        for b in range(ib):
            inside = k0 <= base + b < k0 + nb
            exp = wud[base + b] if inside else np.zeros(2, np.float32)
            assert np.array_equal(wit[b, slot], exp), (slot, b, wit[b, slot], exp)
        cover[k0:k0 + nb] += 1
        seen.append(logical)
        shared += (slot // lpf, base % classes) in taken
        taken.add((slot // lpf, base % classes))
    assert sorted(seen) == list(range(min(n, nfast))), "logical indices of the used slots are not a permutation"
    for i in range(nfast, n):                               # slow path: logical == physical, the true first bin
        d = int(items[i])
        k0, nb, j = want[i]
        assert (d & 1023, (d >> 10) & 15, (d >> 14) & 127, (d >> 21) & 255) == (k0, nb, j, i), (i, hex(d), want[i])
        cover[k0:k0 + nb] += 1
    assert np.all(cover[seg[0]:seg[nseg]] == 1) and cover.sum() == seg[nseg] - seg[0], "a bin outside exactly one item"
    # weights outside the segments are zero: nothing is lost by not reading them
    assert np.all(wud[:seg[0]] == 0) and np.all(wud[seg[nseg]:] == 0)
    per = np.diff(ifirst[:nseg + 1])
    return n, int(per.max()), shared


def plan_grid(seed=20260, count=320):
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        sr = int(rng.choice([8000, 11025, 16000, 22050, 32000, 44100, 48000]))
        win = int(rng.choice([258, 320, 400, 480, 512, 640, 800, 960, 1024]))
        lo = float(rng.choice([0.0, 20.0, 80.0, 300.0, round(rng.uniform(0, sr / 4), 1)]))
        hi = float(rng.choice([sr / 2.0, 3400.0, 4000.0, 7600.0, round(rng.uniform(sr / 8, sr / 2), 1)]))
        if lo < hi <= sr / 2.0 and win <= sr:
            out.append((sr, win, lo, hi, int(rng.randint(0, 3) == 2) * 2))
    return out


def test_plan_tables_invariants(emu_lib):
    """A seeded grid of (sample_rate, nfft, lower, upper), HTK and deploy filterbanks: the item cuts, read bases, slopes per slot,
    logical indices and the dummy slot -- including filterbanks whose matching leaves items unmatched, whose items exceed the unrolled
    trips (slow-path descriptors) and the rows of the sweep."""
    lib = emu_lib
    cases = plan_grid() + [(r[1], r[3], r[5], r[6], 2 if r[8] == "mfcc_deploy" else 0) for r in ROWS]
    over, four, exact, refused, leftover = 0, 0, 0, 0, 0
    for sr, win, lo, hi, method in cases:
        got, msg = host_plan(lib, sr, win, lo, hi, method)
        if got is None:
            assert msg, (sr, win, lo, hi, method)               # a refusal carries its reason
            refused += 1
            continue
        cfg, plan, L = got
        n, per, shared = check_plan_tables(cfg, plan, L)
        leftover += shared > 0
        over += n > L["nfast"]
        exact += n == L["nfast"]
        four += per > 3
    assert refused == 0, refused                                # (every grid point is a valid 64-band configuration)
    assert over >= 3 and four >= 3 and exact >= 1, (over, four, exact)
    assert leftover >= 3, leftover                              # the "takes a free slot at its natural base" branch of the matching
    for win in (640, 480):                                      # ... which the reference filterbanks do not need (91 / 91, 89 / 89 matched)
        (cfg, plan, L), _ = host_plan(lib, 16000, win, 80.0, 7600.0)
        assert check_plan_tables(cfg, plan, L) == ({640: 91, 480: 89}[win], 3, 0)
    # the rows the sweep expects pk3 to decline are the ones whose plan says so.  (frontend_mel_item_count() itself is not exported: that
    # it agrees with mel_ifirst shows in what depends on it -- these rows' dispatch in test_config_row, where pk3 on a filterbank it
    # does not cover misses the oracle, and the streaming refusals' item counts in check_stream_refusals.)
    for r in ROWS:
        if r[8] == "mfcc_deploy":
            continue
        (cfg, plan, L), _ = host_plan(lib, r[1], r[3], r[5], r[6])
        n, per, _ = check_plan_tables(cfg, plan, L)
        declines = n > L["nfast"] or (L["nc"] == 512 and per > 3)
        assert declines == (r[9] == "pk") or r[9] == "general", (r[0], n, per)


def test_plan_refuses_what_it_cannot_hold(emu_lib):
    """More mel-edge segments than the descriptor's 7-bit field, more items than kMelItemsMax: a status and a message, no table."""
    lib = emu_lib
    # (resolve admits 64 bands only, so both are reached past it; the item check comes first in tcr_frontend_plan_init)
    got, msg = host_plan(lib, 16000, 640, 300.0, 3400.0, n_mel=128, nfft=1024)      # ~200 bins in 129 segments: few items
    assert got is None and "129 mel-edge segments do not fit the item descriptor's 7-bit field" in msg, msg
    got, msg = host_plan(lib, 48000, 1024, 0.0, 24000.0, n_mel=256, nfft=1024)      # 513 bins in 257 segments: > 192 items
    assert got is None and "more than 192 work items" in msg, msg
    bad = T._lib.FrontendCfg(16000, 16000, 640, 320, 0, 0, 128, 40, 80.0, 7600.0, 0)
    assert lib.tcr_frontend_resolve(C.byref(bad)) != 0 and "num_mel_bins" in lib.tcr_last_error().decode()
    bad = T._lib.FrontendCfg(16000, 16000, 256, 128, 0, 0, 64, 40, 80.0, 7600.0, 0)
    assert lib.tcr_frontend_resolve(C.byref(bad)) != 0 and "fft_length" in lib.tcr_last_error().decode()
    bad = T._lib.FrontendCfg(8000, 8000, 320, 160, 0, 0, 64, 40, 80.0, 7600.0, 0)
    assert lib.tcr_frontend_resolve(C.byref(bad)) != 0 and "mel edges" in lib.tcr_last_error().decode()


# ---- 4: streaming and scanning away from the reference framings -----------------------------------------------------------------------
STREAM_ROWS = [("8k_320_160", 8000, 320, 160, 80.0, 3800.0, 49), ("16k_512_256", 16000, 512, 256, 80.0, 7600.0, 61),
               ("16k_640_320_lo", 16000, 640, 320, 20.0, 4000.0, 49)]
STREAM_REFUSED = [("odd_hop", 16000, 1000, 640, 321, 80.0, 7600.0, "hop 321"), ("win_400", 16000, 1000, 400, 160, 80.0, 7600.0, "window 400"),
                  # windows pk3 covers (rows pk3_512_15_32k_c64, pk3_512_16_lo_c16), filterbanks it does not: the text names the filterbank
                  ("four_per_segment", 32000, 1000, 960, 480, 0.0, 16000.0, "mel filterbank 0 - 16000 Hz at sample rate 32000|segment of more than 24 bins"),
                  ("97_items", 32000, 1000, 1024, 512, 80.0, 16000.0, "mel filterbank 80 - 16000 Hz at sample rate 32000|97 work items|take 96")]


def stream_setup(lib, sr, win, hop, lo, hi, seed=0):
    fe = Cm.make_frontend(lib, win, hop, sample_rate=sr, lower_hz=lo, upper_hz=hi)
    arch = R.make_tcresnet("TCResNet8", 1.0, in_channels=fe.n_coef)
    p, s = R.init_params(arch, seed)
    R.randomize_bn(arch, p, s, seed + 1)
    return fe, Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef), arch, p, s


def check_stream_row(lib, row, n_streams):
    from tests import test_scan as TSc
    from tests import test_stream_scan as TSS
    from tests import test_streaming as TSt
    _, sr, win, hop, lo, hi, frames = row
    fe, net, arch, p, s = stream_setup(lib, sr, win, hop, lo, hi)
    assert fe.n_frames == frames
    TSt.run_checked(lib, fe, net, arch, p, s, n_streams, 2, 5, {3: [1]})                   # a push == the offline front-end, bitwise
    k = 3
    step_ms = 1000.0 * k * hop / sr
    det = dict(average_window_ms=3 * step_ms, min_count=2, detection_threshold=0.0, suppression_ms=4 * step_ms)
    audio = TSt.segment_audio(n_streams, 14 * k * hop, 11)
    TSc.check_scan_equals_stream(lib, fe, net, audio, k, det=det)                          # a scan == the pushes
    TSS.check_chunks_equal_scan(lib, fe, net, audio, k, [1, 4, 7, 2], det, max_windows=5)  # push_many == the scan


@pytest.mark.parametrize("row", STREAM_ROWS, ids=[r[0] for r in STREAM_ROWS])
def test_stream_scan_other_framings(emu_lib, row):
    check_stream_row(emu_lib, row, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("row", STREAM_ROWS, ids=[r[0] for r in STREAM_ROWS])
def test_gpu_stream_scan_other_framings(hip_lib, row):
    check_stream_row(hip_lib, row, 96)


def check_stream_refusals(lib):
    from tcresnet_amd import scanning as Sc
    from tcresnet_amd import streaming as St
    for _, sr, clip_ms, win, hop, lo, hi, cause in STREAM_REFUSED:
        fe = Cm.make_frontend(lib, win, hop, sample_rate=sr, clip_ms=clip_ms, lower_hz=lo, upper_hz=hi)
        arch = R.make_tcresnet("TCResNet8", 1.0, in_channels=fe.n_coef)
        p, s = R.init_params(arch, 0)
        net = Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef)
        for make in (lambda: St.StreamingDetector(net, fe, 2), lambda: Sc.KeywordScanner(net, fe)):
            with pytest.raises(T.TcrError) as e:
                make()
            msg = str(e.value)
            assert "frontend_pk3_kernel" in msg and all(c in msg for c in cause.split("|")) and "bitwise" in msg, msg
            assert ("window" in msg) == (not cause.startswith("mel filterbank")), msg      # a covered window is not blamed


def test_stream_refuses_what_pk3_declines(emu_lib):
    check_stream_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_stream_refuses_what_pk3_declines(hip_lib):
    check_stream_refusals(hip_lib)


# ---- 5: batch and pointer edges of the launchers ----------------------------------------------------------------------------------------
EDGE_ROWS = ["pk3_512_1_frame", "pk3_256_1_frame", "gen_1_frame"]


def check_batch_edges(lib, name):
    """total_frames 1, 63, 64, 65 and one more than a whole number of chunks over the persistent grid (one-frame clips: batch = frames):
    each against the oracle, on every arm, and rounds = 1 / the maximum bitwise the launcher's own choice."""
    row = ROW[name]
    fe, ocfg = build(lib, row)
    assert fe.n_frames == 1
    base = Cm.config_waveforms(fe.n_samples, 23)
    ref = METHODS[row[8]](base, ocfg)
    cus = device_cus(lib)
    max_rounds = 8 if fe.cfg.nfft == 1024 else 4
    worst = 0.0
    for batch in (1, 63, 64, 65, 3 * cus * 64 + 1, 2 * cus * 64 + 1):
        wav, idx = tiled(lib, base, batch)
        arms = run_arms(lib, fe, wav)
        for k, v in arms.items():
            e = worst_errors(fe, v, ref, idx)
            worst = max(worst, e)
            assert e < Cm.MFCC_TOL, (name, batch, k, e)
        for rounds in (1, max_rounds, 64):                      # (64: clamped to the maximum)
            got = fe(wav, rounds=rounds)
            assert torch.equal(got, arms["default"]), (name, batch, rounds)
        if batch > 1:
            check_dispatch(arms, row[9], (name, batch))
    return worst


@pytest.mark.parametrize("name", EDGE_ROWS)
def test_batch_edges(emu_lib, name):
    check_batch_edges(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_ROWS)
def test_gpu_batch_edges(hip_lib, name):
    check_batch_edges(hip_lib, name)


POINTER_ROWS = ["pk3_512_10_ref4020", "pk3_256_16_tel_c17", "pk_512_10_4_per_seg", "gen_400_160", "gen_odd_clip", "f64_8k_c16"]


def check_pointer_offset(lib, name):
    """A waveform view that starts one float behind an aligned buffer (4- but not 8-byte aligned): the packed kernels' 8-byte loads do
    not apply, the call falls through to the general kernel -- bitwise the aligned result where that kernel (or the float64 one) runs
    anyway, bitwise the scalar arm and within tolerance of the oracle on packed rows."""
    row = ROW[name]
    fe, ocfg = build(lib, row)
    base = Cm.config_waveforms(fe.n_samples, 7)
    ref = METHODS[row[8]](base, ocfg)
    batch = 7 if lib.kind != "hip" else 41
    wav, idx = tiled(lib, base, batch)
    buf = torch.zeros(wav.numel() + 3, dtype=torch.float32, device=wav.device)
    assert buf.data_ptr() % 8 == 0
    off = buf[1:1 + wav.numel()].view(wav.shape)
    off.copy_(wav)
    assert off.data_ptr() % 8 == 4 and off.is_contiguous()
    arms = run_arms(lib, fe, wav)
    for rounds in (1, 3, 64):                                   # (several frames per utterance: chunks of rounds x 8 / 16 frames cut them)
        assert torch.equal(fe(wav, rounds=rounds), arms["default"]), (name, rounds)
    got = fe(off)
    tol = DEPLOY_TOL if row[8] == "mfcc_deploy" else Cm.MFCC_TOL
    e = worst_errors(fe, got, ref, idx)
    assert e < tol, (name, e)
    if row[9] in ("pk3", "pk"):
        assert torch.equal(got, arms["scalar"]), (name, "the offset view did not run the general kernel")
        assert float((got - arms["default"]).abs().max()) < 2 * tol
    else:
        assert torch.equal(got, arms["default"]), (name, float((got - arms["default"]).abs().max()))
    return e


@pytest.mark.parametrize("name", POINTER_ROWS)
def test_pointer_offset(emu_lib, name):
    check_pointer_offset(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", POINTER_ROWS)
def test_gpu_pointer_offset(hip_lib, name):
    check_pointer_offset(hip_lib, name)
