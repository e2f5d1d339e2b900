"""frontend_pk3_kernel with its per-round bookkeeping taken out of the round loop -- frame coordinates stepped from round to round
(frame_next), item descriptors and band ranges in registers for a chunk's rounds, per instance (pk3_round_policy, frontend_pk3.hip) --
gives the bits of frontend_pk_kernel, the two-waves sibling that shares none of that code and is selected in the same process by the
TCR_TUNE_FE_KERNEL knob.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`).

Which instance does what (profiles/fe_carry_kernel_regs.txt):
    4020  640 / 320  <512,10>  49 frames   descriptors and band ranges in REGISTERS, coordinates worked out from the frame number
    3010  480 / 160  <256,15>  98 frames   coordinates CARRIED, item descriptors in registers, band ranges from LDS
    3020  480 / 320  <256,15>  49 frames   (the same instance at an odd frame count: four frames per wave and round, 49 = 12 * 4 + 1)
    2010  320 / 160  <256,10>  99 frames   coordinates carried, item descriptors in registers
    6020  960 / 320  <512,15>  48 frames   everything from LDS, coordinates from the frame number (the instance is at its register ceiling)
    3210  512 / 160  <256,16>  97 frames   item descriptors in registers, coordinates from the frame number
Short clips (1, 2, 3 and 5 frames) run the carried step at FPWV / n_frames >= 1 utterances per round: what the streaming instance
sees at k = 1.  The streaming launcher itself runs one round per chunk until the chunks outnumber three per CU, so a detector's
pushes (test_stream_*) go through the coordinates' full computation; they are here because the instance shares the round body."""
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from tests import common as Cm

KNOB_FE_GRID, KNOB_FE_KERNEL = 13, 23
SENTINEL = -12345.0
PAD = 4096                                                  # sentinel floats on either side of the output

# name -> (window, stride, clip ms)
CONFIGS = {
    "4020": (640, 320, 1000), "3010": (480, 160, 1000), "3020": (480, 320, 1000), "2010": (320, 160, 1000), "6020": (960, 320, 1000),
    "3210": (512, 160, 1000),
    "3010_1frame": (480, 160, 30), "3010_2frames": (480, 160, 40), "3010_3frames": (480, 160, 50), "3010_5frames": (480, 160, 70),
    "4020_2frames": (640, 320, 60),
}
N_FRAMES = {"4020": 49, "3010": 98, "3020": 49, "2010": 99, "6020": 48, "3210": 97, "3010_1frame": 1, "3010_2frames": 2,
            "3010_3frames": 3, "3010_5frames": 5, "4020_2frames": 2}


def make_frontend(lib, name, coef=40):
    win, hop, ms = CONFIGS[name]
    dev = torch.device("cuda" if lib.kind == "hip" else "cpu")
    fe = T.Frontend(sample_rate=16000, clip_duration_ms=ms, window_size_samples=win, window_stride_samples=hop, num_mfccs=coef, lib=lib, device=dev)
    assert fe.n_frames == N_FRAMES[name], (name, fe.n_frames)
    return fe, dev


def waves(batch, n_samples, dev, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((batch, n_samples), generator=g) * 2.0 - 1.0).to(dev)


def run_in_sentinel(fe, wav, rounds, dev):
    """The features, written into the middle of a sentinel-filled buffer; the buffer comes back with them."""
    shape = (wav.shape[0], fe.n_coef, T._lib.padded_len(fe.n_frames))
    n = shape[0] * shape[1] * shape[2]
    big = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    out = fe(wav, out=big[PAD:PAD + n].view(shape), rounds=rounds)
    return out, big


def check(lib, name, batch, rounds_list=(0, 1, 64), grid_cap=0, coef=40):
    fe, dev = make_frontend(lib, name, coef)
    wav = waves(batch, fe.n_samples, dev)
    try:
        lib.tcr_tune(KNOB_FE_KERNEL, 1)                     # frontend_pk_kernel
        want, big = run_in_sentinel(fe, wav, 0, dev)
        assert bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all())
        want = want.clone()
    finally:
        lib.tcr_tune(KNOB_FE_KERNEL, 0)
    assert not bool((want[:, :, T._lib.HALO:T._lib.HALO + fe.n_frames] == SENTINEL).any())
    try:
        lib.tcr_tune(KNOB_FE_GRID, grid_cap)
        for rounds in rounds_list:                          # (0: the launcher's choice; 64: clamped to the maximum, 8 resp. 4)
            got, big = run_in_sentinel(fe, wav, rounds, dev)
            bad = int((got != want).sum())
            print(name, lib.kind, "batch", batch, "rounds", rounds, "grid cap", grid_cap, "mismatches", bad)
            assert torch.equal(got, want), (name, batch, rounds, bad)
            assert bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all()), (name, batch, rounds, "wrote outside the output")
    finally:
        lib.tcr_tune(KNOB_FE_GRID, 0)


WRAP = ["4020", "3010", "3020", "2010", "6020", "3210"]
SHORT = ["3010_1frame", "3010_2frames", "3010_3frames", "3010_5frames", "4020_2frames"]


def check_wrap(lib, name):
    """Batch 5: utterance boundaries inside a round (49 is odd; 98 with four frames per round wraps at another phase) and across rounds."""
    check(lib, name, 5)


def check_clamp(lib, name, batch):
    """total_frames is no multiple of the frames per chunk (batch 1: less than one chunk): the tail lanes of the last chunk sit past
    total_frames - 1; the valid rows are the sibling's, and nothing outside [B][n_coef][T + 8] is written."""
    check(lib, name, batch)


def check_grid_stride(lib, name):
    """Batch 64 on 8 workgroups: every workgroup walks at least three chunks (64 frames at the most), each entered through the full
    computation of the coordinates."""
    assert 64 * N_FRAMES[name] >= 8 * 3 * 64
    check(lib, name, 64, rounds_list=(0, 64), grid_cap=8)


def check_short(lib, name):
    """Clips of 1 .. 5 frames, 213 of them: whole utterances go by per round and wave (FPWV / n_frames of them, then the wrap), over
    several full chunks and a partial one."""
    check(lib, name, 213)


def check_stream(lib, name, k_is_t, coef=40):
    """The streaming instance on S = 3 streams, k = 1 (n_frames = 1 in the kernel) and k = T: once all of a clip has been pushed, the
    window is the sibling's offline features."""
    from tcresnet_amd import streaming as St
    fe, dev = make_frontend(lib, name, coef)
    clips = waves(3, fe.n_samples, dev, seed=11)
    try:
        lib.tcr_tune(KNOB_FE_KERNEL, 1)
        want = fe(clips).clone()
    finally:
        lib.tcr_tune(KNOB_FE_KERNEL, 0)
    arch = R.make_tcresnet("TCResNet8", 1.0, in_channels=fe.n_coef)
    p, s = R.init_params(arch, 0)
    net = Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef)
    k = fe.n_frames if k_is_t else 1
    det = St.StreamingDetector(net, fe, 3, frames_per_step=k, min_count=1)
    step = k * fe.cfg.hop
    pad = -fe.n_samples % step                              # zeros in front: the pushes end on the clip's last sample
    audio = torch.cat([torch.zeros((3, pad), device=dev), clips], dim=1)
    for i in range(audio.shape[1] // step):
        det.push(audio[:, i * step:(i + 1) * step].contiguous())
    got = det.window()
    print(name, lib.kind, "k", k, "mismatches", int((got != want).sum()))
    assert torch.equal(got, want), (name, k)


STREAM_CASES = [("4020", False), ("4020", True), ("3010", False), ("3010", True)]
STREAM_IDS = [f"{n}-{'kT' if t else 'k1'}" for n, t in STREAM_CASES]


@pytest.mark.parametrize("name", WRAP)
def test_wrap(emu_lib, name):
    check_wrap(emu_lib, name)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["4020", "3010", "3020", "6020"])
def test_last_chunk_clamp(emu_lib, name, batch):
    check_clamp(emu_lib, name, batch)


@pytest.mark.parametrize("name", ["4020", "3010", "3020"])
def test_grid_stride(emu_lib, name):
    check_grid_stride(emu_lib, name)


@pytest.mark.parametrize("name", SHORT)
def test_short_clips(emu_lib, name):
    check_short(emu_lib, name)


def test_ten_coefficients(emu_lib):
    check(emu_lib, "4020", 5, coef=10)
    check(emu_lib, "3010", 5, coef=10)


@pytest.mark.parametrize("name,k_is_t", STREAM_CASES, ids=STREAM_IDS)
def test_stream(emu_lib, name, k_is_t):
    check_stream(emu_lib, name, k_is_t)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WRAP)
def test_gpu_wrap(hip_lib, name):
    check_wrap(hip_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["4020", "3010", "3020", "6020"])
def test_gpu_last_chunk_clamp(hip_lib, name, batch):
    check_clamp(hip_lib, name, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["4020", "3010", "3020"])
def test_gpu_grid_stride(hip_lib, name):
    check_grid_stride(hip_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHORT)
def test_gpu_short_clips(hip_lib, name):
    check_short(hip_lib, name)


@pytest.mark.gpu
def test_gpu_ten_coefficients(hip_lib):
    check(hip_lib, "4020", 5, coef=10)
    check(hip_lib, "3010", 5, coef=10)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k_is_t", STREAM_CASES, ids=STREAM_IDS)
def test_gpu_stream(hip_lib, name, k_is_t):
    check_stream(hip_lib, name, k_is_t)
