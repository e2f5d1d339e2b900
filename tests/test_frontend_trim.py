"""The packed front-end kernels keep the bits they had before their first radix-16 pass stopped adding the FFT's zero padding, the sign
of the second pass's odd outputs moved into the recombination and the power spectrum went out in two-address stores: sha256 digests of
the feature tensors against tests/golden/frontend_trim_digests.json, which tests/frontend_trim_digests.py wrote from the commit before
that change (emulator build and MI355X).  Default (three-waves) and two-waves arm, rounds = 1 / the launcher's choice / the maximum,
and the streaming instance of the kernel at k = 1 and k = T.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import json

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from tests import common as Cm
from tests import frontend_trim_digests as D

CASE_IDS = list(D.CASES)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(D.FIXTURE))


def check_offline(lib, golden, name):
    """Both packed arms, three round counts: every tensor has the recorded digest (so they are bitwise each other as well)."""
    want = golden[lib.kind][name]
    fe, dev = D.make_frontend(T, lib, name)
    wav = torch.from_numpy(D.inputs()).to(dev)
    assert wav.shape[0] * fe.n_frames > 2 * 56, "more than one chunk, a partial last one"
    got = {}
    for rounds in (1, 0, 64):                               # (0: the launcher's choice; 64: clamped to the maximum)
        got["default", rounds] = D.case_digests(fe(wav, rounds=rounds))
    try:
        lib.tcr_tune(23, 1)                                 # the two-waves kernel (frontend_pk.hip)
        for rounds in (1, 0, 64):
            got["two_wave", rounds] = D.case_digests(fe(wav, rounds=rounds))
    finally:
        lib.tcr_tune(23, 0)
    print(name, lib.kind, {k: v["all"][:12] for k, v in got.items()}, "want", want["all"][:12])
    for k, v in got.items():
        assert v == want, (name, k, v, want)


def check_stream(lib, golden, name, k_is_t):
    """The streaming instance of the kernel on 2 streams fed the first two input rows: once every sample of the clips has been pushed
    the window is the offline feature rows, digest for digest.  k = 1: one new frame per push (one hop of samples each); k = T: every
    column new, the clip's tail in the second of two pushes."""
    from tcresnet_amd import streaming as St
    want = golden[lib.kind][name]["rows"][:2]
    fe, dev = D.make_frontend(T, lib, name)
    arch = R.make_tcresnet("TCResNet8", 1.0, in_channels=fe.n_coef)
    p, s = R.init_params(arch, 0)
    net = Cm.make_net(lib, "TCResNet8", 1.0, fe.n_frames, p, s, in_channels=fe.n_coef)
    k = fe.n_frames if k_is_t else 1
    det = St.StreamingDetector(net, fe, 2, frames_per_step=k, min_count=1)
    step = k * fe.cfg.hop
    clips = D.inputs()[:2]
    pad = -fe.n_samples % step                              # zeros in front: the pushes end on the clip's last sample
    audio = torch.from_numpy(np.concatenate([np.zeros((2, pad), np.float32), clips], axis=1)).to(dev)
    assert audio.shape[1] % step == 0 and audio.shape[1] // step == (2 if k_is_t else fe.n_samples // fe.cfg.hop)
    for i in range(audio.shape[1] // step):
        det.push(audio[:, i * step:(i + 1) * step].contiguous())
    got = [D.digest(det.window()[i]) for i in range(2)]
    print(name, lib.kind, "k", k, [g[:12] for g in got], "want", [w[:12] for w in want])
    assert got == want, (name, k, got, want)


STREAM_CASES = [("4020_c40", False), ("4020_c40", True), ("4020_c10", False), ("4020_c10", True), ("3010_c40", True), ("4020_logmel", True)]
STREAM_IDS = [f"{n}-{'kT' if t else 'k1'}" for n, t in STREAM_CASES]


def test_fixture_covers_the_cases(golden):
    for kind in ("emu", "hip"):
        assert sorted(golden[kind]) == sorted(D.CASES), kind
        for name in D.CASES:
            assert len(golden[kind][name]["rows"]) == D.BATCH
    x = D.inputs()
    assert x.shape == (D.BATCH, D.N_SAMPLES) and np.abs(x[0]).max() > 0.99 and np.abs(x[1]).max() > 0.99
    assert x[2, 0] == 1.0 and not x[2, 1:].any()


@pytest.mark.parametrize("name", CASE_IDS)
def test_bits_of_the_parent(emu_lib, golden, name):
    check_offline(emu_lib, golden, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_gpu_bits_of_the_parent(hip_lib, golden, name):
    check_offline(hip_lib, golden, name)


@pytest.mark.parametrize("name,k_is_t", STREAM_CASES, ids=STREAM_IDS)
def test_stream_bits_of_the_parent(emu_lib, golden, name, k_is_t):
    check_stream(emu_lib, golden, name, k_is_t)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k_is_t", STREAM_CASES, ids=STREAM_IDS)
def test_gpu_stream_bits_of_the_parent(hip_lib, golden, name, k_is_t):
    check_stream(hip_lib, golden, name, k_is_t)
