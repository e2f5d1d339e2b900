"""Sample-rate conversion on the device (tcr_resample, resampling.Resampler, the command lines' input stage): the filter table against
a float64 restatement of its design, every output against the float64 dot product over the same float32 table within the bound of a
length-P fmaf chain, chunk / push / position invariance bitwise, refusals, and WAV files at 48 / 44.1 kHz end to end.  Emulator
(`-m "not gpu"`) and MI355X (`-m gpu`).

The arithmetic, restated here: in_rate -> out_rate, g = gcd, L = out_rate / g, M = in_rate / g, scale = max(1, M / L), P = 2 ceil(Z scale)
taps per phase; c[phi][p] = fc sinc(fc tau) kaiser(tau / (Z scale)), tau = (p - P / 2 + 1) - phi / L, fc = rolloff / scale, rows divided
by their sums; y[j] = sum_p c[(j M) mod L][p] x[floor(j M / L) - P / 2 + 1 + p], x = 0 outside the signal."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests.test_streaming import frozen_artifact, segment_audio, setup

RATIOS = [(48000, 16000), (44100, 16000), (32000, 16000), (22050, 16000), (8000, 16000), (16000, 8000)]
LMP = [(1, 3, 192), (160, 441, 178), (1, 2, 128), (320, 441, 90), (2, 1, 64), (1, 2, 128)]
Z, BETA, ROLLOFF = 32, 8.6, 0.915


def resampling():
    from tcresnet_amd import resampling as Rs
    return Rs


# ---- the design and the filter, restated ----------------------------------------------------------------------------------------
def kaiser(u, beta):
    return float(np.i0(beta * math.sqrt(1.0 - u * u)) / np.i0(beta)) if abs(u) <= 1.0 else 0.0


def sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def restated_table(in_rate, out_rate, Z=Z):
    """Entry by entry, as the issue states it (float64 Python scalars)."""
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    if L == M:
        return 1, 1, np.ones((1, 1), np.float64)
    scale = max(1.0, M / L)
    P = 2 * math.ceil(Z * scale)
    fc = ROLLOFF / scale
    c = np.zeros((L, P), np.float64)
    for phi in range(L):
        for p in range(P):
            tau = (p - P // 2 + 1) - phi / L
            c[phi, p] = fc * sinc(fc * tau) * kaiser(tau / (Z * scale), BETA)
        c[phi] /= c[phi].sum()
    return L, M, c


def reference(table, L, M, x, n_out, out_first=0):
    """(ref, bound) float64 [n_out] of one decoded signal x (float32 values), outputs out_first .. out_first + n_out - 1 (which may be
    negative): the float64 dot product over the float32 table, and (P + 1) 2^-24 sum_p |c x|, the bound of a length-P fmaf chain.
    Phase by phase: the outputs of one residue share a table row."""
    P = table.shape[1]
    lead = P // 2 - 1 if P > 1 else 0
    c = table.astype(np.float64)
    n_lo = (out_first * M) // L                                                              # floor: the smallest n_j
    n_hi = ((out_first + max(n_out, 1) - 1) * M) // L
    front = lead + max(0, -n_lo)
    back = max(P + M + 1, n_hi + P - len(x) + 1)
    xp = np.concatenate([np.zeros(front), x.astype(np.float64), np.zeros(back)])             # xp[i + front] = x[i]
    win = np.lib.stride_tricks.sliding_window_view(xp, P)
    ref, bound = np.zeros(n_out), np.zeros(n_out)
    for r in range(min(L, n_out)):
        j = out_first + np.arange(r, n_out, L, dtype=np.int64)
        w = win[(j * M) // L + (front - lead)]                                              # x[n_j - lead + p]
        row = c[((out_first + r) * M) % L]
        ref[r::L] = w @ row
        bound[r::L] = (P + 1) * 2.0 ** -24 * (np.abs(w) @ np.abs(row))
    return ref, bound


def decode(a):
    return a.astype(np.float32) * np.float32(1.0 / 32768.0) if a.dtype == np.int16 else a


def check_values(got, table, L, M, x, what, out_first=0):
    """Every output of every row within the chain's bound of the float64 reference; returns the worst error / bound."""
    worst = 0.0
    for s in range(x.shape[0]):
        ref, bound = reference(table, L, M, decode(x[s]), got.shape[1], out_first)
        err = np.abs(got[s].astype(np.float64) - ref)
        bad = err > bound
        assert not bad.any(), (what, s, int(bad.sum()), int(np.flatnonzero(bad)[0]), float(err[bad].max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    return worst


def dev_tensor(lib, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(Cm.device_of(lib))


def make(lib, in_rate, out_rate, S, dtype, channels=1):
    return resampling().Resampler(in_rate, out_rate, S, device=Cm.device_of(lib), dtype=dtype, channels=channels, lib=lib)


def noise(rng, S, n, dtype):
    if dtype == torch.int16:
        return rng.randint(-32768, 32768, size=(S, n)).astype(np.int16)
    return rng.uniform(-1, 1, size=(S, n)).astype(np.float32)


# ---- 1. the table (CPU only) ----------------------------------------------------------------------------------------------------
def check_table_equals_restatement(rates, lmp, zero_crossings=Z):
    L, M, tab = resampling().design_table(*rates, zero_crossings=zero_crossings)
    rL, rM, ref = restated_table(*rates, Z=zero_crossings)
    P = tab.shape[1]
    assert (L, M, P) == lmp == (rL, rM, ref.shape[1]) and tab.dtype == np.float32 and tab.shape == (L, P)
    want = ref.astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(tab - want) <= ulp), float(np.abs(tab - want).max())
    assert np.abs(tab.astype(np.float64).sum(axis=1) - 1.0).max() <= P * 2.0 ** -24


@pytest.mark.parametrize("rates,lmp", list(zip(RATIOS, LMP)))
def test_table_equals_restatement(rates, lmp):
    check_table_equals_restatement(rates, lmp)


def check_table_quality(rates):
    """The prototype rebuilt from the float32 table, h[(p - P / 2 + 1) L - phi] = c[phi][p], gain / L: within +-0.001 dB up to 0.80
    of the lower rate's Nyquist, at most -80 dB from that Nyquist upwards."""
    L, M, tab = resampling().design_table(*rates)
    P = tab.shape[1]
    h = np.zeros(P * L + L, np.float64)
    off = (P // 2 - 1) * L + L - 1                               # index of the smallest position, -(P / 2 - 1) L - (L - 1), is 0
    for phi in range(L):
        for p in range(P):
            h[(p - P // 2 + 1) * L - phi + off] = tab[phi, p]
    n = 1 << 22
    H = np.abs(np.fft.rfft(h, n)) / L
    f = np.arange(len(H)) / n * 2.0 * L                          # in units of the input's Nyquist (the prototype runs at L x the input rate)
    nyq = min(1.0, L / M)                                        # the lower rate's Nyquist in the same units
    pass_db = 20 * np.log10(H[f <= 0.80 * nyq])
    stop_db = 20 * np.log10(np.maximum(H[f >= nyq], 1e-30))
    print(rates, "ripple %+.5f / %+.5f dB, stop band %.2f dB" % (pass_db.max(), pass_db.min(), stop_db.max()))
    assert pass_db.max() <= 0.001 and pass_db.min() >= -0.001, (pass_db.max(), pass_db.min())
    assert stop_db.max() <= -80.0, stop_db.max()


@pytest.mark.parametrize("rates", RATIOS)
def test_table_quality(rates):
    check_table_quality(rates)


def test_equal_rates_table():
    assert resampling().design_table(16000, 16000)[:2] == (1, 1) and resampling().design_table(16000, 16000)[2].tolist() == [[1.0]]


# ---- 2. values ------------------------------------------------------------------------------------------------------------------
def check_ratio_values(lib, rates, S, n_in):
    """Noise, impulses at both ends and a constant, int16 and float32, in_step 1 and 2, rows with a pitch larger than the row whose
    padding (and second channel) is NaN / 0x7fff: nothing outside the rows is read, nothing outside the outputs written."""
    Rs = resampling()
    L, M, tab = Rs.design_table(*rates)
    rng = np.random.RandomState(S + n_in + rates[0] % 1000)
    worst = 0.0
    for dtype in (torch.int16, torch.float32):
        np_t = np.int16 if dtype == torch.int16 else np.float32
        poison = 0x7fff if dtype == torch.int16 else np.nan
        x = noise(rng, S, n_in, dtype)
        x[0, :] = 0
        x[0, 0] = 32767 if dtype == torch.int16 else 1.0                  # impulse at index 0 ...
        if S > 1:
            x[1, :] = 0
            x[1, -1] = -32768 if dtype == torch.int16 else -1.0           # ... and at the last index
        if S > 2:
            x[2, :] = 12345 if dtype == torch.int16 else 0.37             # a constant
        for step in (1, 2):
            rs = make(lib, *rates, S, dtype, channels=step)
            full = np.full((S, n_in * step + 37), poison, np_t)
            full[:, :n_in * step:step] = x
            xd = dev_tensor(lib, full)
            view = xd[:, :n_in * step] if step == 1 else xd[:, :n_in * step].unflatten(1, (n_in, step))
            n_out = rs.out_length(n_in)
            assert n_out == -(-n_in * L // M)
            outd = torch.full((S, n_out + 5), -7.0, dtype=torch.float32, device=xd.device)
            got = rs.convert(view, 0, 0, n_out, out=outd[:, :n_out])
            assert got.data_ptr() == outd.data_ptr()
            o = outd.cpu().numpy()
            assert np.all(o[:, n_out:] == -7.0) and np.isfinite(o).all()
            worst = max(worst, check_values(o[:, :n_out], tab, L, M, x, (rates, S, dtype, step)))
            assert torch.equal(rs.resample(view.contiguous()), outd[:, :n_out])
            if S > 2:       # the constant: from the first output whose taps lie inside the signal to the last, the constant itself
                P = tab.shape[1]
                v = float(decode(x[2, :1])[0])
                j = np.arange(n_out)
                first = (j * M) // L - (P // 2 - 1 if P > 1 else 0)
                inside = (first >= 0) & (first + P <= n_in)
                assert inside.any()
                tol = (P + 1) * 2.0 ** -24 * abs(v) * np.abs(tab).sum(axis=1).max() + abs(v) * P * 2.0 ** -24
                assert np.abs(o[2, :n_out][inside] - v).max() <= tol
    return worst


@pytest.mark.parametrize("rates", RATIOS)
@pytest.mark.parametrize("S,n_in", [(1, 2999), (3, 1777), (64, 901)])
def test_values(emu_lib, rates, S, n_in):
    M = rates[0] // math.gcd(*rates)
    assert M == 1 or n_in % M                                    # (lengths that are not multiples of M)
    w = check_ratio_values(emu_lib, rates, S, n_in)
    assert w < 1.0


# ---- 3. equal rates -------------------------------------------------------------------------------------------------------------
def check_equal_rates(lib):
    rng = np.random.RandomState(3)
    pcm = noise(rng, 3, 5001, torch.int16)
    got = make(lib, 16000, 16000, 3, torch.int16).resample(dev_tensor(lib, pcm)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), (pcm.astype(np.float32) * (1.0 / 32768.0)).view(np.uint32))
    f = noise(rng, 3, 5001, torch.float32)
    f[0, :3] = [0.0, -0.0, -1.0]                                 # (a chain that starts from +0 returns +0 for -0)
    got = make(lib, 44100, 44100, 3, torch.float32).resample(dev_tensor(lib, f)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32)[:, 2:], f.view(np.uint32)[:, 2:]) and np.all(got[0, :2] == 0.0)


def test_equal_rates(emu_lib):
    check_equal_rates(emu_lib)


# ---- 4. chunk and position invariance -------------------------------------------------------------------------------------------
def check_invariance(lib, rates, S, n_in, dtype, seed):
    rng = np.random.RandomState(seed)
    rs = make(lib, *rates, S, dtype)
    x = dev_tensor(lib, noise(rng, S, n_in, dtype))
    whole = rs.resample(x)
    n_out = whole.shape[1]
    # (a) convert over random splits of the outputs (chunks of one sample among them), each from exactly its span
    cuts = sorted(set(rng.randint(1, n_out, size=12).tolist()) | {1, 2, n_out - 1})
    parts = []
    for a, b in zip([0] + cuts, cuts + [n_out]):
        first, n = rs.span(a, b - a)
        lo, hi = max(first, 0), min(first + n, n_in)
        parts.append(rs.convert(x[:, lo:hi], lo, a, b - a))
    assert torch.equal(torch.cat(parts, dim=1), whole)
    # (b) random push sizes (0 and sizes below P among them) + flush
    sizes, pos = [], 0
    while pos < n_in:
        m = min(int(rng.choice([0, 1, 7, rs.taps - 1, rs.taps, 300, 1000])), n_in - pos)
        sizes.append(m)
        pos += m
    outs, pos, n_got = [], 0, 0
    for m in sizes:
        o = rs.push(x[:, pos:pos + m])
        pos += m
        n_got += o.shape[1]
        assert n_got <= rs.out_length(pos)
        outs.append(o)
    outs.append(rs.flush())
    assert torch.equal(torch.cat(outs, dim=1), whole)
    with pytest.raises(T.TcrError, match="reset"):
        rs.push(x[:, :1])
    # (c) after reset the streams repeat their first run
    rs.reset()
    again = [rs.push(x[:, :n_in // 2]), rs.push(x[:, n_in // 2:]), rs.flush()]
    assert torch.equal(torch.cat(again, dim=1), whole)


def check_positions_64bit(lib, rates, q, r, n_out, dtype, seed):
    """x periodic with period M q: outputs from out_first = L q r (out_first M beyond 2^33) are bitwise those from L q."""
    rs = make(lib, *rates, 2, dtype)
    L, M, P = rs.up, rs.down, rs.taps
    period = noise(np.random.RandomState(seed), 2, M * q, dtype)
    outs = []
    for rr in (1, r):
        o1 = L * q * rr
        first, n = rs.span(o1, n_out)
        lead = P // 2 - 1
        assert first == (o1 * M) // L - lead and first + n - 1 == ((o1 + n_out - 1) * M) // L - lead + P - 1
        x = period[:, (first + np.arange(n)) % (M * q)]
        outs.append(rs.convert(dev_tensor(lib, x), first, o1, n_out))
    assert L * q * r * M > 2 ** 33
    assert torch.equal(outs[0], outs[1])
    assert float(outs[0].abs().max()) > 0
    assert rs.span(5, 0)[1] == 0


@pytest.mark.parametrize("rates,dtype", [((48000, 16000), torch.int16), ((44100, 16000), torch.int16), ((8000, 16000), torch.float32),
                                         ((22050, 16000), torch.float32)])
def test_chunk_and_push_invariance(emu_lib, rates, dtype):
    check_invariance(emu_lib, rates, 3, 4321, dtype, 5)


def test_positions_are_64_bit(emu_lib):
    check_positions_64bit(emu_lib, (44100, 16000), 3, 50000, 700, torch.int16, 6)
    check_positions_64bit(emu_lib, (48000, 16000), 5, 1 << 30, 300, torch.float32, 7)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    dev = Cm.device_of(lib)
    tab = torch.ones(4 * 8, dtype=torch.float32, device=dev)
    x = torch.zeros(4096, dtype=torch.float32, device=dev)
    out = torch.full((4096,), -7.0, dtype=torch.float32, device=dev)
    Cfg = T._lib.ResampleCfg

    def call(cfg=(1, 3, 8, 0, 1), table=tab.data_ptr(), S=2, inp=x.data_ptr(), in_pitch=600, in_first=0, n_in=600, out_first=0, n_out=200,
             outp=out.data_ptr(), out_pitch=200):
        c = Cfg(*cfg) if cfg is not None else None
        return lib.tcr_resample(C.byref(c) if c is not None else None, table, S, inp, in_pitch, in_first, n_in, out_first, n_out, outp,
                                out_pitch, None)
    for kw, msg in [(dict(cfg=None), b"null cfg"), (dict(table=None), b"null argument"), (dict(inp=None), b"null argument"),
                    (dict(outp=None), b"null argument"), (dict(cfg=(0, 3, 8, 0, 1)), b"must be >= 1"), (dict(cfg=(1, 0, 8, 0, 1)), b"must be >= 1"),
                    (dict(cfg=(1, 3, 0, 0, 1)), b"must be >= 1"), (dict(cfg=(1, 3, 7, 0, 1)), b"even or 1"), (dict(cfg=(1, 3, 8, 2, 1)), b"in_format"),
                    (dict(cfg=(1, 3, 8, -1, 1)), b"in_format"), (dict(cfg=(1, 3, 8, 0, 0)), b"in_step"), (dict(S=-1), b"negative count"),
                    (dict(n_in=-1), b"negative count"), (dict(n_out=-1), b"negative count"), (dict(in_pitch=599), b"in_pitch"),
                    (dict(cfg=(1, 3, 8, 0, 2), in_pitch=1198), b"in_pitch"), (dict(out_pitch=199), b"out_pitch")]:
        assert call(**kw) == -1, kw
        assert msg in lib.tcr_last_error(), (kw, lib.tcr_last_error())
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(n_out=0) == 0 and call(S=0) == 0 and bool((out == -7.0).all())
    assert call() == 0 and call(cfg=(1, 3, 1, 0, 1)) == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((out[:400] != -7.0).all()) and bool((out[400:] == -7.0).all())
    first, n = C.c_int64(), C.c_int64()
    assert lib.tcr_resample_span(C.byref(Cfg(1, 3, 7, 0, 1)), 0, 1, C.byref(first), C.byref(n)) == -1
    assert lib.tcr_resample_span(C.byref(Cfg(1, 3, 8, 0, 1)), 0, -1, C.byref(first), C.byref(n)) == -1
    assert lib.tcr_resample_span(C.byref(Cfg(1, 3, 8, 0, 1)), 0, 1, None, C.byref(n)) == -1
    Rs = resampling()
    with pytest.raises(T.TcrError, match="dtype"):
        Rs.Resampler(48000, 16000, 1, device=dev, dtype=torch.float64, lib=lib)
    rs = Rs.Resampler(48000, 16000, 2, device=dev, dtype=torch.int16, lib=lib)
    with pytest.raises(T.TcrError, match="expected torch.int16"):
        rs.resample(torch.zeros((2, 100), dtype=torch.float32, device=dev))
    with pytest.raises(T.TcrError, match="2 streams"):
        rs.push(torch.zeros((3, 100), dtype=torch.int16, device=dev))


def test_refusals(emu_lib):
    check_refusals(emu_lib)


# ---- 6. end to end: WAV files at other rates through the command lines ------------------------------------------------------------
def write_wav_rate(path, pcm, rate, channels=1):
    """16-bit PCM; channels > 1: pcm is channel 0, the others hold its negation."""
    inter = pcm if channels == 1 else np.stack([pcm] + [(-pcm.astype(np.int32)).clip(-32768, 32767).astype(np.int16)] * (channels - 1), axis=1)
    data = inter.astype("<i2").tobytes()
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        fh.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * 2 * channels, 2 * channels, 16))
        fh.write(b"data" + struct.pack("<I", len(data)) + data)


def material(seconds, rate, seed):
    a = segment_audio(1, int(seconds * rate), seed)[0]
    return np.clip(a * 32767, -32768, 32767).astype(np.int16)


CLI_DET = ["--frames_per_step", "2", "--average_window_ms", "200", "--min_count", "2", "--detection_threshold", "0.3", "--suppression_ms", "400"]
CLI_KW = dict(frames_per_step=2, average_window_ms=200, min_count=2, detection_threshold=0.3, suppression_ms=400)


def run_cli(module, argv, capsys):
    capsys.readouterr()
    assert module.main(module.parse_arguments(argv)) == 0
    return capsys.readouterr()


def check_end_to_end(lib, tmp_path, capsys, monkeypatch, seconds):
    from tcresnet_amd import audio_input, deploy, runtime, scan_audio, stream_audio, streaming, sweep_audio
    Rs = resampling()
    dev = Cm.device_of(lib)
    fe, net, _, _, _ = setup(lib)
    path = frozen_artifact(net, fe, str(tmp_path / "kws.npz"))
    pcm = {"a48.wav": (material(seconds, 48000, 41), 48000, 1), "b44.wav": (material(seconds * 0.8 + 0.0123, 44100, 42), 44100, 2),
           "c16.wav": (material(seconds * 0.6, 16000, 43), 16000, 1)}
    wavs = {}
    for name, (x, rate, ch) in pcm.items():
        wavs[name] = str(tmp_path / name)
        write_wav_rate(wavs[name], x, rate, ch)
    labels = [f"c{i}" for i in range(12)]
    saved = runtime.default_lib(), runtime.default_device()
    runtime.set_default(lib, dev)
    try:
        model = deploy.FrozenModel.load(path)
        assert model.resampler(48000, 1).out_rate == 16000 and model.resampler(8000, 3).up == 2          # (7.)
        scanner = model.scanner(**CLI_KW)
        step = scanner.step_samples
        rows = {}

        def recordings(paths, det):
            """(the whole recordings as the tools take them: one chunk of every step, their lengths)"""
            rec = audio_input.Recordings(paths, det)
            (i0, buf), = rec.chunks()
            assert i0 == 0
            return buf, rec.lengths

        for name in ("a48.wav", "b44.wav"):
            x, rate, _ = pcm[name]
            # each row of the buffer: bitwise Resampler(rate, 16000, 1).resample(pcm), cut to whole steps
            want = Rs.Resampler(rate, 16000, 1, device=dev, lib=lib).resample(dev_tensor(lib, x[None, :]))
            want = want[:, :want.shape[1] // step * step]
            buf, lengths = recordings([wavs[name]], scanner)
            assert lengths == [want.shape[1]] and torch.equal(buf, want)
            rows[name] = want
            # scan_audio.py's stdout: exactly the lines scanner.scan of that buffer yields; time_ms in real time
            r = run_cli(scan_audio, ["--frozen", path, "--wav", wavs[name], "--labels", ",".join(labels), *CLI_DET, "--summary"], capsys)
            out = scanner.scan(want)
            fired, top, score = out.is_new.cpu().numpy()[0], out.top.cpu().numpy()[0], out.score.cpu().numpy()[0]
            lines = [f"{wavs[name]},{stream_audio.format_time_ms(1000.0 * (i + 1) * step / 16000)},{labels[top[i]]},{float(score[i]):.6f}"
                     for i in np.flatnonzero(fired)]
            assert r.out.splitlines() == lines and len(lines) >= 1
            assert f"{wavs[name]}: {rate} Hz -> 16000 Hz" in r.err.splitlines()
            last = float(r.out.splitlines()[-1].split(",")[1])
            assert last <= 1000.0 * len(x) / rate + 1e-6                      # real time: inside the recording
            # --chunk_seconds: stdout and stderr byte for byte the one-call run's
            for sec in ("0.5", "0.13"):
                rc = run_cli(scan_audio, ["--frozen", path, "--wav", wavs[name], "--labels", ",".join(labels), *CLI_DET, "--summary",
                                          "--chunk_seconds", sec], capsys)
                assert rc.out == r.out and rc.err == r.err
            # stream_audio.py: the same signal, the same lines
            st, _ = recordings([wavs[name]], model.streaming(1, **CLI_KW))
            assert torch.equal(st.view(torch.int32), want.view(torch.int32))
            fed, push = [], streaming.StreamingDetector.push
            with monkeypatch.context() as m:                                  # what the tool pushes, step by step
                m.setattr(streaming.StreamingDetector, "push", lambda self, x: (fed.append(x.clone()), push(self, x))[1])
                rs_ = run_cli(stream_audio, ["--frozen", path, "--wav", wavs[name], "--labels", ",".join(labels), *CLI_DET], capsys)
            assert rs_.out == r.out
            assert all(x.shape == (1, step) and x.is_contiguous() for x in fed)
            assert torch.equal(torch.cat(fed, dim=1).view(torch.int32), want.view(torch.int32))
        # 16 kHz, 48 kHz and 44.1 kHz in one invocation: each row is the file's single-file row, zero-padded to the longest
        x16 = pcm["c16.wav"][0]
        row16 = dev_tensor(lib, (x16.astype(np.float32) * (1.0 / 32768.0))[None, :len(x16) // step * step])
        order = ["c16.wav", "a48.wav", "b44.wav"]
        rows["c16.wav"] = row16
        buf, lengths = recordings([wavs[n] for n in order], scanner)
        capsys.readouterr()
        assert lengths == [rows[n].shape[1] for n in order] and buf.shape == (3, max(lengths))
        for s, n in enumerate(order):
            assert torch.equal(buf[s, :lengths[s]], rows[n][0]) and not bool(buf[s, lengths[s]:].any())
        mixed = ["--frozen", path, "--wav", *[wavs[n] for n in order], "--labels", ",".join(labels), *CLI_DET]
        r = run_cli(scan_audio, mixed, capsys)
        rc = run_cli(scan_audio, mixed + ["--chunk_seconds", "0.3"], capsys)
        assert rc.out == r.out and rc.err == r.err and len(r.out.splitlines()) >= 3
        chunks = torch.cat([c for _, c in audio_input.Recordings([wavs[n] for n in order], scanner).chunks(0.3)], dim=1)
        capsys.readouterr()
        assert torch.equal(chunks, buf)
        # sweep_audio.py reads the same buffer: its chunked run prints what its one-call run prints
        ev = tmp_path / "events.csv"
        ev.write_text("file,start_ms,end_ms,label\n" + f"{wavs['a48.wav']},200,900,c1\n{wavs['a48.wav']},1200,1900,c2\n{wavs['b44.wav']},100,1500,c3\n")
        sw = ["--frozen", path, "--events", str(ev), "--tolerance_ms", "100", "--wav", *[wavs[n] for n in order], "--labels", ",".join(labels), "--thresholds", "0:0.9:0.3",
              "--frames_per_step", "2", "--average_window_ms", "200", "--min_count", "2", "--suppression_ms", "400", "--keywords", "c1,c2,c3"]
        a, b = run_cli(sweep_audio, sw, capsys), run_cli(sweep_audio, sw + ["--chunk_seconds", "0.3"], capsys)
        assert a.out == b.out and a.err == b.err and "48000 Hz -> 16000 Hz" in a.err
        import json
        assert json.loads(a.err.strip().splitlines()[-1])["hours"] == pytest.approx(sum(lengths) / 16000 / 3600)
        # files at the model's rate: no Resampler is built, the buffer is the host decode
        def boom(*args, **kw):
            raise AssertionError("a Resampler was constructed for files at the model's rate")
        monkeypatch.setattr(audio_input, "Resampler", boom)             # the one place the tools construct one
        buf, lengths = recordings([wavs["c16.wav"]], scanner)
        assert torch.equal(buf, row16)
        only16 = ["--frozen", path, "--wav", wavs["c16.wav"], "--labels", ",".join(labels), *CLI_DET]
        r16 = run_cli(scan_audio, only16, capsys)
        assert run_cli(scan_audio, only16 + ["--chunk_seconds", "0.3"], capsys).out == r16.out
        assert run_cli(stream_audio, only16, capsys).out == r16.out and "Hz ->" not in r16.err
    finally:
        runtime.set_default(*saved)


def test_end_to_end_short(emu_lib, tmp_path, capsys, monkeypatch):
    check_end_to_end(emu_lib, tmp_path, capsys, monkeypatch, 2.5)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rates", RATIOS)
def test_gpu_values(hip_lib, rates):
    for S, n_in in [(1, 29999), (3, 17777), (64, 9001)]:
        assert check_ratio_values(hip_lib, rates, S, n_in) < 1.0


@pytest.mark.gpu
def test_gpu_values_ten_minutes_44100(hip_lib):
    rng = np.random.RandomState(9)
    n_in = 600 * 44100 + 17
    x = noise(rng, 8, n_in, torch.int16)
    rs = make(hip_lib, 44100, 16000, 8, torch.int16)
    got = rs.resample(dev_tensor(hip_lib, x)).cpu().numpy()
    assert got.shape == (8, -(-n_in * 160 // 441))
    L, M, tab = resampling().design_table(44100, 16000)
    worst = check_values(got, tab, L, M, x, "ten minutes at 44.1 kHz")
    print("worst error / bound", worst)


@pytest.mark.gpu
def test_gpu_equal_rates(hip_lib):
    check_equal_rates(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("rates,dtype", [((48000, 16000), torch.int16), ((44100, 16000), torch.int16), ((8000, 16000), torch.float32),
                                         ((22050, 16000), torch.float32), ((16000, 8000), torch.int16), ((32000, 16000), torch.float32)])
def test_gpu_chunk_and_push_invariance(hip_lib, rates, dtype):
    check_invariance(hip_lib, rates, 5, 54321, dtype, 5)


@pytest.mark.gpu
def test_gpu_positions_are_64_bit(hip_lib):
    check_positions_64bit(hip_lib, (44100, 16000), 3, 50000, 7000, torch.int16, 6)
    check_positions_64bit(hip_lib, (48000, 16000), 5, 1 << 30, 3000, torch.float32, 7)


@pytest.mark.gpu
def test_gpu_refusals(hip_lib):
    check_refusals(hip_lib)


@pytest.mark.gpu
def test_gpu_end_to_end(hip_lib, tmp_path, capsys, monkeypatch):
    check_end_to_end(hip_lib, tmp_path, capsys, monkeypatch, 40.0)
