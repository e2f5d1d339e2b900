"""tcr_resample across its tile geometries (table: tests/resample_configs.py): short last row groups, G cut by the table budget, B in
{1, 2, 3, 4} and B rounded to four-chain units, a second q-tile under several row groups, P in {1, 2} and the largest P, negative
out_first, the second launch past 65 535 streams, and the three size refusals.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`).

Per row, at the C ABI, rows inside poisoned buffers (NaN / 0x7fff in the pitch padding, in the other channel of in_step 2 and in
guard zones around the rows; -7 around and between the output rows):
  exact      integer table in -3 .. 3, int16-valued input small enough that every partial sum is an integer multiple of 2^-15 below
             2^24 of those units: the fmaf chain is exact, the output BITWISE the int64 sum
             y[j] = sum_p c[(j M) mod L][p] x[floor(j M / L) - lead + p]
  probe      one-hot rows, table[phi][p0(phi)] = 2^-(phi mod 8), p0(phi) = (lead + (3 + 5 phi) mod min(P, 7)) mod P, every input sample distinct: the output
             is bitwise one scaled sample, so a wrong row, offset, lead or tile base is an exact mismatch
  noise      random float32 table (raw rows) or design_table (real pairs), random input: within test_resample.py's chain bound
             (P + 1) 2^-24 sum |c x| of the float64 dot product
  positions  the same outputs from out_first values that shift the tile grid, from a negative out_first through 0, from exactly
             tcr_resample_span's slice, from a buffer that starts at a negative index: bitwise the row's whole conversion
The exact and position checks run on the emulator a second time with the workgroups of a launch last to first: a tile that wrote
into its neighbour's q (the `b >= B` mask at B in {1, 2, 3}) is overwritten by the neighbour in launch order and shows only then.
What no check of values can tell: the kernel's `G = L - r0` of a short last group only saves work -- with the full G the surplus
rows are residues r >= L, the same outputs of q + 1 that the first group writes, from the same staged samples to the same bits.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tests import common as Cm
from tests import resample_configs as RC
from tests.test_net_configs import Log
from tests.test_resample import (check_invariance, check_table_equals_restatement, check_table_quality, check_values, dev_tensor,
                                 resampling)

GUARD = 64                      # poisoned elements in front of the first and behind the last row
S = 2
CMAX = 3                        # |integer table entry| of the exact case
assert (int(np.int64(-7) // np.int64(3)), int(np.int64(-7) % np.int64(3))) == (-3, 2) == (-7 // 3, -7 % 3)      # floor and non-negative, as Python's


def lead_of(P):
    return P // 2 - 1 if P > 1 else 0


def n_in_of(row):
    """The last output's first-tap-after-lead is the last sample: its later taps, and only they, read past the end."""
    return ((row.n_out - 1) * row.M) // row.L + 1


def cfg_of(row, in_format, step=1):
    return T._lib.ResampleCfg(row.L, row.M, row.P, in_format, step)


def sync(lib):
    if lib.kind == "hip":
        torch.cuda.synchronize()


class BlocksLastToFirst:
    """Emulator: the launches of the block run their workgroups last to first (tests/emu/hip/hip_runtime.h).  Workgroups that write
    disjoint outputs give the same bits in either order; a tile that also wrote its neighbour's outputs is overwritten by the
    neighbour in one order and overwrites it in the other.  The device has no such order: a no-op there."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        if self.lib.kind == "emu":
            f = self.lib._dll.tcr_emu_block_order
            f.restype, f.argtypes = C.c_int, [C.c_int]
            self.was = f(1)
        return self

    def __exit__(self, *exc):
        if self.lib.kind == "emu":
            self.lib._dll.tcr_emu_block_order(self.was)
        return False


def run(lib, row, table, x, in_first, out_first, n_out, step=1, pad=37):
    """tcr_resample of x (np int16 or float32 [S, n]: samples in_first .. in_first + n - 1) -> np float32 [S, n_out].  Asserts that
    nothing outside the n_out columns is written and nothing that is poison was read."""
    rows, n = x.shape
    is16 = x.dtype == np.int16
    poison = 0x7fff if is16 else np.nan
    in_pitch = n * step + pad
    buf = np.full(2 * GUARD + rows * in_pitch, poison, x.dtype)
    buf[GUARD:GUARD + rows * in_pitch].reshape(rows, in_pitch)[:, :n * step:step] = x
    out_pitch = n_out + (5 if pad else 0)
    xd = dev_tensor(lib, buf)
    od = torch.full((2 * GUARD + rows * out_pitch,), -7.0, dtype=torch.float32, device=xd.device)
    cfg = cfg_of(row, 1 if is16 else 0, step)
    rc = lib.tcr_resample(C.byref(cfg), table.data_ptr(), rows, xd.data_ptr() + GUARD * buf.itemsize, in_pitch, int(in_first), n,
                          int(out_first), int(n_out), od.data_ptr() + GUARD * 4, out_pitch, None)
    assert rc == 0, (row.name, lib.tcr_last_error())
    sync(lib)
    o = od.cpu().numpy()
    body = o[GUARD:GUARD + rows * out_pitch].reshape(rows, out_pitch)
    assert np.all(o[:GUARD] == -7.0) and np.all(o[GUARD + rows * out_pitch:] == -7.0) and np.all(body[:, n_out:] == -7.0), row.name
    got = body[:, :n_out].copy()
    assert np.isfinite(got).all(), (row.name, "poison was read")
    return got


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), "first at (stream, column)", bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def as_format(x16, in_format):
    """int16 values as the call's input: the int16 themselves, or their exact float32 decode."""
    return x16 if in_format == 1 else x16.astype(np.float32) * np.float32(1.0 / 32768.0)


def exact_reference(row, table, x, out_first, n_out, in_first=0):
    """float32 [S, n_out] from integers: table int64 [L, P], x int64 [S, n] in units of 2^-15 with global index in_first on.
    y[j] = sum_p c[(j M) mod L][p] x[floor(j M / L) - lead + p], x = 0 outside: floor division and non-negative modulo per output,
    no shared windows."""
    L, M, P = row.L, row.M, row.P
    n = x.shape[1]
    jm = (out_first + np.arange(n_out, dtype=np.int64)) * M
    n_j, phi = jm // L, jm % L
    assert (phi >= 0).all() and (n_j * L + phi == jm).all()
    idx = n_j[:, None] - lead_of(P) + np.arange(P, dtype=np.int64)[None, :] - in_first
    ok = (idx >= 0) & (idx < n)
    xi = np.where(ok[None], x[:, np.clip(idx, 0, n - 1)], 0)                        # [S, n_out, P]
    y = (xi * table[phi][None]).sum(axis=2)
    assert np.abs(y).max(initial=0) < 2 ** 24
    return (y.astype(np.float64) / 32768.0).astype(np.float32)


def formats_and_steps(row):
    """(in_format, in_step): both formats and both steps on every row; the short-group and table-limited rows all four pairs."""
    if row.cls in (RC.SHORT, RC.TABLE, RC.BOUNDARY):
        return [(1, 1), (1, 2), (0, 1), (0, 2)]
    return [(1, 1), (0, 2)]


# ---- the table of rows against the restated arithmetic (CPU only) -----------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.ROW_IDS)
def test_row_states_its_geometry(name):
    row = RC.ROW[name]
    g = RC.geometry(row.L, row.M, row.P)
    assert isinstance(g, RC.Geometry), g
    assert (row.G, row.B, row.groups, row.last, row.lds) == tuple(g[:5]), g
    assert RC.CLASSES[row.cls](row, g), (row.cls, g)
    assert row.lds <= RC.MAX_LDS and n_in_of(row) <= 65536
    if row.pair:
        L, M, tab = resampling().design_table(row.pair[0], row.pair[1], zero_crossings=row.pair[2])
        assert (L, M, tab.shape[1]) == (row.L, row.M, row.P)


def test_every_class_has_rows():
    assert {r.cls for r in RC.ROWS} == set(RC.CLASSES)
    by = {c: [r for r in RC.ROWS if r.cls == c] for c in RC.CLASSES}
    assert {r.last for r in by[RC.SHORT]} >= {1, 19, 25} and {r.G for r in by[RC.TABLE]} >= {2, 17, 31}
    assert {r.B for r in by[RC.SMALL_B]} >= {1, 2, 3, 4, 232, 532, 340} and {r.P for r in by[RC.DEGENERATE]} >= {1, 2, 6142}
    # a second q-tile under several row groups, and under a short last group
    assert any(r.groups > 1 and r.last < r.G and r.n_out > r.B * r.L for r in RC.ROWS)
    assert max(r.lds for r in RC.ROWS) == RC.ROW["44100_8000"].lds == 80876 > 64 * 1024
    for cause, L, M, P in RC.REFUSED:
        g = RC.geometry(L, M, P)
        assert (g == cause) if cause != "groups" else (g.groups == 65536), (cause, L, M, P, g)
        if cause == "span":             # the deficit is below M: truncating division gives b_fit = 1
            G = min(L, RC.MAX_ROWS, RC.TABLE_FLOATS // (P | 1))
            assert -M < RC.SPAN_FLOATS - P - (-(-G * M // L) + 1) < 0
    assert RC.geometry(1, 14333, 2).B == 1 and RC.geometry(1, 1, 6142).G == 1 and RC.geometry(1, 1, 6144) == RC.TAPS_REFUSED


def tile_spans(L, M, P, g):
    """Per row group: (the samples the kernel stages, the last LDS sample a chain reads + 1), from the kernel's expressions."""
    out = []
    for r0 in range(0, L, g.G):
        G = min(g.G, L - r0)
        f0 = r0 * M // L
        span = (g.B - 1) * M + ((r0 + G - 1) * M // L - f0) + P
        reach = (g.B - 1) * M + max((r0 + k) * M // L - f0 for k in range(G)) + P
        out.append((span, reach))
    return out


def test_restated_tile_stays_inside_lds():
    """What the kernel stages and reads, per row group, against the span region the host sizes: every accepted triple of the table and
    of a grid around the limits stays inside span_cap <= 14336 floats and inside 80.25 KB."""
    triples = [(r.L, r.M, r.P) for r in RC.ROWS]
    rng = np.random.RandomState(11)
    for _ in range(3000):
        L = int(rng.choice([1, 2, 3, 31, 32, 33, 64, 80, 147, 441, int(rng.randint(1, 700))]))
        M = int(rng.choice([1, 2, 7, 160, 441, 4700, 14333, 14334, 30000, int(rng.randint(1, 120000))]))
        P = int(rng.choice([1, 2, 4, 64, 190, 192, 354, 2048, 6142, 2 * int(rng.randint(1, 3072))]))
        triples.append((L, M, P))
    accepted = 0
    for L, M, P in triples:
        g = RC.geometry(L, M, P)
        if not isinstance(g, RC.Geometry):
            continue
        accepted += 1
        span_cap = g.lds // 4 - g.G * (P | 1) - 2 * RC.MAX_ROWS
        assert span_cap <= RC.SPAN_FLOATS and g.lds <= RC.MAX_LDS and g.B >= 1, (L, M, P, g)
        for span, reach in tile_spans(L, M, P, g):
            assert reach <= span <= span_cap, (L, M, P, g, span, reach)
    assert accepted > 1000


# ---- per row ------------------------------------------------------------------------------------------------------------------------------
def exact_case(row):
    rng = np.random.RandomState(1000 + RC.ROW_IDS.index(row.name))
    xmax = min(32767, (2 ** 24 - 1) // (CMAX * row.P))
    table = rng.randint(-CMAX, CMAX + 1, size=(row.L, row.P)).astype(np.int64)
    x = rng.randint(-xmax, xmax + 1, size=(S, n_in_of(row))).astype(np.int16)
    return table, x


def check_exact(lib, row):
    table, x = exact_case(row)
    td = dev_tensor(lib, table.astype(np.float32))
    want = exact_reference(row, table, x.astype(np.int64), 0, row.n_out)
    assert np.abs(want).max() > 0
    for in_format, step in formats_and_steps(row):
        same_bits(run(lib, row, td, as_format(x, in_format), 0, 0, row.n_out, step=step), want, (row.name, "exact", in_format, step))
    with BlocksLastToFirst(lib):
        same_bits(run(lib, row, td, x, 0, 0, row.n_out), want, (row.name, "exact, workgroups last to first"))
    # a negative out_first through 0: zeros, plus the samples the taps reach
    o = -(row.L + 2)
    n = min(row.n_out - o, 3 * row.L + 11)
    want = exact_reference(row, table, x.astype(np.int64), o, n)
    same_bits(run(lib, row, td, x, 0, o, n), want, (row.name, "exact, negative out_first", o, n))
    if row.L > row.M and lead_of(row.P) >= 2:
        assert np.abs(want[:, :-o]).max() > 0                         # (interpolation: outputs before 0 whose taps reach the signal)


def probe_case(row):
    L, P = row.L, row.P
    p0 = (lead_of(P) + (3 + 5 * np.arange(L)) % min(P, 7)) % P         # (at the lead and up to six taps on: most outputs land on a sample)
    scale = 2.0 ** -(np.arange(L) % 8)
    table = np.zeros((L, P), np.float32)
    table[np.arange(L), p0] = scale
    n = n_in_of(row)
    assert n <= 65536
    x = (((np.arange(n, dtype=np.int64)[None, :] * 7919 + np.arange(S, dtype=np.int64)[:, None] * 12345) % 65536) - 32768).astype(np.int16)
    assert all(len(np.unique(r)) == n for r in x)
    return table, p0, scale, x


def check_probe(lib, row):
    table, p0, scale, x = probe_case(row)
    td = dev_tensor(lib, table)
    L, M, P = row.L, row.M, row.P
    xdec = x.astype(np.float64) / 32768.0
    for o, n_out in [(0, row.n_out), (-(row.L + 2), min(row.n_out, 2 * row.L + 9) + row.L + 2)]:
        jm = (o + np.arange(n_out, dtype=np.int64)) * M
        at = jm // L - lead_of(P) + p0[jm % L]
        ok = (at >= 0) & (at < x.shape[1])
        want = np.where(ok[None], xdec[:, np.clip(at, 0, x.shape[1] - 1)] * scale[jm % L][None], 0.0).astype(np.float32)
        assert o < 0 or ok.mean() > 0.5, (row.name, float(ok.mean()))
        for in_format, step in (formats_and_steps(row) if o == 0 else [(1, 1)]):
            same_bits(run(lib, row, td, as_format(x, in_format), 0, o, n_out, step=step), want, (row.name, "probe", o, in_format, step))


def noise_case(row):
    rng = np.random.RandomState(2000 + RC.ROW_IDS.index(row.name))
    if row.pair:
        table = resampling().design_table(row.pair[0], row.pair[1], zero_crossings=row.pair[2])[2]
    else:
        table = rng.uniform(-1, 1, size=(row.L, row.P)).astype(np.float32)
    n = n_in_of(row)
    return table, rng.randint(-32768, 32768, size=(S, n)).astype(np.int16), rng.uniform(-1, 1, size=(S, n)).astype(np.float32)


def check_noise(lib, row):
    table, x16, xf = noise_case(row)
    td = dev_tensor(lib, table)
    worst = 0.0
    for x, step in ((x16, 2), (xf, 1)):
        got = run(lib, row, td, x, 0, 0, row.n_out, step=step)
        worst = max(worst, check_values(got, table, row.L, row.M, x, (row.name, "noise", x.dtype)))
    o = -(row.L + 2)
    n = min(row.n_out - o, 3 * row.L + 11)
    worst = max(worst, check_values(run(lib, row, td, xf, 0, o, n), table, row.L, row.M, xf, (row.name, "noise, negative out_first"), out_first=o))
    print("RESAMPLE_CONFIGS_ERR " + json.dumps({"row": row.name, "lib": lib.kind, "lmp": [row.L, row.M, row.P], "worst_err_over_bound": worst}))
    assert worst < 1.0
    return worst


def restated_span(row, o, n):
    first = (o * row.M) // row.L - lead_of(row.P)
    return first, (((o + n - 1) * row.M) // row.L - lead_of(row.P) + row.P - first if n else 0)


def check_positions(lib, row):
    """Noise, so that an order of summation that depended on the tile would show: everything bitwise the whole conversion."""
    table, x16, xf = noise_case(row)
    x = x16 if RC.ROW_IDS.index(row.name) % 2 else xf
    td = dev_tensor(lib, table)
    L, N, n_in, tile = row.L, row.n_out, x.shape[1], row.B * row.L
    whole = run(lib, row, td, x, 0, 0, N)
    assert np.abs(whole).max() > 0
    with BlocksLastToFirst(lib):
        same_bits(run(lib, row, td, x, 0, 0, N), whole, (row.name, "workgroups last to first"))
    # out_first = 0, 1, L - 1 (mod L), just below and above multiples of B L: the tile grid moves under the same outputs
    firsts = sorted({o for o in (1, L - 1, L, L + 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1, N - 1) if 0 < o < N})
    for o in firsts:
        n = min(N - o, tile + L + 5)
        same_bits(run(lib, row, td, x, 0, o, n), whole[:, o:o + n], (row.name, "out_first", o, n))
    # a negative out_first through 0: its j >= 0 part
    o = -(L + 2)
    n = min(N, 2 * L + 9) - o
    got = run(lib, row, td, x, 0, o, n)
    same_bits(got[:, -o:], whole[:, :n + o], (row.name, "negative out_first", o, n))
    # exactly tcr_resample_span's slice with its in_first; tcr_resample_span against the floor formula, negative positions included
    cfg = cfg_of(row, 1 if x.dtype == np.int16 else 0)
    first, ns = C.c_int64(), C.c_int64()
    for o, n in [(0, N), (N // 3, min(N - N // 3, L + 7)), (N - 1, 1), (max(tile - 1, 0), min(N - max(tile - 1, 0), 2))]:
        if not 0 <= o < N or n < 1:
            continue
        assert lib.tcr_resample_span(C.byref(cfg), o, n, C.byref(first), C.byref(ns)) == 0
        assert (first.value, ns.value) == restated_span(row, o, n)
        lo, hi = max(first.value, 0), min(first.value + ns.value, n_in)
        if hi > lo:
            same_bits(run(lib, row, td, x[:, lo:hi], lo, o, n), whole[:, o:o + n], (row.name, "span slice", o, n, lo, hi))
    for o in (-3 * L - 1, -L - 1, -L, -1, 0, 1, -(1 << 40) - 1):
        for n in (0, 1, L, 2 * L + 1):
            assert lib.tcr_resample_span(C.byref(cfg), o, n, C.byref(first), C.byref(ns)) == 0
            assert (first.value, ns.value) == restated_span(row, o, n), (row.name, o, n)
    # a buffer whose first sample has a negative global index (five zeros in front of the signal)
    n = min(N, tile + L + 5)
    xz = np.concatenate([np.zeros((S, 5), x.dtype), x], axis=1)
    same_bits(run(lib, row, td, xz, -5, 0, n), whole[:, :n], (row.name, "in_first = -5"))


CHECKS = {"exact": check_exact, "probe": check_probe, "noise": check_noise, "positions": check_positions}


@pytest.mark.parametrize("name", RC.ROW_IDS)
@pytest.mark.parametrize("kind", list(CHECKS))
def test_row(emu_lib, kind, name):
    CHECKS[kind](emu_lib, RC.ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.ROW_IDS)
@pytest.mark.parametrize("kind", list(CHECKS))
def test_gpu_row(hip_lib, kind, name):
    CHECKS[kind](hip_lib, RC.ROW[name])


# ---- through Resampler: the real pairs ------------------------------------------------------------------------------------------------------
PAIRS = [r for r in RC.ROWS if r.pair]


def check_resampler(lib, row):
    """Resampler of the pair gives the C-ABI call's bits (same table, same cfg), for whole signals and push / flush."""
    table, x16, _ = noise_case(row)
    rs = resampling().Resampler(row.pair[0], row.pair[1], S, device=Cm.device_of(lib), dtype=torch.int16, lib=lib, zero_crossings=row.pair[2])
    assert (rs.up, rs.down, rs.taps) == (row.L, row.M, row.P) and np.array_equal(rs.table.cpu().numpy(), table)
    n = rs.out_length(x16.shape[1])
    assert n >= row.n_out - row.L
    want = run(lib, row, rs.table, x16, 0, 0, n)
    xd = dev_tensor(lib, x16)
    same_bits(rs.resample(xd).cpu().numpy(), want, (row.name, "Resampler.resample"))
    half = x16.shape[1] // 2
    parts = [rs.push(xd[:, :half]), rs.push(xd[:, half:]), rs.flush()]
    same_bits(torch.cat(parts, dim=1).cpu().numpy(), want, (row.name, "push / flush"))


@pytest.mark.parametrize("name", [r.name for r in PAIRS])
def test_resampler(emu_lib, name):
    check_resampler(emu_lib, RC.ROW[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in PAIRS])
def test_gpu_resampler(hip_lib, name):
    check_resampler(hip_lib, RC.ROW[name])


# ---- once per family ------------------------------------------------------------------------------------------------------------------------
INVARIANCE = [((44100, 8000), torch.int16, 9000), ((16000, 44100), torch.float32, 4321), ((192000, 8000), torch.int16, 40000)]


@pytest.mark.parametrize("rates,dtype,n_in", INVARIANCE)
def test_chunk_and_push_invariance(emu_lib, rates, dtype, n_in):
    check_invariance(emu_lib, rates, 2, n_in, dtype, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("rates,dtype,n_in", INVARIANCE)
def test_gpu_chunk_and_push_invariance(hip_lib, rates, dtype, n_in):
    check_invariance(hip_lib, rates, 3, n_in, dtype, 5)


@pytest.mark.parametrize("name", [r.name for r in PAIRS])
def test_table_equals_restatement(name):
    row = RC.ROW[name]
    check_table_equals_restatement(row.pair[:2], (row.L, row.M, row.P), zero_crossings=row.pair[2])


@pytest.mark.parametrize("name", [r.name for r in PAIRS if r.pair[2] == 32])
def test_table_quality(name):
    check_table_quality(RC.ROW[name].pair[:2])                  # (the design's own zero_crossings: what its limits are stated for)


MESSAGES = {"taps": b"taps per phase are more than the kernel stages", "span": b"need more than the 14336 samples a workgroup stages",
            "groups": b"more phase groups than one launch covers"}


def check_size_refusals(lib):
    """Each with its message, -1, no launch, the output untouched.  The table is never read: one small allocation serves."""
    dev = Cm.device_of(lib)
    tab = torch.ones(64, dtype=torch.float32, device=dev)
    x = torch.zeros(64, dtype=torch.float32, device=dev)
    out = torch.full((64,), -7.0, dtype=torch.float32, device=dev)
    for cause, L, M, P in RC.REFUSED:
        for n_out in (3, 0) if cause != "groups" else (3,):     # (the size of a filter is refused whatever the counts)
            cfg = T._lib.ResampleCfg(L, M, P, 0, 1)
            with Log(lib) as g:
                rc = lib.tcr_resample(C.byref(cfg), tab.data_ptr(), 1, x.data_ptr(), 16, 0, 16, 0, n_out, out.data_ptr(), 3, None)
            assert rc == -1, (cause, L, M, P, n_out, rc, lib.tcr_last_error())
            assert MESSAGES[cause] in lib.tcr_last_error(), (cause, L, M, P, lib.tcr_last_error())
            assert g.entries == []
    sync(lib)
    assert bool((out == -7.0).all())


def test_size_refusals(emu_lib):
    check_size_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_size_refusals(hip_lib):
    check_size_refusals(hip_lib)


def check_second_launch(lib):
    """65 539 streams of 8 samples at (2, 1, 4): a launch of 65 535 and one of 4.  Stream s holds base row s mod 7: every stream is
    bitwise the 7-stream conversion's row, on both sides of the split."""
    n_streams, n = 65539, 8
    rng = np.random.RandomState(65539)
    table = dev_tensor(lib, rng.uniform(-1, 1, size=(2, 4)).astype(np.float32))
    base = dev_tensor(lib, rng.uniform(-1, 1, size=(7, n)).astype(np.float32))
    x = base[torch.arange(n_streams, device=base.device) % 7].contiguous()
    cfg = T._lib.ResampleCfg(2, 1, 4, 0, 1)
    outs = []
    for inp in (base, x):
        rows = inp.shape[0]
        out = torch.full((rows, 2 * n + 3), -7.0, dtype=torch.float32, device=base.device)
        assert lib.tcr_resample(C.byref(cfg), table.data_ptr(), rows, inp.data_ptr(), n, 0, n, 0, 2 * n, out.data_ptr(), 2 * n + 3, None) == 0
        outs.append(out)
    sync(lib)
    small, big = outs
    assert bool((small[:, 2 * n:] == -7.0).all()) and bool((big[:, 2 * n:] == -7.0).all()) and float(small[:, :2 * n].abs().max()) > 0
    want = small[torch.arange(n_streams, device=base.device) % 7]
    assert torch.equal(big.view(torch.int32), want.view(torch.int32))
    for s in (0, 65534, 65535, 65536, 65538):
        assert torch.equal(big[s], small[s % 7])


@pytest.mark.gpu
def test_gpu_second_launch_past_65535_streams(hip_lib):
    check_second_launch(hip_lib)


def test_second_launch_past_65535_streams(emu_lib):
    check_second_launch(emu_lib)                                # (3 s on the emulator: 65 539 workgroups of one tile)
