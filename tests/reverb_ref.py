"""The reference of tcr_reverb's rule (include/tcresnet_hip.h), in NumPy, independent of the kernel's tiling.

The rule: y[i] = the float32 fmaf chain from 0 over the input index jj ascending, acc = fmaf(h[i - jj], x[jj], acc),
jj = max(0, i - L + 1) .. min(i, n - 1).  NumPy has no fmaf, so `chain` is exact only on a fixed-point grid:

    |h| <= 1, h a multiple of 2^-11 (`grid_response`);  x = int16 / 32768 (a multiple of 2^-15, |x| <= 1), also when passed as float32.

Then every product h x is a multiple of 2^-26 of magnitude <= 1, every float32 partial sum is a multiple of 2^-26 too (rounding a
multiple of 2^-26 to 24 bits gives a multiple of 2^-26 or of a higher power of two) and, over at most 2^14 terms, below 2^15 in
magnitude.  A multiple of 2^-26 below 2^15 has at most 41 significant bits, so float64(acc) + float64(h) * float64(x) -- product and sum --
is exact in float64, and the cast to float32 is the one rounding fmaf does.  `check_grid_argument` re-checks that against rational
arithmetic.  Off the grid (`dot64`), the float64 dot product and the fmaf-chain bound (terms + 1) 2^-24 sum |h x|, the form of
test_resample.reference."""
from fractions import Fraction

import numpy as np

GRID = 2.0 ** -11


def grid_response(rng, L, scale=1.0):
    """L taps on the grid: multiples of 2^-11 in [-scale, scale], scale <= 1, the first one non-zero."""
    k = int(round(scale / GRID))
    h = rng.randint(-k, k + 1, L).astype(np.float64) * GRID
    if h[0] == 0:
        h[0] = GRID * k
    return h.astype(np.float32)


def decode(x):
    """The kernel's decode: int16 -> (float)v * (1 / 32768.f), exact; float32 as it is."""
    x = np.asarray(x)
    return (x.astype(np.float32) * np.float32(1.0 / 32768.0)) if x.dtype == np.int16 else x.astype(np.float32)


def chain(x, h, idx):
    """y[i] for i in idx (any i >= 0; 0 at or beyond n + L - 1), bitwise on the grid.  Vectorised over the outputs, a loop over the
    chain position."""
    x64, h64 = decode(x).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
    n, L = x64.size, h64.size
    idx = np.asarray(idx, np.int64).reshape(-1)
    lo, hi = np.maximum(idx - L + 1, 0), np.minimum(idx, n - 1)         # the chain of output i: jj = lo .. hi
    acc = np.zeros(idx.size, np.float32)
    steps = int((hi - lo).max()) + 1 if idx.size and n else 0
    for t in range(max(steps, 0)):
        jj = lo + t
        on = jj <= hi
        j = np.where(on, jj, 0)
        term = np.where(on, h64[np.clip(idx - j, 0, L - 1)] * x64[j], 0.0)
        acc = np.where(on, (acc.astype(np.float64) + term).astype(np.float32), acc)
    return acc


def dot64(x, h, m):
    """(float64 y[0 .. m - 1], bound): the exact-input dot product in float64 and (terms + 1) 2^-24 sum |h x| per output."""
    x64, h64 = decode(x).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
    n, L = x64.size, h64.size
    y, mag = np.zeros(m), np.zeros(m)
    if n and m:
        full, fmag = np.convolve(x64, h64), np.convolve(np.abs(x64), np.abs(h64))
        k = min(m, full.size)
        y[:k], mag[:k] = full[:k], fmag[:k]
    i = np.arange(m, dtype=np.int64)
    terms = np.maximum(np.minimum(i, n - 1) - np.maximum(i - L + 1, 0) + 1, 0)
    return y, (terms + 1) * 2.0 ** -24 * mag


def np_pcm(y):
    """tcr_mine_gather's rounding: clamp(rint(y * 32768), -32768, 32767), ties to even."""
    return np.clip(np.rint(np.asarray(y, np.float32).astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def check_grid_argument(seed=0, outputs=8, taps=40):
    """The float64 step against rational arithmetic with one correctly rounded cast per term.  Returns the terms checked."""
    rng = np.random.RandomState(seed)
    checked = 0
    for _ in range(outputs):
        h = grid_response(rng, taps)
        x = rng.randint(-32768, 32768, taps).astype(np.int16)
        xs = decode(x)
        acc = np.float32(0)
        for k in range(taps):
            exact = Fraction(float(acc)) + Fraction(float(h[k])) * Fraction(float(xs[k]))
            step = np.float32(np.float64(acc) + np.float64(h[k]) * np.float64(xs[k]))
            assert Fraction(float(np.float64(acc) + np.float64(h[k]) * np.float64(xs[k]))) == exact        # the float64 step is exact
            # and float32(exact) is the nearest float32: its neighbours are no closer
            err = abs(Fraction(float(step)) - exact)
            for nb in (np.nextafter(step, np.float32(np.inf)), np.nextafter(step, np.float32(-np.inf))):
                assert err <= abs(Fraction(float(nb)) - exact)
            acc = step
            checked += 1
    return checked
