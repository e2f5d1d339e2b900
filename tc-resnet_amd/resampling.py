"""Sample-rate conversion on the device (tcr_resample of include/tcresnet_hip.h): int16 PCM or float32 at any rate in, the float32
at the model's rate that the detectors take out.

in_rate -> out_rate, g = gcd, L = out_rate / g (up), M = in_rate / g (down), scale = max(1, M / L).  `design_table` builds the
polyphase filter on the host in float64 (a Kaiser-windowed sinc, unit DC gain in every phase) and rounds it once to float32 [L, P];
output j is one fmaf chain over the P taps of phase (j M) mod L from input floor(j M / L) - P / 2 + 1 on, zeros outside the signal.
Every output is a pure function of its global index (64-bit positions), so converting a signal in chunks (`convert` over any split of
the outputs, or `push` ... `flush` over any split of the inputs) is bitwise converting it at once (`resample`).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, runtime
from ._lib import TcrError
from .engine import _resolve


def design_table(in_rate: int, out_rate: int, zero_crossings: int = 32, beta: float = 8.6, rolloff: float = 0.915
                 ) -> Tuple[int, int, np.ndarray]:
    """(L, M, table float32 [L, P]).  P = 2 ceil(zero_crossings * scale) taps per phase; for phase phi and tap p, tau = (p - P / 2 + 1)
    - phi / L input samples, fc = rolloff / scale, c = fc sinc(fc tau) kaiser(tau / (zero_crossings * scale); beta); every phase row is
    divided by its float64 sum, then rounded to float32.  Equal rates: L = M = P = 1 and the table is the single value 1."""
    in_rate, out_rate = int(in_rate), int(out_rate)
    if in_rate < 1 or out_rate < 1:
        raise ValueError(f"sample rates must be positive (got {in_rate} -> {out_rate})")
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    if L == M:
        return 1, 1, np.ones((1, 1), np.float32)
    scale = max(1.0, M / L)
    half = zero_crossings * scale
    P = 2 * int(math.ceil(half))
    fc = rolloff / scale
    tau = (np.arange(P, dtype=np.float64) - P // 2 + 1)[None, :] - (np.arange(L, dtype=np.float64) / L)[:, None]
    u = tau / half
    window = np.where(np.abs(u) <= 1.0, np.i0(beta * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(beta), 0.0)
    c = fc * np.sinc(fc * tau) * window
    c /= c.sum(axis=1, keepdims=True)
    return L, M, c.astype(np.float32)


def _ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


class Resampler:
    """Converts n_streams signals from in_rate to out_rate on `device`.  dtype: torch.int16 (PCM, decoded as v / 32768) or
    torch.float32; channels > 1: the input is interleaved [S, n, channels] and channel 0 is read.  **design: `design_table`'s
    zero_crossings, beta, rolloff."""

    def __init__(self, in_rate: int, out_rate: int, n_streams: int, device=None, dtype: torch.dtype = torch.int16, channels: int = 1,
                 lib: Optional[_lib.Library] = None, **design):
        if dtype not in (torch.int16, torch.float32):
            raise TcrError(f"Resampler: dtype must be torch.int16 or torch.float32 (got {dtype})")
        if n_streams < 1 or channels < 1:
            raise TcrError(f"Resampler: n_streams and channels must be >= 1 (got {n_streams}, {channels})")
        self.lib, self.device = _resolve(lib if lib is not None else runtime.default_lib(),
                                         device if device is not None else runtime.default_device())
        self.in_rate, self.out_rate, self.n_streams, self.dtype, self.channels = int(in_rate), int(out_rate), int(n_streams), dtype, int(channels)
        self.up, self.down, table = design_table(in_rate, out_rate, **design)
        self.taps = int(table.shape[1])
        self.lead = self.taps // 2 - 1 if self.taps > 1 else 0
        self.table = torch.from_numpy(table).to(self.device)
        self.cfg = _lib.ResampleCfg(self.up, self.down, self.taps, 1 if dtype == torch.int16 else 0, self.channels)
        self.reset()

    def _stream(self):
        return runtime.stream_of(self.device)

    # ---- positions (host integers) ----------------------------------------------------------------------------------------------
    def out_length(self, n_in: int) -> int:
        """Outputs of a signal of n_in samples: ceil(n_in L / M)."""
        return _ceil_div(int(n_in) * self.up, self.down)

    def span(self, out_first: int, n_out: int) -> Tuple[int, int]:
        """(first, n): the input samples [first, first + n) that outputs [out_first, out_first + n_out) read (tcr_resample_span)."""
        first, n = C.c_int64(), C.c_int64()
        self.lib.check(self.lib.tcr_resample_span(C.byref(self.cfg), int(out_first), int(n_out), C.byref(first), C.byref(n)),
                       "tcr_resample_span")
        return int(first.value), int(n.value)

    # ---- the stateless call -----------------------------------------------------------------------------------------------------
    def _rows(self, x: torch.Tensor, what: str) -> Tuple[int, int, int]:
        """(S, n, pitch) of x [S, n] (channels == 1) or [S, n, channels]: rows of interleaved samples, any row pitch."""
        ok = x.dim() == 2 + (self.channels > 1) and x.dtype == self.dtype and x.device.type == self.device.type
        if ok and self.channels > 1:
            ok = x.shape[2] == self.channels and (x.shape[1] == 0 or (x.stride(2) == 1 and x.stride(1) == self.channels))
        elif ok:
            ok = x.shape[1] <= 1 or x.stride(1) == 1
        if not ok:
            shape = "[S, n, %d]" % self.channels if self.channels > 1 else "[S, n]"
            raise TcrError(f"{what}: expected {self.dtype} {shape} on {self.device} with contiguous rows, got {x.dtype} "
                           f"{tuple(x.shape)} (strides {tuple(x.stride())}) on {x.device}")
        S, n = int(x.shape[0]), int(x.shape[1])
        return S, n, (int(x.stride(0)) if S > 1 else max(int(x.stride(0)), n * self.channels))

    def convert(self, x: torch.Tensor, in_first: int, out_first: int, n_out: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Outputs [out_first, out_first + n_out) of every row of x, whose first sample has global index in_first (samples outside x
        read as zeros) -> float32 [S, n_out].  `out`: a float32 [S, n_out] tensor or view with contiguous rows to write into."""
        S, n, pitch = self._rows(x, "convert")
        n_out = int(n_out)
        if out is None:
            out = torch.empty((S, max(n_out, 0)), dtype=torch.float32, device=self.device)
        elif (out.dim() != 2 or out.dtype != torch.float32 or out.device.type != self.device.type or tuple(out.shape) != (S, n_out)
              or (n_out > 1 and out.stride(1) != 1)):
            raise TcrError(f"convert: out must be float32 [{S}, {n_out}] on {self.device} with contiguous rows")
        if n_out == 0:
            return out
        out_pitch = int(out.stride(0)) if S > 1 else max(int(out.stride(0)), n_out)
        self.lib.check(self.lib.tcr_resample(C.byref(self.cfg), self.table.data_ptr(), S, x.data_ptr(), pitch, int(in_first), n,
                                             int(out_first), n_out, out.data_ptr(), out_pitch, self._stream()), "tcr_resample")
        return out

    def resample(self, x: torch.Tensor) -> torch.Tensor:
        """Whole signals [S, N_in] (or [S, N_in, channels]) -> float32 [S, ceil(N_in L / M)]."""
        return self.convert(x, 0, 0, self.out_length(int(x.shape[1])))

    # ---- live audio -------------------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """Every stream starts over: nothing pushed, nothing returned."""
        self._hist: Optional[torch.Tensor] = None        # the last inputs, [S, <= taps] (+ channels)
        self._n_in = 0                                   # samples pushed so far
        self._n_out = 0                                  # outputs returned so far
        self._flushed = False

    def _available(self) -> int:
        """Outputs whose taps have all arrived: those with floor(j M / L) - lead + taps - 1 <= n_in - 1."""
        t = self._n_in - self.taps + self.lead
        return _ceil_div((t + 1) * self.up, self.down) if t >= 0 else 0

    def push(self, x: torch.Tensor) -> torch.Tensor:
        """The next samples of every stream, [n_streams, n] (or [n_streams, n, channels]), n >= 0 -> every output whose taps have all
        arrived and that no earlier push returned, float32 [n_streams, m] (m from host integers: no synchronisation)."""
        S, n, _ = self._rows(x, "push")
        if S != self.n_streams:
            raise TcrError(f"push: expected {self.n_streams} streams, got {S}")
        if self._flushed:
            raise TcrError("push after flush: call reset() to start new streams")
        buf = x if self._hist is None else torch.cat([self._hist, x], dim=1)
        in_first = self._n_in - (0 if self._hist is None else int(self._hist.shape[1]))
        self._n_in += n
        avail = max(self._available(), self._n_out)
        out = self.convert(buf, in_first, self._n_out, avail - self._n_out)
        self._n_out = avail
        self._hist = buf[:, max(0, int(buf.shape[1]) - self.taps):].clone()
        return out

    def flush(self) -> torch.Tensor:
        """The remaining outputs, up to out_length(samples pushed), with the samples that never came read as zeros."""
        if self._flushed:
            raise TcrError("flush called twice: call reset() to start new streams")
        self._flushed = True
        total = self.out_length(self._n_in)
        if self._hist is None:
            return torch.empty((self.n_streams, 0), dtype=torch.float32, device=self.device)
        out = self.convert(self._hist, self._n_in - int(self._hist.shape[1]), self._n_out, total - self._n_out)
        self._n_out = total
        return out
