"""Reverberation on the device (tcr_reverb of include/tcresnet_hip.h): clip pools and whole recordings convolved with room impulse
responses, so that a composed corpus can vary the room as `Composer` varies the noise.

    irs = ImpulseResponses.synthetic(64, (0.2, 0.6), 16000, seed=1, device=dev)     # or .from_files(paths, 16000)
    wet = composer.reverberated(irs, probability=0.8, tail_ms=200, seed=2)          # a Composer over the wet int16 pool
    rec = wet.compose(wet.plan(64, 3600.0, scanner.step_samples, snr_db=(5, 20)))

    wet_signals = reverberate_signals(*rec.signals, irs, ir_index)                  # or: the room over clips and background together

Output i of a clip is one float32 fmaf chain over the input index ascending (the rule in the header), so a sample's bits do not
depend on the tile, the launch, the clip's neighbours or the buffers' layout; the int16 form is `mine`'s rounding of it, and the
response [1.0] reproduces an int16 clip byte for byte."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, runtime
from ._lib import TcrError
from .engine import _resolve
from .runtime import stream_of

TILE, STAGE, TAPS_MAX = _lib.REVERB_TILE, _lib.REVERB_STAGE, _lib.REVERB_TAPS_MAX


def _normalized(h: np.ndarray, normalize: Optional[str]) -> np.ndarray:
    h = np.asarray(h, np.float64).reshape(-1)
    if normalize == "energy":
        e = float(np.sum(h * h))
        if e > 0:
            h = h / math.sqrt(e)
    elif normalize == "peak":
        p = float(np.abs(h).max()) if h.size else 0.0
        if p > 0:
            h = h / p
    elif normalize is not None:
        raise TcrError(f"ImpulseResponses: normalize must be 'energy', 'peak' or None (got {normalize!r})")
    return h


class ImpulseResponses:
    """A bank of impulse responses: `data`, one float32 tensor on the device, and the host tables `offsets` / `lengths` (int64) of
    the responses in it.  Every response has 1 .. TAPS_MAX finite taps."""

    def __init__(self, data: torch.Tensor, offsets, lengths, lib: Optional[_lib.Library] = None):
        self.lib = lib if lib is not None else (runtime.default_lib() or _lib.get())
        self.data = data
        self.offsets = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
        self.lengths = np.ascontiguousarray(np.asarray(lengths, np.int64).reshape(-1))
        if data.dim() != 1 or data.dtype != torch.float32 or not data.is_contiguous():
            raise TcrError(f"ImpulseResponses: data must be a contiguous 1-D float32 tensor, got {data.dtype} {tuple(data.shape)}")
        if self.offsets.shape != self.lengths.shape or self.lengths.size < 1:
            raise TcrError(f"ImpulseResponses: {self.offsets.size} offsets for {self.lengths.size} lengths; at least one response")
        bad = np.flatnonzero((self.lengths < 1) | (self.lengths > TAPS_MAX))
        if bad.size:
            raise TcrError(f"ImpulseResponses: response {int(bad[0])} has {int(self.lengths[bad[0]])} taps; 1 .. {TAPS_MAX} are taken")
        if (self.offsets < 0).any() or (self.offsets + self.lengths > int(data.shape[0])).any():
            raise TcrError(f"ImpulseResponses: a response lies outside the bank's {int(data.shape[0])} floats")

    def __len__(self) -> int:
        return int(self.lengths.size)

    @property
    def device(self):
        return self.data.device

    def numpy(self) -> List[np.ndarray]:
        """The responses as host float32 arrays."""
        flat = self.data.cpu().numpy()
        return [flat[o:o + n].copy() for o, n in zip(self.offsets, self.lengths)]

    @classmethod
    def from_arrays(cls, responses: Sequence, normalize: Optional[str] = "energy", device=None, lib: Optional[_lib.Library] = None):
        """One response per array.  normalize: "energy" scales each to sum h^2 == 1 (in float64, cast once: a clip keeps its expected
        power), "peak" to max |h| == 1, None leaves them."""
        lib, dev = _resolve(lib if lib is not None else runtime.default_lib(), device if device is not None else runtime.default_device())
        hs = [_normalized(h, normalize) for h in responses]
        if not hs:
            raise TcrError("ImpulseResponses: at least one response")
        for r, h in enumerate(hs):
            if not 1 <= h.size <= TAPS_MAX:
                raise TcrError(f"ImpulseResponses: response {r} has {h.size} taps; 1 .. {TAPS_MAX} are taken")
            if not np.isfinite(h).all():
                raise TcrError(f"ImpulseResponses: response {r} has taps that are not finite")
        lengths = np.array([h.size for h in hs], np.int64)
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        flat = np.concatenate(hs).astype(np.float32)
        if not np.isfinite(flat).all():
            raise TcrError("ImpulseResponses: a tap does not fit float32")
        return cls(torch.from_numpy(flat).to(dev), offsets, lengths, lib)

    @classmethod
    def dry(cls, device=None, lib: Optional[_lib.Library] = None):
        """The bank of the single response [1.0]."""
        return cls.from_arrays([np.ones(1)], normalize=None, device=device, lib=lib)

    @classmethod
    def from_files(cls, paths: Sequence[str], sample_rate: int, max_ms: Optional[float] = None, normalize: Optional[str] = "energy",
                   device=None, lib: Optional[_lib.Library] = None):
        """16-bit PCM WAV files (channel 0, through the package's `WavFile`); a file at another rate goes through
        `resampling.Resampler` first.  Everything ahead of the largest |h| is dropped, so the direct path sits at tap 0 and a wet
        clip's onset is the dry clip's; the rest is cut to max_ms (if given) and to TAPS_MAX taps."""
        from .audio_input import WavFile
        from .resampling import Resampler
        lib, dev = _resolve(lib if lib is not None else runtime.default_lib(), device if device is not None else runtime.default_device())
        sr = int(sample_rate)
        cap = TAPS_MAX if max_ms is None else max(1, min(TAPS_MAX, int(float(max_ms) * sr / 1000.0)))
        hs = []
        for path in paths:
            f = WavFile(path)
            if f.length < 1:
                raise TcrError(f"ImpulseResponses.from_files: {path} has no samples")
            pcm = f.read_pcm(0, f.length)
            if f.rate != sr:
                rs = Resampler(f.rate, sr, 1, device=dev, lib=lib)
                h = rs.resample(torch.from_numpy(pcm).to(dev).reshape(1, -1)).reshape(-1).cpu().numpy().astype(np.float64)
            else:
                h = pcm.astype(np.float64) / 32768.0
            if not np.abs(h).max() > 0:
                raise TcrError(f"ImpulseResponses.from_files: {path} is silent")
            at = int(np.argmax(np.abs(h)))
            hs.append(h[at:at + cap])
        return cls.from_arrays(hs, normalize=normalize, device=dev, lib=lib)

    @classmethod
    def synthetic(cls, count: int, rt60, sample_rate: int, seed: int = 0, drr_db: float = 6.0, normalize: Optional[str] = "energy",
                  device=None, lib: Optional[_lib.Library] = None):
        """`count` responses of exponentially decaying Gaussian noise behind a unit direct path.  rt60 (seconds): a number, or (lo, hi)
        drawn uniformly per response from np.random.default_rng(seed).  L = min(TAPS_MAX, ceil(rt60 sr)); h[0] = 1,
        h[t >= 1] = c N(0, 1) 10^(-3 t / (rt60 sr)) -- 60 dB down at t = rt60 sr -- with c such that the direct energy over the
        reverberant energy is drr_db.  Float64, normalised, cast once to float32."""
        rng = np.random.default_rng(seed)
        sr, count = int(sample_rate), int(count)
        lo, hi = (float(rt60), float(rt60)) if np.ndim(rt60) == 0 else (float(rt60[0]), float(rt60[1]))
        if count < 1 or sr < 1 or not (0 < lo <= hi) or not math.isfinite(hi) or not math.isfinite(float(drr_db)):
            raise TcrError(f"ImpulseResponses.synthetic: count {count}, rt60 {rt60}, sample_rate {sr}, drr_db {drr_db}: count and rate "
                           "positive, 0 < rt60 (lo <= hi), finite")
        hs = []
        for _ in range(count):
            t60 = rng.uniform(lo, hi) if hi > lo else lo
            L = max(1, min(TAPS_MAX, int(math.ceil(t60 * sr))))
            h = np.zeros(L, np.float64)
            h[0] = 1.0
            if L > 1:
                t = np.arange(1, L, dtype=np.float64)
                tail = rng.standard_normal(L - 1) * 10.0 ** (-3.0 * t / (t60 * sr))
                e = float(np.sum(tail * tail))
                if e > 0:
                    h[1:] = tail * math.sqrt(10.0 ** (-float(drr_db) / 10.0) / e)
            hs.append(h)
        return cls.from_arrays(hs, normalize=normalize, device=device, lib=lib)


def _tables(n_in: np.ndarray, taps: np.ndarray, tail) -> np.ndarray:
    """Output lengths: n + min(L - 1, tail) (tail None: the whole L - 1); an empty clip stays empty."""
    room = taps - 1 if tail is None else np.minimum(taps - 1, int(tail))
    return np.where(n_in > 0, n_in + room, 0).astype(np.int64)


def reverb(lib, data: torch.Tensor, in_off, in_len, irs: ImpulseResponses, clip_ir, out_len, floats: bool = True, pcm: bool = False):
    """The raw form of tcr_reverb: clip j, the in_len[j] samples of `data` (1-D int16 or float32) from in_off[j] on, under response
    clip_ir[j] of `irs`, out_len[j] outputs each -> (packed float32 or None, packed int16 or None, out_off int64 [n + 1])."""
    if not (floats or pcm):
        raise TcrError("reverb: neither floats nor pcm asked for")
    if data.dim() != 1 or data.dtype not in (torch.int16, torch.float32) or not data.is_contiguous():
        raise TcrError(f"reverb: expected a contiguous 1-D int16 or float32 tensor, got {data.dtype} {tuple(data.shape)}")
    dev = data.device
    if irs.data.device != dev:
        raise TcrError(f"reverb: the responses are on {irs.data.device}, the audio on {dev}")
    arr = lambda x, dt: np.ascontiguousarray(np.asarray(x, dt).reshape(-1))
    in_off, in_len, clip_ir, out_len = arr(in_off, np.int64), arr(in_len, np.int64), arr(clip_ir, np.int64), arr(out_len, np.int64)
    n = int(in_off.size)
    if not (in_len.size == clip_ir.size == out_len.size == n):
        raise TcrError(f"reverb: {n} offsets for {in_len.size} lengths, {clip_ir.size} responses and {out_len.size} output lengths")
    size = int(data.shape[0])
    if n and ((in_len < 0).any() or (in_off < 0).any() or (in_off + in_len > size).any()):
        raise TcrError(f"reverb: clips outside the audio's {size} samples")
    if n and ((clip_ir < 0).any() or (clip_ir >= len(irs)).any()):
        bad = int(np.flatnonzero((clip_ir < 0) | (clip_ir >= len(irs)))[0])
        raise TcrError(f"reverb: clip {bad} asks for response {int(clip_ir[bad])} of a bank of {len(irs)}")
    if n and (out_len < 0).any():
        raise TcrError("reverb: a negative output length")
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(out_len, out=out_off[1:])
    tile_off = np.zeros(n + 1, np.int64)
    np.cumsum((out_len + TILE - 1) // TILE, out=tile_off[1:])
    total = int(out_off[-1])
    out = torch.empty(total, dtype=torch.float32, device=dev) if floats else None
    out_pcm = torch.empty(total, dtype=torch.int16, device=dev) if pcm else None
    if total > 0:
        up = lambda a: torch.from_numpy(a).to(dev)
        keep = [up(in_off), up(in_len), up(irs.offsets), up(irs.lengths.astype(np.int32)), up(clip_ir.astype(np.int32)), up(out_off), up(tile_off)]
        p = lambda t: None if t is None else t.data_ptr()
        lib.check(lib.tcr_reverb(n, data.data_ptr(), 1 if data.dtype == torch.int16 else 0, size, keep[0].data_ptr(), keep[1].data_ptr(),
                                 irs.data.data_ptr(), int(irs.data.shape[0]), keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(),
                                 keep[5].data_ptr(), keep[6].data_ptr(), int(tile_off[-1]), p(out), p(out_pcm), stream_of(dev)), "tcr_reverb")
    return out, out_pcm, out_off


def _with_dry(irs: ImpulseResponses, ir_index) -> Tuple[ImpulseResponses, np.ndarray]:
    """ir_index with -1 (dry) mapped onto a response [1.0] appended to the bank."""
    idx = np.asarray(ir_index, np.int64).reshape(-1).copy()
    if (idx < -1).any() or (idx >= len(irs)).any():
        bad = int(np.flatnonzero((idx < -1) | (idx >= len(irs)))[0])
        raise TcrError(f"reverberate: clip {bad} asks for response {int(idx[bad])} of a bank of {len(irs)} (-1: dry)")
    if not (idx == -1).any():
        return irs, idx
    one = torch.ones(1, dtype=torch.float32, device=irs.data.device)
    bank = ImpulseResponses(torch.cat([irs.data, one]), np.append(irs.offsets, int(irs.data.shape[0])), np.append(irs.lengths, 1), irs.lib)
    idx[idx == -1] = len(irs)
    return bank, idx


def reverberate(pool, irs: ImpulseResponses, ir_index, tail_ms: Optional[float] = None, sample_rate: int = 16000):
    """A new int16 pool on the pool's device: clip j convolved with response ir_index[j] (-1: the dry response [1.0]) and
    lengthened by min(L - 1, tail) samples, tail = tail_ms at sample_rate (None: the whole response).  Written on the device
    without a host trip; a valid pool for `Composer` and the training input stage."""
    from .datasets.augmentation_factory import PcmPool
    n = len(pool)
    bank, idx = _with_dry(irs, ir_index)
    if idx.size != n:
        raise TcrError(f"reverberate: {idx.size} responses for {n} clips")
    tail = None
    if tail_ms is not None:
        if not float(tail_ms) >= 0:
            raise TcrError(f"reverberate: tail_ms must be >= 0 (got {tail_ms})")
        tail = int(float(tail_ms) * int(sample_rate) / 1000.0)
    lengths = np.asarray(pool.lengths, np.int64)
    out_len = _tables(lengths, bank.lengths[idx] if n else np.zeros(0, np.int64), tail)
    wet = PcmPool.__new__(PcmPool)
    wet.lib, wet.device = pool.lib, pool.data.device
    wet.lengths = out_len
    wet.offsets = (np.concatenate([[0], np.cumsum(out_len)[:-1]]) if n else np.zeros(0)).astype(np.int64)
    _, pcm, _ = reverb(pool.lib, pool.data, pool.offsets, lengths, bank, idx, out_len, floats=False, pcm=True)
    wet.data = pcm if int(pcm.shape[0]) else torch.zeros(1, dtype=torch.int16, device=wet.device)
    return wet


def reverberate_signals(packed: torch.Tensor, lengths, irs: ImpulseResponses, ir_index, tail: bool = False, lib=None):
    """Whole float32 recordings (for example `ComposedRecordings.signals`): recording j convolved with response ir_index[j] (-1:
    dry) -> (packed float32, lengths).  tail=False keeps every recording's length (what `scan_ragged` needs to stay on whole steps);
    tail=True appends the L - 1 samples of the response's tail."""
    if packed.dtype != torch.float32:
        raise TcrError(f"reverberate_signals: expected packed float32, got {packed.dtype}")
    lens = np.asarray(lengths, np.int64).reshape(-1)
    bank, idx = _with_dry(irs, ir_index)
    if idx.size != lens.size:
        raise TcrError(f"reverberate_signals: {idx.size} responses for {lens.size} recordings")
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if lens.size else np.zeros(0, np.int64)
    out_len = _tables(lens, bank.lengths[idx], None) if tail else lens
    out, _, _ = reverb(lib if lib is not None else irs.lib, packed, off, lens, bank, idx, out_len, floats=True, pcm=False)
    return out, out_len


def draw_responses(n_clips: int, n_responses: int, probability: float = 1.0, seed: int = 0) -> np.ndarray:
    """Per clip a response drawn uniformly from the bank, or -1 (dry) at probability 1 - p, from np.random.default_rng(seed)."""
    if not 0.0 <= float(probability) <= 1.0:
        raise TcrError(f"reverberated: probability must be in [0, 1] (got {probability})")
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_responses, int(n_clips)).astype(np.int64)
    wet = rng.random(int(n_clips)) < float(probability)
    return np.where(wet, idx, -1)
