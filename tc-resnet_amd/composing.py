"""Labelled test recordings composed on the device (tcr_compose, tcr_pcm_energy): the "streaming accuracy" corpus of a keyword
spotter -- dataset clips pasted at known times onto looping background noise -- written straight into the packed layout
`KeywordScanner.scan_ragged` takes, with the events `sweep` / `tune` / `mine` take.

    composer = Composer.from_dataset(wrapper)                       # the pools the training input stage already holds
    plan = composer.plan(64, 3600.0, scanner.step_samples, snr_db=(5, 20), seed=1)
    rec = composer.compose(plan)                                    # one launch; nothing crosses the host but the small tables
    out = scanner.scan_ragged(rec.signals)
    curve = scanner.sweep(out, thresholds, events=rec.events).curve(keywords)

The rule per sample is the input stage's (`datasets.augmentation_factory`, tcr_augment_fwd), see include/tcresnet_hip.h: the clip
times its gain, the background times its volume added in float32, clipped to [-1, 1].  A plan is host tables only, drawn from one
seeded NumPy generator; `CompositionPlan` also takes hand-made tables."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TcrError
from .runtime import stream_of


def pcm_energy(data: torch.Tensor, offsets, lengths, lib=None) -> torch.Tensor:
    """The raw form of tcr_pcm_energy: int64 [n] on data's device, the sum of v * v over the `lengths[j]` samples of the int16 pool
    `data` from `offsets[j]` on.  Exact integer sums."""
    if lib is None:
        lib = _lib.get()
    if data.dim() != 1 or data.dtype != torch.int16 or not data.is_contiguous():
        raise TcrError(f"pcm_energy expects a contiguous 1-D int16 pool, got {data.dtype} {tuple(data.shape)}")
    off, lens = np.asarray(offsets, np.int64).reshape(-1), np.asarray(lengths, np.int64).reshape(-1)
    if off.shape != lens.shape:
        raise TcrError(f"pcm_energy: {off.size} offsets for {lens.size} lengths")
    if off.size and ((lens < 0).any() or (off < 0).any() or (off + lens > int(data.shape[0])).any()):
        raise TcrError(f"pcm_energy: clips outside the pool's {int(data.shape[0])} samples")
    dev = data.device
    out = torch.zeros(off.size, dtype=torch.int64, device=dev)
    if off.size:
        d_off, d_len = torch.from_numpy(np.ascontiguousarray(off)).to(dev), torch.from_numpy(np.ascontiguousarray(lens)).to(dev)
        lib.check(lib.tcr_pcm_energy(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), int(off.size), out.data_ptr(), stream_of(dev)),
                  "tcr_pcm_energy")
    return out


class CompositionPlan:
    """The host tables of one tcr_compose call (see include/tcresnet_hip.h) and the events they imply.

    lengths int64 [N] (samples per recording); place_offsets int32 [N + 1], the CSR over the placements; per placement
    place_clip_off int64 (the pool index of the clip's first sample), place_len int32, place_first int64 (the recording's sample
    where the clip starts; it may be negative or run past the end: the part outside is dropped), place_gain float32, place_label
    int64 (the clip's class); per recording bg_off / bg_len / bg_phase int64 and bg_vol float32, or bg_vol None: no background.
    Refused: placements of a recording that are not sorted by place_first and disjoint, negative lengths, a gain or volume that is
    not finite, a background of bg_vol != 0 with bg_len < 1 or a phase outside 0 .. bg_len - 1.

    events: per recording, one (start_ms, end_ms, label) per placed clip that has samples inside the recording -- its extent there
    after cropping, [first sample, one past the last) in float64 ms, label the class index: what `KeywordScanner.sweep`, `tune` and
    `mine` take."""

    def __init__(self, sample_rate: int, lengths, place_offsets, place_clip_off, place_len, place_first, place_gain, place_label,
                 bg_off=None, bg_len=None, bg_phase=None, bg_vol=None):
        arr = lambda x, dt: np.ascontiguousarray(np.asarray(x, dtype=dt).reshape(-1))
        self.sample_rate = int(sample_rate)
        self.lengths, self.place_offsets = arr(lengths, np.int64), arr(place_offsets, np.int32)
        self.place_clip_off, self.place_len, self.place_first = arr(place_clip_off, np.int64), arr(place_len, np.int32), arr(place_first, np.int64)
        self.place_gain, self.place_label = arr(place_gain, np.float32), arr(place_label, np.int64)
        N, off = int(self.lengths.size), self.place_offsets
        if N < 1 or (self.lengths < 0).any():
            raise TcrError(f"CompositionPlan: {N} recordings of lengths {self.lengths.tolist()[:8]}: at least one, none negative")
        if off.size != N + 1 or off[0] != 0 or (np.diff(off) < 0).any():
            raise TcrError(f"CompositionPlan: place_offsets must be [{N + 1}], from 0, non-decreasing")
        P = int(off[-1])
        for name in ("place_clip_off", "place_len", "place_first", "place_gain", "place_label"):
            if getattr(self, name).size != P:
                raise TcrError(f"CompositionPlan: {name} has {getattr(self, name).size} entries for {P} placements")
        self.place_recording = np.repeat(np.arange(N, dtype=np.int64), np.diff(off))
        bad = np.flatnonzero(self.place_len < 0)
        if bad.size:
            raise TcrError(f"CompositionPlan: recording {int(self.place_recording[bad[0]])}: placement {int(bad[0])} has a negative length")
        bad = np.flatnonzero(~np.isfinite(self.place_gain))
        if bad.size:
            raise TcrError(f"CompositionPlan: recording {int(self.place_recording[bad[0]])}: placement {int(bad[0])} has a gain that is not "
                           f"finite ({self.place_gain[bad[0]]})")
        if P > 1:
            end = self.place_first + self.place_len
            bad = np.flatnonzero((end[:-1] > self.place_first[1:]) & (self.place_recording[:-1] == self.place_recording[1:]))
            if bad.size:
                j = int(bad[0])
                raise TcrError(f"CompositionPlan: recording {int(self.place_recording[j])}: placements {j} (samples {int(self.place_first[j])} .. "
                               f"{int(end[j]) - 1}) and {j + 1} (from {int(self.place_first[j + 1])}) overlap or are not sorted")
        self.bg_vol = None if bg_vol is None else arr(bg_vol, np.float32)
        self.bg_off = self.bg_len = self.bg_phase = None
        if self.bg_vol is not None:
            if bg_off is None or bg_len is None or bg_phase is None:
                raise TcrError("CompositionPlan: bg_vol needs bg_off, bg_len and bg_phase")
            self.bg_off, self.bg_len, self.bg_phase = arr(bg_off, np.int64), arr(bg_len, np.int64), arr(bg_phase, np.int64)
            for name in ("bg_vol", "bg_off", "bg_len", "bg_phase"):
                if getattr(self, name).size != N:
                    raise TcrError(f"CompositionPlan: {name} has {getattr(self, name).size} entries for {N} recordings")
            bad = np.flatnonzero(~np.isfinite(self.bg_vol))
            if bad.size:
                raise TcrError(f"CompositionPlan: recording {int(bad[0])}: a background volume that is not finite ({self.bg_vol[bad[0]]})")
            on = self.bg_vol != 0
            bad = np.flatnonzero(on & ((self.bg_len < 1) | (self.bg_phase < 0) | (self.bg_phase >= self.bg_len)))
            if bad.size:
                n = int(bad[0])
                raise TcrError(f"CompositionPlan: recording {n}: background of {int(self.bg_len[n])} samples at phase {int(self.bg_phase[n])}: "
                               "bg_len >= 1 and 0 <= bg_phase < bg_len")
        self.sample_offsets = np.zeros(N + 1, np.int64)
        np.cumsum(self.lengths, out=self.sample_offsets[1:])

    @property
    def n_recordings(self) -> int:
        return int(self.lengths.size)

    @property
    def total_samples(self) -> int:
        return int(self.sample_offsets[-1])

    def extents(self) -> Tuple[np.ndarray, np.ndarray]:
        """Per placement, its samples inside its recording after cropping: (first, one past the last); empty where last <= first."""
        lo = np.maximum(self.place_first, 0)
        hi = np.minimum(self.place_first + self.place_len, self.lengths[self.place_recording])
        return lo, hi

    @property
    def events(self) -> List[List[Tuple[float, float, int]]]:
        lo, hi = self.extents()
        out: List[List[Tuple[float, float, int]]] = [[] for _ in range(self.n_recordings)]
        for j in np.flatnonzero(hi > lo):
            out[int(self.place_recording[j])].append((1000.0 * float(lo[j]) / self.sample_rate, 1000.0 * float(hi[j]) / self.sample_rate,
                                                      int(self.place_label[j])))
        return out


class ComposedRecordings:
    """What `Composer.compose` returns: signals = (packed float32 on the device, lengths) as `scan_ragged` / `scan_steps` / `mine`
    take them (None with floats=False), pcm the packed int16 (None without pcm=True), and the plan's events and lengths."""

    def __init__(self, packed: Optional[torch.Tensor], pcm: Optional[torch.Tensor], plan: CompositionPlan, label_names: Sequence[str]):
        self.plan, self.pcm, self.label_names = plan, pcm, list(label_names)
        self.lengths, self.events, self.sample_rate = plan.lengths, plan.events, plan.sample_rate
        self.signals = None if packed is None else (packed, plan.lengths)

    def write_wavs(self, directory: str, prefix: str = "rec") -> List[str]:
        """DIR/<prefix>_<n>.wav, 16-bit mono (the int16 output: needs compose(..., pcm=True)), and DIR/events.csv with the header
        file,start_ms,end_ms,label -- label NAMES, files spelled as the paths returned here, which is how a later
        `sweep_audio.py --wav DIR/*.wav --events DIR/events.csv` spells them.  Returns the WAV paths."""
        from .audio_input import write_wav
        if self.pcm is None:
            raise TcrError("ComposedRecordings.write_wavs: composed without pcm=True")
        os.makedirs(directory, exist_ok=True)
        pcm, off = self.pcm.cpu().numpy(), self.plan.sample_offsets
        width = max(4, len(str(len(self.lengths) - 1)))
        paths = [os.path.join(directory, f"{prefix}_{n:0{width}d}.wav") for n in range(len(self.lengths))]
        for n, path in enumerate(paths):
            write_wav(path, pcm[off[n]:off[n + 1]], self.sample_rate)
        with open(os.path.join(directory, "events.csv"), "w", newline="") as fh:
            fh.write("file,start_ms,end_ms,label\n")
            for path, evs in zip(paths, self.events):
                for start, end, label in evs:
                    fh.write(f"{path},{start!r},{end!r},{self.label_names[label]}\n")
        return paths


class Composer:
    """Composes recordings from `pool` (a `datasets.augmentation_factory.PcmPool` of clips; a `MinedClips.to_pool()` works), `labels`
    (one class index per clip), `label_names` and optionally `background` (a PcmPool of noise recordings), all on one device."""

    def __init__(self, pool, labels, label_names: Sequence[str], background=None, sample_rate: int = 16000, device=None):
        self.pool, self.background, self.sample_rate = pool, background, int(sample_rate)
        self.lib, self.device = pool.lib, pool.data.device              # (the tensor's: it carries the device index)
        want = None if device is None else torch.device(device)
        if want is not None and (want.type != self.device.type or (want.index is not None and want.index != self.device.index)):
            raise TcrError(f"Composer: the pool is on {self.device}, not on {want}")
        if background is not None and background.data.device != self.device:
            raise TcrError(f"Composer: the background pool is on {background.data.device}, the clips on {self.device}")
        self.labels = np.asarray(labels, dtype=np.int64).reshape(-1)
        self.label_names = [str(x) for x in label_names]
        if self.labels.size != len(pool):
            raise TcrError(f"Composer: {self.labels.size} labels for {len(pool)} clips")
        if self.labels.size and (self.labels.min() < 0 or self.labels.max() >= len(self.label_names)):
            raise TcrError(f"Composer: labels outside 0..{len(self.label_names) - 1}")
        self._energies = None

    @classmethod
    def from_dataset(cls, wrapper) -> "Composer":
        """Everything from a `SingleLabelAudioDataWrapper`: its clip pool, labels, label names and background pool."""
        return cls(wrapper.pool, wrapper.labels, wrapper.label_names, wrapper.background, int(wrapper.args.sample_rate))

    def reverberated(self, irs, probability: float = 1.0, tail_ms: Optional[float] = None, seed: int = 0) -> "Composer":
        """A composer over the wet pool (`reverberation.reverberate`, on the device): the same labels, label names and background;
        every clip convolved with a response drawn uniformly from `irs` (an `ImpulseResponses`), or left dry at probability
        1 - probability, the draws from np.random.default_rng(seed) (`wet.ir_index`: the response per clip, -1 dry).  A wet clip is
        min(L - 1, tail_ms) samples longer than the dry one, and a plan's events cover that whole extent, tail included: a small
        tail_ms tightens the events to the audible part of the decay (None keeps the whole response).  `energies()` and snr_db act
        on the wet clips."""
        from .reverberation import draw_responses, reverberate
        idx = draw_responses(len(self.pool), len(irs), probability, seed)
        wet = Composer(reverberate(self.pool, irs, idx, tail_ms, self.sample_rate), self.labels, self.label_names, self.background,
                       self.sample_rate)
        wet.ir_index = idx
        return wet

    def energies(self) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """(per clip, per background recording or None) the int64 sums of squared samples (tcr_pcm_energy), computed once."""
        if self._energies is None:
            clip = pcm_energy(self.pool.data, self.pool.offsets, self.pool.lengths, self.lib).cpu().numpy()
            bg = self.background
            self._energies = (clip, None if bg is None else pcm_energy(bg.data, bg.offsets, bg.lengths, self.lib).cpu().numpy())
        return self._energies

    def plan(self, n_recordings: int, seconds, step_samples: int, min_gap_ms: float = 1500, max_gap_ms: float = 4000,
             classes: Optional[Sequence[int]] = None, foreground_gain: float = 1.0, background_volume: float = 0.1, snr_db=None,
             seed: int = 0) -> CompositionPlan:
        """n_recordings recordings of `seconds` (a number, or one per recording), each rounded down to a multiple of step_samples (the
        scanner's k * hop), so that the result goes into `scan_ragged` as it is.  Everything is drawn from np.random.default_rng(seed),
        recording by recording: the background recording and its phase (uniform; with a background pool and background_volume != 0),
        the first clip's start (uniform in 0 .. max_gap_ms), then clip, gap, clip, gap .. -- a clip uniform over the pool's non-empty
        clips whose label is in `classes` (None: every label), a gap uniform in min_gap_ms .. max_gap_ms (whole samples) after each
        clip -- for as long as the whole clip fits.  A clip's gain is foreground_gain, or with snr_db (a number, or (lo, hi): uniform
        per clip)  sqrt(10^(snr / 10) * vol^2 * bg_sumsq / bg_len * clip_len / clip_sumsq)  in float64 from the exact energies, cast
        to float32 (1 where the clip's energy is 0): the clip's mean power over the background's, scaled by the volume, is snr_db.

        min_gap_ms has to exceed the tolerance_ms used later: `sweep` refuses events closer than its tolerance (default 1000)."""
        rng = np.random.default_rng(seed)
        N, sr, step = int(n_recordings), self.sample_rate, int(step_samples)
        if N < 1 or step < 1:
            raise TcrError(f"plan: n_recordings {N} and step_samples {step} must be positive")
        if not float(min_gap_ms) > 0 or float(max_gap_ms) < float(min_gap_ms):
            raise TcrError(f"plan: gaps need 0 < min_gap_ms <= max_gap_ms (got {min_gap_ms}, {max_gap_ms})")
        gap_lo, gap_hi = int(np.ceil(float(min_gap_ms) * sr / 1000.0)), int(np.floor(float(max_gap_ms) * sr / 1000.0))
        if gap_hi < gap_lo:
            raise TcrError(f"plan: no whole number of samples between min_gap_ms {min_gap_ms} and max_gap_ms {max_gap_ms}")
        secs = np.broadcast_to(np.asarray(seconds, np.float64), (N,)) if np.ndim(seconds) == 0 else np.asarray(seconds, np.float64).reshape(-1)
        if secs.size != N or (secs < 0).any():
            raise TcrError(f"plan: seconds must be one value or {N} of them, none negative")
        lengths = np.floor(secs * sr).astype(np.int64) // step * step
        pool_len = np.asarray(self.pool.lengths, np.int64)
        ok = pool_len > 0
        if classes is not None:
            cls = np.asarray(list(classes), np.int64)
            if cls.size and (cls.min() < 0 or cls.max() >= len(self.label_names)):
                raise TcrError(f"plan: classes outside 0..{len(self.label_names) - 1}: {cls.tolist()}")
            ok &= np.isin(self.labels, cls)
        cand = np.flatnonzero(ok)
        if cand.size == 0:
            raise TcrError("plan: no clip with samples among the classes to draw from")
        vol = np.float32(background_volume)
        if not np.isfinite(vol) or not np.isfinite(np.float32(foreground_gain)):
            raise TcrError(f"plan: foreground_gain {foreground_gain} and background_volume {background_volume} must be finite")
        mixed = self.background is not None and len(self.background) > 0 and vol != 0
        if snr_db is not None:
            if not mixed:
                raise TcrError("plan: snr_db needs a background pool and a background_volume != 0")
            snr_lo, snr_hi = (float(snr_db), float(snr_db)) if np.ndim(snr_db) == 0 else (float(snr_db[0]), float(snr_db[1]))
            if not (np.isfinite(snr_lo) and np.isfinite(snr_hi) and snr_hi >= snr_lo):
                raise TcrError(f"plan: snr_db {snr_db} must be a finite number or (lo, hi) with hi >= lo")
            clip_sq, bg_sq = self.energies()
        bg_idx, bg_phase = np.zeros(N, np.int64), np.zeros(N, np.int64)
        clip, first, gain, counts = [], [], [], np.zeros(N + 1, np.int64)
        for n in range(N):
            if mixed:
                bg_idx[n] = rng.integers(len(self.background))
                bg_phase[n] = rng.integers(int(self.background.lengths[bg_idx[n]]))
            room = int(lengths[n]) // (gap_lo + 1) + 1                   # (a clip and its gap take more than gap_lo samples)
            at0 = int(rng.integers(0, gap_hi + 1))
            c = cand[rng.integers(0, cand.size, room)]
            gaps = rng.integers(gap_lo, gap_hi + 1, room)
            ln = pool_len[c]
            start = at0 + np.concatenate([[0], np.cumsum(ln + gaps)[:-1]])
            m = int(np.searchsorted(start + ln > int(lengths[n]), True))  # the clips in front of the first that does not fit whole
            c, start = c[:m], start[:m]
            if snr_db is not None:
                snr = rng.uniform(snr_lo, snr_hi, m) if snr_hi > snr_lo else np.full(m, snr_lo)
                b = int(bg_idx[n])
                power = 10.0 ** (snr / 10.0) * float(vol) ** 2 * (float(bg_sq[b]) / float(self.background.lengths[b]))
                with np.errstate(divide="ignore", invalid="ignore"):
                    g = np.sqrt(power * pool_len[c].astype(np.float64) / clip_sq[c].astype(np.float64))
                g = np.where(clip_sq[c] > 0, g, 1.0)
            else:
                g = np.full(m, float(foreground_gain))
            clip.append(c)
            first.append(start)
            gain.append(g.astype(np.float32))
            counts[n + 1] = counts[n] + m
        clip = np.concatenate(clip).astype(np.int64)
        bg = self.background
        plan = CompositionPlan(sr, lengths, counts.astype(np.int32), np.asarray(self.pool.offsets, np.int64)[clip], pool_len[clip],
                               np.concatenate(first), np.concatenate(gain), self.labels[clip],
                               *((np.asarray(bg.offsets, np.int64)[bg_idx], np.asarray(bg.lengths, np.int64)[bg_idx], bg_phase, np.full(N, vol))
                                 if mixed else ()))
        plan.place_clip, plan.bg_index = clip, bg_idx if mixed else None
        return plan

    def compose(self, plan: CompositionPlan, floats: bool = True, pcm: bool = False) -> ComposedRecordings:
        """One tcr_compose launch on the pool's device: the plan's tables go up, the packed float32 (`floats`) and / or int16 (`pcm`)
        recordings are written there."""
        if not (floats or pcm):
            raise TcrError("compose: neither floats nor pcm asked for")
        if plan.sample_rate != self.sample_rate:
            raise TcrError(f"compose: the plan is at {plan.sample_rate} Hz, the pools at {self.sample_rate} Hz")
        dev, lib, size = self.device, self.lib, int(self.pool.data.shape[0])
        used = plan.place_len > 0
        if ((plan.place_clip_off[used] < 0) | (plan.place_clip_off[used] + plan.place_len[used] > size)).any():
            raise TcrError(f"compose: a placement's clip lies outside the pool's {size} samples")
        mixed = plan.bg_vol is not None and bool((plan.bg_vol != 0).any())
        if mixed:
            if self.background is None:
                raise TcrError("compose: the plan has a background, the composer has no background pool")
            on, bsize = plan.bg_vol != 0, int(self.background.data.shape[0])
            if ((plan.bg_off[on] < 0) | (plan.bg_off[on] + plan.bg_len[on] > bsize)).any():
                raise TcrError(f"compose: a recording's background lies outside the background pool's {bsize} samples")
        total, N = plan.total_samples, plan.n_recordings
        out = torch.empty(total, dtype=torch.float32, device=dev) if floats else None
        out_pcm = torch.empty(total, dtype=torch.int16, device=dev) if pcm else None
        if total > 0:
            up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(dev)
            keep = [up(a) for a in (plan.sample_offsets, plan.place_offsets, plan.place_clip_off, plan.place_len, plan.place_first, plan.place_gain)]
            bgt = [up(a) for a in (plan.bg_off, plan.bg_len, plan.bg_phase, plan.bg_vol)] if mixed else []
            p = lambda t: None if t is None else t.data_ptr()
            lib.check(lib.tcr_compose(N, keep[0].data_ptr(), total, self.pool.data.data_ptr(), *(t.data_ptr() for t in keep[1:]),
                                      self.background.data.data_ptr() if mixed else None, *([t.data_ptr() for t in bgt] or [None] * 4),
                                      p(out), p(out_pcm), stream_of(dev)), "tcr_compose")
        return ComposedRecordings(out, out_pcm, plan, self.label_names)
