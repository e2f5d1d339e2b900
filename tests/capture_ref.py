"""The capture definition of include/tcresnet_hip.h in NumPy, over a stream's whole recording and whole row arrays, and the emission
schedule: which clips each call emits and in which order.  Test infrastructure; nothing here looks at the code under test."""
from typing import List, NamedTuple, Optional, Sequence

import numpy as np


class Clip(NamedTuple):
    stream: int
    step: int           # the trigger's row, counted from the stream's start or last reset
    label: int
    score: np.float32
    clip: np.ndarray    # float32 [n_samples]
    first: int          # the clip's first sample in the recording (may be negative)


def delay(lead: int, step_samples: int) -> int:
    """D = max(0, ceil(lead / step_samples)): the rows between a trigger and the row whose call emits its clip."""
    return max(0, -(-int(lead) // int(step_samples)))


def clip_of(recording: np.ndarray, i: int, step_samples: int, n_samples: int, lead: int) -> np.ndarray:
    """recording[(i + 1) * step + lead - n : (i + 1) * step + lead], zeros outside the recording."""
    end = (i + 1) * step_samples + lead
    first = end - n_samples
    out = np.zeros(n_samples, np.float32)
    lo, hi = max(first, 0), min(end, len(recording))
    if hi > lo:
        out[lo - first:hi - first] = recording[lo:hi]
    return out


class _Stream:
    def __init__(self):
        self.rec = np.zeros(0, np.float32)
        self.top, self.score, self.flag, self.done = np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, bool), np.zeros(0, bool)


class Reference:
    """S streams.  `push` takes, per stream, the call's samples [rows_s * step] and rows (top, score, is_new [rows_s]) and returns the
    clips the call emits in (stream, row) order; a stream without rows is not touched and its reset flag is ignored (the caller
    passes it again).  `flush` returns the pending clips of the masked streams, audio not yet heard as zeros, and forgets them."""

    def __init__(self, n_streams: int, step_samples: int, n_samples: int, lead: int, classes: Optional[Sequence[int]] = None):
        self.S, self.step, self.n, self.lead, self.D = n_streams, step_samples, n_samples, lead, delay(lead, step_samples)
        self.classes = None if classes is None else set(int(c) for c in classes)
        self.streams = [_Stream() for _ in range(n_streams)]
        self.carried = 0            # clips emitted by a later call than their trigger's

    def _emit(self, s: int, i: int, heard_all: bool) -> Clip:
        st = self.streams[s]
        end = (i + 1) * self.step + self.lead
        if heard_all:               # a push emits a clip only once all its samples have been heard
            assert end <= len(st.rec), (s, i, end, len(st.rec))
        st.done[i] = True
        return Clip(s, i, int(st.top[i]), st.score[i], clip_of(st.rec, i, self.step, self.n, self.lead), end - self.n)

    def push(self, samples, top, score, is_new, reset=None) -> List[Clip]:
        out = []
        for s, st in enumerate(self.streams):
            rows = len(top[s])
            assert len(samples[s]) == rows * self.step
            if rows == 0:
                continue
            if reset is not None and reset[s]:
                self.streams[s] = st = _Stream()
            r0 = len(st.top)
            t = np.asarray(top[s], np.int32)
            flag = np.asarray(is_new[s]) != 0
            if self.classes is not None:
                flag &= np.array([int(c) in self.classes for c in t], bool)
            st.rec = np.concatenate([st.rec, np.asarray(samples[s], np.float32)])
            st.top, st.score = np.concatenate([st.top, t]), np.concatenate([st.score, np.asarray(score[s], np.float32)])
            st.flag, st.done = np.concatenate([st.flag, flag]), np.concatenate([st.done, np.zeros(rows, bool)])
            for r in range(r0, r0 + rows):
                i = r - self.D
                if i >= 0 and st.flag[i] and not st.done[i]:
                    self.carried += i < r0
                    out.append(self._emit(s, i, True))
        return out

    def flush(self, mask=None) -> List[Clip]:
        out = []
        for s, st in enumerate(self.streams):
            if mask is not None and not mask[s]:
                continue
            rows = len(st.top)
            for i in range(max(0, rows - self.D), rows):
                if st.flag[i] and not st.done[i]:
                    out.append(self._emit(s, i, False))
        return out
