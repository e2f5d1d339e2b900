"""The detector rule of include/tcresnet_hip.h (tcr_stream_step) in NumPy, float32 operation by operation, written from that
documentation: smoothing over the last count = min(steps since the reset, W) probability vectors (float32 adds, oldest to newest,
times float32(1) / float32(count)), the argmax with the lowest index on ties, the min_count gate, the strict threshold and the
suppression rule.  One call takes any number of steps of one stream, from a fresh detector or from the state an earlier call
returned, and reports which named edges its input exercised, so that a test can assert that its inputs reach them.
tests/test_detector_rule.py checks it against the two older restatements and the library against it."""
import numpy as np

F = np.float32
PASS, PROBE = 8192, 256         # the suppression walk's geometry (scan.hip: 256 x kSuppressPer steps a pass, 256 steps a probe)
BRANCHES = {"warming up", "below threshold", "same label", "suppressed", "first", "new label"}


class State:
    """A stream between calls: the last min(n, W) vectors (oldest first), the call each of them came from, prev_label, prev_step and
    the step counter n (steps since the reset; prev_step counts in the same units)."""

    def __init__(self, ncls):
        self.ring = np.zeros((0, ncls), F)
        self.ring_call = np.zeros(0, np.int64)
        self.prev_label, self.prev_step, self.n, self.calls = -1, 0, 0, 0

    def integers(self, W):
        """The five integers the device keeps: head, count, prev_label, prev_step, n."""
        return [self.n % W, min(self.n, W), self.prev_label, self.prev_step, self.n]


def smooth(ext, h, W, newest_first=False):
    """ext [h + steps, C]: the h = count0 vectors before the call, then the call's -> smoothed [steps, C], count [steps]."""
    steps = ext.shape[0] - h
    i = np.arange(steps)
    count = np.minimum(h + i + 1, W)
    acc = np.zeros((steps, ext.shape[1]), F)
    for q in range(int(count.max()) if steps else 0):
        m = q < count
        src = (h + i - q) if newest_first else (h + i - count + 1 + q)
        acc[m] = acc[m] + ext[src[m]]
    return acc * (F(1) / count.astype(F))[:, None], count


def detect(probs, W, min_count, suppression, threshold, state=None, reset=False):
    """probs [steps, C] float32 of one stream -> (smoothed, top, score, is_new, the state afterwards, the set of edges taken).
    state None or reset: a fresh detector.  The state passed in is left as it was."""
    probs = np.ascontiguousarray(probs, F)
    steps, ncls = probs.shape
    old = State(ncls) if state is None or reset else state
    st = State(ncls)
    st.calls = (0 if state is None else state.calls) + 1
    h = old.ring.shape[0]
    ext = np.concatenate([old.ring, probs])
    ext_call = np.concatenate([old.ring_call, np.full(steps, st.calls, np.int64)])
    sm, count = smooth(ext, h, W)
    edges = set()
    best = np.argmax(sm, axis=1).astype(np.int32)       # (the first maximum: the lowest index on ties)
    i = np.arange(steps)
    best_v = sm[i, best]
    warm = count >= min_count
    top = np.where(warm, best, -1).astype(np.int32)
    score = np.where(warm, best_v, F(0)).astype(F)
    cand = warm & (score > F(threshold))
    new = np.zeros(steps, np.int32)
    if (~warm).any():
        edges.add("warming up")
    if (warm & ~cand).any():
        edges.add("below threshold")
    if (warm & ((sm == best_v[:, None]).sum(axis=1) > 1)).any():
        edges.add("tie")
    if (warm & (score == F(threshold))).any():
        edges.add("score equals threshold")
    if W >= 2 and old.n % W + steps >= W:
        edges.add("head wraps")
    if steps and h and W >= 2:
        oldest = ext_call[np.maximum(h + i - count + 1, 0)]
        newest_old = ext_call[h - 1]
        if ((h + i - count + 1 < h) & (oldest != newest_old)).any():
            edges.add("window reads two earlier calls")
    prev, pstep, n0 = old.prev_label, old.prev_step, old.n
    run = 0                                             # candidates in a row that did not fire for their label
    for s in np.nonzero(cand)[0]:
        s = int(s)
        if top[s] == prev:
            edges.add("same label")
            run += 1
            if pstep < n0:
                edges.add("same label as an earlier call's detection")
            continue
        if prev != -1 and n0 + s - pstep <= suppression:
            edges.add("suppressed")
            if pstep < n0:
                edges.add("suppressed by an earlier call's detection")
            elif s // PASS != (pstep - n0) // PASS:
                edges.add("suppressed across a pass")
            if n0 + s - pstep >= PROBE:
                edges.add("suppressed across a probe")
            if n0 + s - pstep == suppression:
                edges.add("suppressed at the interval's last step")
            continue
        edges.add("first" if prev == -1 else "new label")
        if prev != -1 and n0 + s - pstep == suppression + 1:
            edges.add("fires at the first step behind the interval")
        if run >= PROBE:
            edges.add("fires behind a probe of its own label")
        if prev != -1 and pstep >= n0 and s // PASS != (pstep - n0) // PASS:
            edges.add("fires in a later pass")
        if prev != -1 and pstep >= n0 and s // PASS > (pstep - n0) // PASS + 1:
            edges.add("fires behind a pass without candidates")
        if prev == -1 and s >= PASS and not cand[:s // PASS * PASS].any():
            edges.add("first behind passes without candidates")
        if s % PASS == 0 and s:
            edges.add("fires at a pass's first step")
        if s % PASS == PASS - 1:
            edges.add("fires at a pass's last step")
        if s % PROBE == PROBE - 1:
            edges.add("fires at a probe's last step")
        if s == steps - 1:
            edges.add("fires at the last step")
        if top[s] == ncls - 1:
            edges.add("last label fires")
        if top[s] == 255:
            edges.add("label 255 fires")
        prev, pstep, new[s], run = int(top[s]), n0 + s, 1, 0
    keep = min(W, h + steps)
    st.ring, st.ring_call = ext[h + steps - keep:].copy(), ext_call[h + steps - keep:].copy()
    st.prev_label, st.prev_step, st.n = prev, pstep, n0 + steps
    return sm, top, score, new, st, edges


def order_matters(probs, W, state=None):
    """Does summing newest to oldest change the bits of `smoothed` in some row?"""
    probs = np.ascontiguousarray(probs, F)
    ring = state.ring if state is not None else np.zeros((0, probs.shape[1]), F)
    ext = np.concatenate([ring, probs])
    a, b = smooth(ext, ring.shape[0], W)[0], smooth(ext, ring.shape[0], W, newest_first=True)[0]
    return not np.array_equal(a.view(np.uint32), b.view(np.uint32))
