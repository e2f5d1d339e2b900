"""The template-matching score of include/tcresnet_hip.h (tcr_dtw_scores) in NumPy, float32 operation by operation, as a
straightforward loop over the steps (a column of the DP is one array: the rule has no dependency inside a column), and the minimum
over every admissible path by brute force.  tests/test_templates.py checks the two against each other and the library against the
loop."""
import itertools

import numpy as np

F = np.float32
INF = F(np.inf)
N_MAX = np.int32(2 ** 31 - 2)


def distances(T, row):
    """d(j, t) for every frame j of the template T [L, F] against one row [F]: |.| summed with f ascending."""
    d = np.abs(T[:, 0] - row[0]).astype(F)
    for f in range(1, T.shape[1]):
        d = (d + np.abs(T[:, f] - row[f]).astype(F)).astype(F)
    return d


def initial(L):
    return np.full(L, INF, F), np.zeros(L, np.int32)


def step(T, row, D, n):
    """One step: the previous column (D, n) -> the new one."""
    L = T.shape[0]
    diag_D, diag_n = np.concatenate([[F(0)], D[:-1]]).astype(F), np.concatenate([[0], n[:-1]]).astype(np.int32)
    skip_D, skip_n = np.concatenate([[INF, F(0)], D[:-2]])[:L].astype(F), np.concatenate([[0, 0], n[:-2]])[:L].astype(np.int32)
    best_D, best_n = diag_D.copy(), diag_n.copy()
    for cand_D, cand_n in ((D, n), (skip_D, skip_n)):       # stay, then skip: strict comparisons keep the earlier candidate
        m = cand_D < best_D
        best_D[m], best_n[m] = cand_D[m], cand_n[m]
    return (distances(T, row) + best_D).astype(F), (np.minimum(best_n, N_MAX) + 1).astype(np.int32)


def walk(T, v, state=None):
    """One template over one signal's rows v [steps, F] -> cost [steps] float32, len [steps] int32 and the column after the last row."""
    T, v = np.ascontiguousarray(T, F), np.ascontiguousarray(v, F)
    D, n = initial(T.shape[0]) if state is None else state
    cost, length = np.zeros(v.shape[0], F), np.zeros(v.shape[0], np.int32)
    for t in range(v.shape[0]):
        D, n = step(T, v[t], D, n)
        cost[t], length[t] = D[-1], n[-1]
    return cost, length, (D, n)


def conf_of(cost, length, scale, max_steps):
    with np.errstate(invalid="ignore"):
        c = np.maximum(F(1.0) - (cost * F(scale)).astype(F), F(0)).astype(F)
    if max_steps > 0:
        c[length > max_steps] = F(0)
    return c


def scores_signal(v, templates, keyword_offsets, scale, max_steps=0):
    """One signal: v [steps, F] -> (out [steps, K + 1] float32, lengths [steps, K] int32)."""
    steps, K = v.shape[0], len(keyword_offsets) - 1
    out, lengths = np.zeros((steps, K + 1), F), np.zeros((steps, K), np.int32)
    for k in range(K):
        for q in range(keyword_offsets[k], keyword_offsets[k + 1]):     # ascending, strict >: the first maximum wins
            cost, length, _ = walk(templates[q], v)
            c = conf_of(cost, length, scale[q], max_steps)
            better = np.ones(steps, bool) if q == keyword_offsets[k] else c > out[:, k]
            out[better, k], lengths[better, k] = c[better], length[better]
    out[:, K] = F(1.0) - out[:, :K].max(axis=1)
    return out, lengths


def scores(values, offsets, templates, keyword_offsets, scale, max_steps=0):
    """Packed values [total, F] with offsets [N + 1] -> (out [total, K + 1], lengths [total, K]): every signal on its own rows."""
    values = np.ascontiguousarray(values, F)
    K = len(keyword_offsets) - 1
    out, lengths = np.zeros((values.shape[0], K + 1), F), np.zeros((values.shape[0], K), np.int32)
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            out[a:b], lengths[a:b] = scores_signal(values[a:b], templates, keyword_offsets, scale, max_steps)
    return out, lengths


def cost_brute(T, v, t):
    """min over every admissible path that ends in frame L - 1 at step t of the left-to-right float32 sum of its distances: a path
    starts at any step in frame 0 or 1 (the free start, on the diagonal or by a skip) and moves 0, 1 or 2 frames a step."""
    L = T.shape[0]
    d = np.stack([distances(np.ascontiguousarray(T, F), np.ascontiguousarray(v[s], F)) for s in range(t + 1)])       # [step][frame]
    best = INF
    for m in range(1, t + 2):                               # the steps on the path: t - m + 1 .. t
        for j_first in (0, 1):
            if j_first >= L:
                continue
            for moves in itertools.product((0, 1, 2), repeat=m - 1):
                if j_first + sum(moves) != L - 1:
                    continue
                j, acc = j_first, F(d[t - m + 1, j_first] + F(0))
                for i, mv in enumerate(moves):
                    j += mv
                    acc = F(d[t - m + 2 + i, j] + acc)
                if acc < best:
                    best = acc
    return best
