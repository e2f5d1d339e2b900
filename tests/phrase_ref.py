"""The phrase score of include/tcresnet_hip.h (tcr_phrase_scores) in NumPy, float32 operation by operation, in both forms the header
gives: the maximum over all chains t_1 <= .. <= t_n of the window (brute force; it also reports the first chain that reaches it) and
the DP.  tests/test_phrases.py checks the two against each other and the library against the DP."""
import itertools

import numpy as np

F = np.float32
PRODUCT, MIN = 0, 1


def combine_f(combine, a, b):
    """f(a, b): the float32 product or the minimum."""
    a, b = F(a), F(b)
    return F(a * b) if combine == PRODUCT else F(min(a, b))


def fold(combine, xs):
    r = F(xs[0])
    for x in xs[1:]:
        r = combine_f(combine, r, x)
    return r


def conf_brute(v, words, w, ordered, combine, i):
    """conf of one phrase at step i of the signal v [steps, C] by the definition -> (conf, the first best chain (t_1 .. t_n) in
    lexicographic order; unordered: the first maximum of every word)."""
    h = max(0, i - w + 1)
    if not ordered:
        chain = [h + int(np.argmax(v[h:i + 1, c])) for c in words]
        return fold(combine, [v[t, c] for t, c in zip(chain, words)]), tuple(chain)
    best, best_chain = None, None
    for chain in itertools.combinations_with_replacement(range(h, i + 1), len(words)):
        r = fold(combine, [v[t, c] for t, c in zip(chain, words)])
        if best is None or r > best:
            best, best_chain = r, chain
    return best, best_chain


def conf_dp(v, words, w, ordered, combine, i):
    """The same number by the DP (ordered) or the running maxima (unordered), started afresh for step i."""
    h, n = max(0, i - w + 1), len(words)
    E = [None] * n
    for t in range(h, i + 1):
        for m in range(n):                              # m ascending inside each t
            x = F(v[t, words[m]])
            if ordered and m > 0:
                x = combine_f(combine, E[m - 1], x)     # E[m - 1] is E_{m-1}(t): written above, in this t
            E[m] = x if E[m] is None else F(max(E[m], x))
    return E[n - 1] if ordered else fold(combine, E)


def scores_signal(v, phrases, w, ordered, combine, conf=conf_dp):
    """One signal: v [steps, C] float32 -> [steps, P + 1] float32, the background last."""
    steps, P = v.shape[0], len(phrases)
    out = np.zeros((steps, P + 1), F)
    for i in range(steps):
        for q, words in enumerate(phrases):
            c = conf(v, words, w, ordered, combine, i)
            out[i, q] = c[0] if isinstance(c, tuple) else c
        out[i, P] = F(F(1.0) - out[i, :P].max())
    return out


def scores_dp_fast(v, phrases, w, ordered, combine):
    """`scores_signal` with the DP vectorised over the steps i (row t of every window at once): the same float32 operations in the
    same order per step, at NumPy speed for the larger cases."""
    steps, P = v.shape[0], len(phrases)
    out = np.zeros((steps, P + 1), F)
    i = np.arange(steps)
    count = np.minimum(i + 1, w)
    for q, words in enumerate(phrases):
        n = len(words)
        E = np.full((n, steps), -np.inf, F)
        for k in range(min(w, steps)):                  # the k-th row of each step's window, oldest first
            live = k < count
            t = (i - count + 1 + k)[live]
            for m in range(n):
                x = v[t, words[m]].astype(F)
                if ordered and m > 0:
                    x = (E[m - 1, live] * x).astype(F) if combine == PRODUCT else np.minimum(E[m - 1, live], x)
                E[m, live] = np.maximum(E[m, live], x)
        if ordered:
            out[:, q] = E[n - 1]
        else:
            r = E[0].copy()
            for m in range(1, n):
                r = (r * E[m]).astype(F) if combine == PRODUCT else np.minimum(r, E[m])
            out[:, q] = r
    out[:, P] = F(1.0) - out[:, :P].max(axis=1)
    return out


def scores(values, offsets, phrases, w, ordered, combine, fast=True):
    """Packed values [total, C] with offsets [N + 1] -> [total, P + 1]: every signal on its own rows."""
    values = np.ascontiguousarray(values, F)
    out = np.zeros((values.shape[0], len(phrases) + 1), F)
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            out[a:b] = (scores_dp_fast if fast else scores_signal)(values[a:b], phrases, w, bool(ordered), combine)
    return out


def detect_rule(post, supp, thr):
    """np_detect's rule (tests/test_detect_grid.py) at W = 1, min_count = 1 on posteriors [steps, K] of one signal ->
    top, score, is_new."""
    steps = post.shape[0]
    sm = post * F(1.0)                                  # the mean of one vector: x * (1 / 1)
    top = np.argmax(sm, axis=1).astype(np.int32)
    score = sm[np.arange(steps), top].astype(F)
    new = np.zeros(steps, np.int32)
    prev, pstep = -1, 0
    for s in range(steps):
        if score[s] > F(thr) and top[s] != prev and (prev == -1 or s - pstep > supp):
            prev, pstep, new[s] = int(top[s]), s, 1
    return top, score, new
