"""The switch-cost path decoder's definition (include/tennis_hip.h, docs/kernels.md "Event decoding with a switch cost") taken apart in
float64 numpy, for the tests of ``events.viterbi_labels`` and of the kernels: the emissions, the score of a path, the optimum by brute
force and by a textbook max-plus recursion without the normalisation, the forward values with their ties, and the bound on what fp32
rounding can cost a path.  Nothing of the kernels' tiling is in it."""
import itertools

import numpy as np

U = 2.0 ** -24


def begins_of(start):
    b = np.asarray(start).reshape(-1) != 0
    b = b.copy()
    if len(b):
        b[0] = True
    return b


def videos(start):
    """-> list of (first, end) of every video, end exclusive"""
    b = np.flatnonzero(begins_of(start)).tolist()
    return list(zip(b, b[1:] + [len(np.asarray(start).reshape(-1))]))


def emissions(logits, rows):
    """e[m, c] = q[c] - max q, q = logits[clip(rows[m])], float64 (exact for fp32 logits)"""
    logits = np.asarray(logits, np.float64)
    q = logits[np.clip(np.asarray(rows, np.int64), 0, len(logits) - 1)]
    return q - q.max(1, keepdims=True)


def path_score(e, label, start, cost):
    """sum of e[m, label[m]] minus cost for every change of label inside a video"""
    label = np.asarray(label, np.int64)
    m = len(label)
    change = (label[1:] != label[:-1]) & ~begins_of(start)[1:] if m > 1 else np.zeros(0, bool)
    return float(e[np.arange(m), label].sum() - float(cost) * change.sum())


def brute_force(e, start, cost):
    """the best score over all C^M paths (tiny cases only)"""
    m, c = e.shape
    assert c ** m <= 4 ** 7
    paths = np.asarray(list(itertools.product(range(c), repeat=m)), np.int64)            # (C^M, M)
    change = (paths[:, 1:] != paths[:, :-1]) & ~begins_of(start)[None, 1:]
    return float((e[np.arange(m)[None, :], paths].sum(1) - float(cost) * change.sum(1)).max())


def optimum(e, start, cost):
    """the best score by the textbook recursion: w_t[c] = e_t[c] + max(w_{t-1}[c], max_k w_{t-1}[k] - cost), no normalisation"""
    total = 0.0
    for a, b in videos(start):
        w = e[a].copy()
        for t in range(a + 1, b):
            w = e[t] + np.maximum(w, w.max() - cost)
        total += float(w.max())
    return total


def forward_values(e, start, cost):
    """v (M, C) of the definition's forward recurrence in float64, and per position whether the arg-max of v is tied (``amax_tie``)
    and whether some class enters the position with v_{t-1}[c] == -cost exactly (``stay_tie``; False at a video's first position)"""
    m, c = e.shape
    v = np.zeros((m, c))
    amax_tie, stay_tie = np.zeros(m, bool), np.zeros(m, bool)
    for a, b in videos(start):
        v[a] = e[a]
        for t in range(a + 1, b):
            stay_tie[t] = bool(np.any(v[t - 1] == -cost))
            u = e[t] + np.maximum(v[t - 1], -cost)
            v[t] = u - u.max()
    amax_tie[:] = (v == 0).sum(1) > 1                  # (the maximum of every v is 0)
    return v, amax_tie, stay_tie


def path_bound(m, cost, emax):
    """What fp32 rounding can cost the returned path against the optimum, in float64 score: 2 * m * 3 u (cost + emax), u = 2^-24.
    Every fp32 step rounds one emission (q - max q), one addition (e + max(v, -cost)) and one normalisation (u - max u), each result
    of magnitude at most cost + emax, so each off by at most u (cost + emax); max(), the comparisons and the common shift by max u
    change no decision.  The fp32 run is therefore an exact run on emissions moved by at most 3 u (cost + emax) each, for which its
    path is optimal; the score of ANY path of m positions moves by at most m times that, and two paths are compared."""
    return 2.0 * m * 3.0 * U * (float(cost) + float(emax))
