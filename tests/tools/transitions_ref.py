"""The transition-matrix path decoder's definition (include/tennis_hip.h, docs/kernels.md "Event decoding with a transition matrix")
taken apart in float64 numpy, for the tests of ``events.viterbi_labels(transitions=...)`` and of the kernels: the score of a path
under a matrix, the optimum by brute force and by the textbook max-plus recursion without the normalisation, the forward values
with their ties, and the bound on what fp32 rounding can cost a path.  Nothing of the kernels' tiling is in it.  The emissions and
the video bounds are viterbi_ref's."""
import itertools

import numpy as np

from .viterbi_ref import U, begins_of, emissions, videos  # noqa: F401  (re-exported for the tests)


def potts(c, cost):
    """-cost (1 - I): the matrix under which the decoder is the switch-cost decoder"""
    return (-float(cost) * (1.0 - np.eye(c))).astype(np.float32)


def cyclic(c):
    """c -> c and c -> c + 1 mod C cost nothing, everything else is forbidden"""
    t = np.full((c, c), -np.inf, np.float32)
    for k in range(c):
        t[k, k] = 0.0
        t[k, (k + 1) % c] = 0.0
    return t


def path_score(e, label, start, trans):
    """sum of e[m, label[m]] plus trans[label[m-1], label[m]] at every position that is not its video's first (-inf for a path
    that takes a forbidden transition)"""
    label = np.asarray(label, np.int64)
    trans = np.asarray(trans, np.float64)
    m = len(label)
    total = float(e[np.arange(m), label].sum())
    if m > 1:
        inside = ~begins_of(start)[1:]
        total += float(trans[label[:-1][inside], label[1:][inside]].sum())
    return total


def brute_force(e, start, trans):
    """the best score over all C^M paths (tiny cases only)"""
    m, c = e.shape
    assert c ** m <= 4 ** 7
    trans = np.asarray(trans, np.float64)
    paths = np.asarray(list(itertools.product(range(c), repeat=m)), np.int64)            # (C^M, M)
    score = e[np.arange(m)[None, :], paths].sum(1)
    if m > 1:
        step = trans[paths[:, :-1], paths[:, 1:]]
        score = score + np.where(begins_of(start)[None, 1:], 0.0, step).sum(1)
    return float(score.max())


def optimum(e, start, trans):
    """the best score by the textbook recursion: w_t[c] = e_t[c] + max_p (w_{t-1}[p] + T[p, c]), no normalisation"""
    trans = np.asarray(trans, np.float64)
    total = 0.0
    for a, b in videos(start):
        w = e[a].copy()
        for t in range(a + 1, b):
            w = e[t] + (w[:, None] + trans).max(0)
        total += float(w.max())
    return total


def forward_values(e, start, trans):
    """v (M, C) of the definition's forward recurrence in float64, and per position whether the arg-max of v is tied (``amax_tie``),
    whether for some class staying ties with another predecessor (``stay_tie``), and whether for some class two predecessors other
    than the class itself tie for the maximum while staying does not attain it (``pred_tie``: the smallest wins).  The last two are
    False at a video's first position."""
    trans = np.asarray(trans, np.float64)
    m, c = e.shape
    v = np.zeros((m, c))
    amax_tie, stay_tie, pred_tie = np.zeros(m, bool), np.zeros(m, bool), np.zeros(m, bool)
    for a, b in videos(start):
        v[a] = e[a]
        for t in range(a + 1, b):
            cand = v[t - 1][:, None] + trans
            w = cand.max(0)
            hits = cand == w[None, :]
            stays = np.diagonal(hits)
            stay_tie[t] = bool(np.any(stays & (hits.sum(0) > 1)))
            pred_tie[t] = bool(np.any(~stays & (hits.sum(0) > 1)))
            u = e[t] + w
            v[t] = u - u.max()
    amax_tie[:] = (v == 0).sum(1) > 1                  # (the maximum of every v is 0)
    return v, amax_tie, stay_tie, pred_tie


def forbidden_pairs(label, start, trans):
    """how many adjacent positions of one video take a transition whose score is -inf"""
    label = np.asarray(label, np.int64)
    if len(label) < 2:
        return 0
    inside = ~begins_of(start)[1:]
    return int(np.isneginf(np.asarray(trans)[label[:-1][inside], label[1:][inside]]).sum())


def path_bound(m, tmax, emax):
    """What fp32 rounding can cost the returned path against the optimum, in float64 score, for a matrix whose entries are all
    finite: 2 * m * 4 u (emax + tmax) (1 + 2^-20), u = 2^-24, tmax = max |T|, emax = max |e|.

    Magnitudes.  The best predecessor has v = 0, so w[c] >= -tmax; with e >= -emax, u[c] >= -(emax + tmax), and max_c u <= 0 is
    subtracted, so v[c] = u[c] - max u lies in [-(emax + tmax), 0] too.  A candidate v[p] + T[p, c] therefore lies in
    [-(emax + 2 tmax), 0].

    Roundings.  A step of the fp32 run rounds, for a position labelled c that follows one labelled p, four results that the score of
    a path through (p, c) depends on: the emission q - max q (off by at most u emax), the candidate v[p] + T[p, c] (u (emax + 2
    tmax)), the sum e + w (u (emax + tmax)) and the normalisation u - max u (u (emax + tmax)); the maxima, the comparisons and the
    shift by max u, which is common to every class, change no decision.  Their sum is at most 4 u (emax + tmax).  Read the other
    way, the fp32 run is an EXACT run on emissions and (position-dependent) transition scores moved by at most that much per
    position, and its back-pointers are true arg-maxima of that run, so its path is optimal for the moved inputs.  The score of ANY
    path of m positions moves by at most m times that, and two paths are compared: the returned one and the optimum.  The factor
    1 + 2^-20 covers the second-order terms (the magnitudes above are those of the rounded values, off by a few u themselves)."""
    return 2.0 * m * 4.0 * U * (float(emax) + float(tmax)) * (1.0 + 2.0 ** -20)
