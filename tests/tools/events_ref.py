"""The event decoder's definitions (include/tennis_hip.h, docs/kernels.md "Event decoding") restated in float64 numpy: softmax, the
window mean cut at video boundaries, the first arg-max, the runs, and an event's mean and peak.  Written from the definitions, with
nothing of the kernels' tiling in it: every position is treated alike."""
import numpy as np


def decode_ref(logits, rows, start, width):
    """-> dict: ``p`` (M, C) and ``score`` (M, C) float64, ``label`` (M,), ``conf`` (M,), ``margin`` (M,) the best score minus the
    second best (inf for one class), and the events ``first``, ``last``, ``cls`` (int64), ``ev_score``, ``ev_peak`` (float64)."""
    logits = np.asarray(logits, np.float64)
    n, c = logits.shape
    rows = np.clip(np.asarray(rows, np.int64), 0, n - 1)
    begins = np.asarray(start).reshape(-1) != 0
    m = len(rows)
    assert len(begins) == m and m >= 1 and width % 2 == 1 and 1 <= width <= 63
    begins = begins.copy()
    begins[0] = True
    x = logits[rows]
    e = np.exp(x - x.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    vid = np.cumsum(begins) - 1                       # the video of every position
    vfirst = np.flatnonzero(begins)[vid]              # first position of its video
    vlast = np.append(np.flatnonzero(begins)[1:], m)[vid] - 1
    h = (width - 1) // 2
    pos = np.arange(m)
    lo, hi = np.maximum(pos - h, vfirst), np.minimum(pos + h, vlast)
    cs = np.concatenate([np.zeros((1, c)), np.cumsum(p, 0)])
    score = p.copy() if width == 1 else (cs[hi + 1] - cs[lo]) / (hi - lo + 1)[:, None]
    if width > 1 and m * c * width <= 1 << 24:       # small enough: the direct sum instead of differences of running sums
        score = np.stack([p[lo[i]:hi[i] + 1].sum(0) / (hi[i] - lo[i] + 1) for i in range(m)])
    label = score.argmax(1)                           # (numpy's argmax is the first maximum)
    conf = score[pos, label]
    if c > 1:
        top = np.sort(score, 1)
        margin = top[:, -1] - top[:, -2]
    else:
        margin = np.full(m, np.inf)
    run = begins.copy()
    run[1:] |= label[1:] != label[:-1]
    first = np.flatnonzero(run)
    last = np.append(first[1:], m) - 1
    ev_score = np.asarray([conf[a:b + 1].mean() for a, b in zip(first, last)])
    ev_peak = np.asarray([conf[a:b + 1].max() for a, b in zip(first, last)])
    return dict(p=p, score=score, label=label, conf=conf, margin=margin, first=first, last=last, cls=label[first], ev_score=ev_score,
                ev_peak=ev_peak, lo=lo, hi=hi)


U = 2.0 ** -24


def score_bound(c, width):
    """Absolute bound on an fp32 score against float64, every score being at most 1: the softmax costs the subtraction (1), expf (2
    ulp assumed), the C-term sum of the denominator (C - 1) and the division (1), each relative to a value <= 1; the window adds
    width - 1 additions and one division; two spare.  (C + width + 8) u, u = 2^-24."""
    return (c + width + 8) * U


def mean_bound(length):
    """An event's mean over ``length`` confs <= 1 on top of the confs' own error: ceil(length / 64) - 1 additions in a lane, six levels
    of the tree, one division, one spare: (ceil(length / 64) + 7) u."""
    return (-(-length // 64) + 7) * U
