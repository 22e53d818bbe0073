"""From per-sample logits to events: the host side of ``evaluate --save_events`` (the decoding itself is ``engine.EventDecoder``).

A split's samples are not stored in time order (balancing thins them, splits interleave videos), so ``time_order`` sorts them once
per split on the host into the position list the decoder walks; ``label_runs`` applies the decoder's run rule to integer labels, which
is where the ground-truth events come from (not from ``TennisSet._events``, which opens every video with an empty ``OTH`` run and is
built before balancing); ``save_events`` / ``load_events`` keep one ``.npz`` of flat arrays.
"""
from __future__ import annotations

import os

import numpy as np

EVENT_COLUMNS = ("video", "first_frame", "last_frame", "cls", "score", "peak", "first_sample", "last_sample",
                 "gt_video", "gt_first_frame", "gt_last_frame", "gt_cls", "smooth", "tiou", "precision", "recall", "f1")
MAX_SMOOTH = 63


def check_save_events(flags, world=1):
    """``--save_events`` is for a test run that yields per-sample logits, on one rank: exits with the reason otherwise.  Touches no
    device."""
    smooth = getattr(flags, "event_smooth", None)
    cost = getattr(flags, "event_switch_cost", None)
    trans = getattr(flags, "event_transitions", None)
    prior = getattr(flags, "event_transition_prior", None)
    scale = getattr(flags, "event_transition_scale", None)
    post = getattr(flags, "event_posteriors", False)
    if trans is None:
        for name, value in (("prior", prior), ("scale", scale)):
            if value is not None:
                raise SystemExit("--event_transition_%s %s sets how --event_transitions train turns counts into scores: give "
                                 "--event_transitions too" % (name, value))
    if not getattr(flags, "save_events", False):
        if smooth is not None:
            raise SystemExit("--event_smooth %s sets the smoothing window of --save_events: give --save_events too" % smooth)
        if cost is not None:
            raise SystemExit("--event_switch_cost %s sets the label-switch penalty of --save_events: give --save_events too" % cost)
        if trans is not None:
            raise SystemExit("--event_transitions %s sets the class-transition scores of --save_events: give --save_events too" % trans)
        if post:
            raise SystemExit("--event_posteriors sets how the events of --save_events are scored: give --save_events too")
        return
    if post and trans is None and cost is None:
        raise SystemExit("--event_posteriors scores events with the posteriors of the path's model: give --event_transitions or "
                         "--event_switch_cost too")
    if trans is not None:
        if cost is not None:
            raise SystemExit("--event_transitions is a matrix of switch costs: not together with --event_switch_cost %s" % cost)
        if smooth is not None and smooth > 1:
            raise SystemExit("--event_transitions decodes the unsmoothed scores as one path: not together with --event_smooth %d" % smooth)
        if trans != "train" and (prior is not None or scale is not None):
            raise SystemExit("--event_transition_prior and --event_transition_scale shape the matrix that --event_transitions train "
                             "counts: %s is used as it is" % trans)
        for name, value in (("prior", prior), ("scale", scale)):
            if value is not None and not (np.isfinite(value) and value > 0):
                raise SystemExit("--event_transition_%s %s: it must be finite and > 0, so that every score is finite" % (name, value))
    if cost is not None:
        if not (np.isfinite(cost) and cost >= 0):
            raise SystemExit("--event_switch_cost %s: the penalty for every change of label is subtracted from a path's summed scores, "
                             "so it must be finite and >= 0" % cost)
        if smooth is not None and smooth > 1:
            raise SystemExit("--event_switch_cost decodes the unsmoothed scores as one path: not together with --event_smooth %d" % smooth)
    if smooth is not None and (smooth < 1 or smooth > MAX_SMOOTH or smooth % 2 == 0):
        raise SystemExit("--event_smooth %d: the smoothing window is centred on a frame, so it must be odd, and it is summed directly, "
                         "so it must lie in [1, %d]" % (smooth, MAX_SMOOTH))
    if flags.save_feats:
        raise SystemExit("--save_events decodes the logits of a test run: not together with --save_feats")
    if flags.corpus_frames > 0:
        raise SystemExit("--save_events writes the events of a split's samples: --corpus_frames runs a synthetic corpus that has none")
    if flags.num_gpus > 1 or world > 1:
        raise SystemExit("--save_events decodes one time-ordered list on one rank: run it with --num_gpus 1")


def time_order(dataset, order=None):
    """-> ``(rows, start, video, frame)`` of the time-ordered position list: ``rows (M,)`` int32 the logit row of every position,
    ``start (M,)`` int32 1 where a video begins, ``video (M,)`` unicode and ``frame (M,)`` int64 of every position.  ``order``: the
    dataset index whose logits row r holds (None: row r is sample r).  Samples are sorted by (video, frame number) with a stable
    sort, on the host."""
    order = np.arange(len(dataset._samples)) if order is None else np.asarray(order, np.int64).reshape(-1)
    samples = [dataset._samples[int(i)] for i in order]
    video = np.asarray([s[0] for s in samples], dtype=np.str_)
    frame = np.asarray([int(s[1]) for s in samples], np.int64)
    rows = np.lexsort((frame, video)) if len(samples) else np.zeros(0, np.int64)      # (lexsort is stable; the last key is the primary)
    video, frame = video[rows], frame[rows]
    start = np.ones(len(rows), np.int32)
    if len(rows) > 1:
        start[1:] = video[1:] != video[:-1]
    return rows.astype(np.int32), start, video, frame


def label_runs(labels, start):
    """The decoder's run rule on integer labels: a run begins where ``start`` is non-zero (position 0 always) or the label differs from
    the one before.  -> ``(first, last, cls)`` int64 arrays, positions inclusive, ordered by ``first``."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    start = np.asarray(start).reshape(-1) != 0
    if len(labels) != len(start):
        raise ValueError(f"label_runs: {len(labels)} labels for {len(start)} start flags")
    if not len(labels):
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    begins = start.copy()
    begins[0] = True
    begins[1:] |= labels[1:] != labels[:-1]
    first = np.flatnonzero(begins)
    last = np.append(first[1:], len(labels)) - 1
    return first, last, labels[first]


def check_transitions(transitions, classes=None, who="transitions"):
    """-> the matrix as (C, C) float32, or ValueError naming the first entry ``[from, to]`` that is NaN or positive, or the first
    diagonal entry that is not finite (the contract of ``tn_event_decoder_run_transitions``)."""
    t = np.asarray(transitions, np.float32)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] < 1 or (classes is not None and t.shape[0] != classes):
        raise ValueError(f"{who}: the matrix must be (C, C)" + ("" if classes is None else f" = ({classes}, {classes})") + f", got {t.shape}")
    bad = np.isnan(t) | (t > 0) | (np.eye(len(t), dtype=bool) & ~np.isfinite(t))
    if bad.any():
        p, c = (int(i) for i in np.argwhere(bad)[0])
        why = "is NaN" if np.isnan(t[p, c]) else "is positive" if t[p, c] > 0 else "is not finite (staying must always be possible)"
        raise ValueError(f"{who}: transitions[{p}][{c}] {why}")
    return t


def transition_scores(labels, start, classes, prior=1.0, scale=1.0):
    """Transition scores from the label bigrams of a time-ordered list: ``N[p, c]`` counts the positions that are not a video's first
    (``start`` zero, position 0 never counts) with ``labels[m - 1] = p`` and ``labels[m] = c``;
    ``T = scale * ln((N + prior) / (N.sum(1, keepdims=True) + prior * classes))`` in float64 -> ``(classes, classes)`` float32, every
    entry finite and < 0, the rows of ``exp(T / scale)`` summing to 1.  ``prior`` > 0 (additive smoothing) and ``scale`` > 0."""
    classes = int(classes)
    if classes < 1:
        raise ValueError(f"transition_scores: classes must be >= 1, got {classes}")
    if not (np.isfinite(prior) and prior > 0):
        raise ValueError(f"transition_scores: prior must be finite and > 0, got {prior}")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"transition_scores: scale must be finite and > 0, got {scale}")
    labels = np.asarray(labels, np.int64).reshape(-1)
    begins = np.asarray(start).reshape(-1) != 0
    if len(labels) != len(begins):
        raise ValueError(f"transition_scores: {len(labels)} labels for {len(begins)} start flags")
    if len(labels) and (labels.min() < 0 or labels.max() >= classes):
        raise ValueError(f"transition_scores: labels must lie in [0, {classes}), got [{labels.min()}, {labels.max()}]")
    counts = np.zeros((classes, classes), np.float64)
    if len(labels) > 1:
        inside = ~begins[1:]
        np.add.at(counts, (labels[:-1][inside], labels[1:][inside]), 1.0)
    t = float(scale) * np.log((counts + float(prior)) / (counts.sum(1, keepdims=True) + float(prior) * classes))
    return t.astype(np.float32)


def viterbi_labels(logits, rows, start, switch_cost=None, dtype=np.float64, transitions=None):
    """The label path of ``EventDecoder.decode(..., switch_cost=...)`` on the host, in ``dtype`` arithmetic (docs/kernels.md "Event
    decoding with a switch cost"): per video the path that maximises the sum of ``e[m, label[m]]`` minus ``switch_cost`` for every
    change of label, ``e[m] = q - max(q)``, ``q = logits[clip(rows[m], 0, N - 1)]``.  Forward ``v_0 = e_0``, ``stay_t = v_{t-1} >=
    -switch_cost``, ``u_t = e_t + max(v_{t-1}, -switch_cost)``, ``v_t = u_t - max(u_t)``, ``a_t`` the first arg-max of ``v_t``; back
    ``label[T-1] = a_{T-1}``, ``label[t-1] = label[t] if stay_t[label[t]] else a_{t-1}``.  A Python loop over the positions.
    With ``transitions`` (C, C) in place of ``switch_cost`` (exactly one of the two): the path of ``decode(..., transitions=...)``
    (docs/kernels.md "Event decoding with a transition matrix"), which adds ``transitions[label[m-1], label[m]]`` at every position
    that is not its video's first: ``w_t[c] = max_p (v_{t-1}[p] + T[p, c])``, ``b_t[c] = c`` if ``v_{t-1}[c] + T[c, c]`` attains it,
    else the smallest ``p`` that does, ``u_t = e_t + w_t``, ``v_t`` and ``a_t`` as above; back ``label[t-1] = b_t[label[t]]``.
    -> ``label (M,)`` int64."""
    if (switch_cost is None) == (transitions is None):
        raise ValueError("viterbi_labels: give exactly one of switch_cost and transitions")
    dtype = np.dtype(dtype).type
    if transitions is None:
        cost = float(switch_cost)
        if not (np.isfinite(cost) and cost >= 0):
            raise ValueError(f"viterbi_labels: switch_cost must be finite and >= 0, got {switch_cost}")
    logits, rows, bounds = _viterbi_positions(logits, rows, start, "viterbi_labels")
    m, c = len(rows), logits.shape[1]
    # step: v_{t-1} -> (w_t, what the way back needs of the step);  back: (that, label[t], a_{t-1}) -> label[t-1]
    if transitions is None:
        neg = dtype(-cost)
        kept = np.zeros((m, c), bool)                                            # stay_t
        step = lambda v: (np.maximum(v, neg), v >= neg)
        back = lambda stay, lab, a: lab if stay[lab] else a
    else:
        trans = check_transitions(transitions, c, "viterbi_labels").astype(dtype)
        diag, cls = np.diagonal(trans), np.arange(c)
        kept = np.zeros((m, c), np.int64)                                        # b_t

        def step(v):
            cand = v[:, None] + trans                                            # [p, c], every sum rounded to dtype
            w = cand.max(0)
            return w, np.where(v + diag == w, cls, cand.argmax(0))               # staying wins a tie, else the smallest p
        back = lambda b, lab, a: b[lab]
    label = np.zeros(m, np.int64)
    if not m:
        return label
    q = logits[rows].astype(dtype)
    e = q - q.max(1, keepdims=True)
    amax = np.zeros(m, np.int64)
    for first, end in zip(bounds[:-1], bounds[1:]):
        v = e[first]
        amax[first] = int(np.argmax(v))                                          # (numpy's argmax is the first maximum)
        for t in range(first + 1, end):
            w, kept[t] = step(v)
            u = e[t] + w
            v = u - u.max()
            amax[t] = int(np.argmax(v))
        lab = amax[end - 1]
        label[end - 1] = lab
        for t in range(end - 1, first, -1):
            lab = back(kept[t], lab, amax[t - 1])
            label[t - 1] = lab
    return label


def hmm_posteriors(logits, rows, start, transitions, dtype=np.float64):
    """The posterior marginals behind ``EventDecoder.decode(..., transitions=..., posteriors=True)`` on the host, in ``dtype`` arithmetic
    (docs/kernels.md "Event scores from posteriors"): ``gamma[t, c] = P(label_t = c | every position of the video)`` under the HMM with
    emissions ``e_t = q_t - max(q_t)``, ``q_t = logits[clip(rows[t], 0, N - 1)]``, and transition scores ``T`` (``check_transitions``),
    per video, in the log domain.  ``LSE(x) = mx + ln(sum_i exp(x_i - mx))``, ``mx = max(x)``, the sum in ascending ``i``, a ``-inf`` term
    adding 0 and all ``-inf`` giving ``-inf``.  Forward ``a_0 = e_0``, ``a_t[c] = e_t[c] + LSE_p(ah_{t-1}[p] + T[p, c])``, ``ah_t = a_t -
    max(a_t)``; backward ``b_{L-1} = 0``, ``b_t[p] = LSE_c(T[p, c] + (e_{t+1}[c] + bh_{t+1}[c]))``, ``bh_t = b_t - max(b_t)``;
    ``gamma_t = softmax(ah_t + bh_t)``: maximum subtracted, ``exp``, the sum in ascending ``c``, one division per value.  The finite
    diagonal keeps every ``b_t[p]`` and at least one ``a_t[c]`` finite, so nothing is clamped.  A Python loop over the positions.
    -> ``gamma (M, C)`` of ``dtype``."""
    dtype = np.dtype(dtype).type
    logits, rows, bounds = _viterbi_positions(logits, rows, start, "hmm_posteriors")
    m, c = len(rows), logits.shape[1]
    trans = check_transitions(transitions, c, "hmm_posteriors").astype(dtype)
    gamma = np.zeros((m, c), dtype)
    if not m:
        return gamma
    zero = dtype(0)

    def lse(x):                                                                  # over axis 0, whose slices numpy adds in ascending order
        mx = x.max(0)
        mx = np.where(np.isneginf(mx), zero, mx)
        return mx + np.log(np.exp(x - mx).sum(0))
    q = logits[rows].astype(dtype)
    e = q - q.max(1, keepdims=True)
    trans_t = np.ascontiguousarray(trans.T)                                      # [c, p]: the backward sum runs over axis 0 as well
    ah, bh = np.zeros((m, c), dtype), np.zeros((m, c), dtype)
    with np.errstate(divide="ignore"):                                           # (ln 0 = -inf is the definition's)
        for first, end in zip(bounds[:-1], bounds[1:]):
            ah[first] = e[first]                                                 # (its maximum is 0)
            for t in range(first + 1, end):
                a = e[t] + lse(ah[t - 1][:, None] + trans)
                ah[t] = a - a.max()
            for t in range(end - 2, first - 1, -1):
                b = lse(trans_t + (e[t + 1] + bh[t + 1])[:, None])
                bh[t] = b - b.max()
    g = np.ascontiguousarray((ah + bh).T)                                        # (C, M): sums over axis 0 run in ascending c
    x = np.exp(g - g.max(0))
    return np.ascontiguousarray((x / x.sum(0)).T)


def _viterbi_positions(logits, rows, start, who):
    """the argument checks of ``viterbi_labels`` -> ``(logits (N, C), rows (M,) clipped into [0, N), the videos' bounds [0, ..., M])``"""
    logits = np.asarray(logits)
    if logits.ndim != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"{who}: logits must be (N, C), got {logits.shape}")
    rows = np.clip(np.asarray(rows, np.int64).reshape(-1), 0, logits.shape[0] - 1)
    begins = np.asarray(start).reshape(-1) != 0
    if len(rows) != len(begins):
        raise ValueError(f"{who}: {len(rows)} rows for {len(begins)} start flags")
    bounds = np.flatnonzero(begins).tolist()
    if not bounds or bounds[0] != 0:
        bounds = [0] + bounds
    bounds.append(len(rows))
    return logits, rows, bounds


def save_events(file_path, video, first_frame, last_frame, cls, score, peak, first_sample, last_sample, gt_video, gt_first_frame,
                gt_last_frame, gt_cls, smooth, tiou, precision, recall, f1, switch_cost=None, transitions=None, posteriors=None):
    """One ``.npz`` of flat arrays (``np.load(..., allow_pickle=False)`` reads it).  Per predicted event ``video`` (unicode),
    ``first_frame`` / ``last_frame`` (frame numbers, inclusive), ``cls``, ``score`` the mean and ``peak`` the maximum of the smoothed
    score of ``cls``, ``first_sample`` / ``last_sample`` (dataset indices of the two end frames); per ground-truth event ``gt_video``,
    ``gt_first_frame``, ``gt_last_frame``, ``gt_cls``; ``smooth`` the window width, ``tiou (T,)`` the thresholds and ``precision``,
    ``recall``, ``f1`` (T, classes) of ``metrics.events.EventPRF1``.  A run of the background class is an event too, and smoothing
    moves boundaries by up to (smooth - 1) / 2 frames.  ``switch_cost`` (None: the file has no such column): the label-switch penalty the
    events were decoded with, a float64 scalar; ``score`` and ``peak`` are then of the unsmoothed probability.  ``transitions`` (None:
    the file has no such column): the (classes, classes) float32 transition scores the events were decoded with, ``[from, to]``.
    ``posteriors`` (None: the file has no such column; needs ``switch_cost`` or ``transitions``): a bool scalar, true where ``score`` and
    ``peak`` are of the posterior probability of ``cls`` under the path's HMM (``hmm_posteriors``)."""
    i64 = lambda a: np.asarray(a, np.int64).reshape(-1)
    f32 = lambda a: np.asarray(a, np.float32).reshape(-1)
    txt = lambda a: np.asarray(list(a), dtype=np.str_).reshape(-1)
    cols = dict(video=txt(video), first_frame=i64(first_frame), last_frame=i64(last_frame), cls=i64(cls), score=f32(score), peak=f32(peak),
                first_sample=i64(first_sample), last_sample=i64(last_sample), gt_video=txt(gt_video), gt_first_frame=i64(gt_first_frame),
                gt_last_frame=i64(gt_last_frame), gt_cls=i64(gt_cls), smooth=np.asarray(int(smooth), np.int64),
                tiou=np.asarray(tiou, np.float64).reshape(-1), precision=np.asarray(precision, np.float64),
                recall=np.asarray(recall, np.float64), f1=np.asarray(f1, np.float64))
    n, g, t = len(cols["video"]), len(cols["gt_video"]), len(cols["tiou"])
    for k in ("first_frame", "last_frame", "cls", "score", "peak", "first_sample", "last_sample"):
        if len(cols[k]) != n:
            raise ValueError(f"save_events: {k} has {len(cols[k])} entries for {n} events")
    for k in ("gt_first_frame", "gt_last_frame", "gt_cls"):
        if len(cols[k]) != g:
            raise ValueError(f"save_events: {k} has {len(cols[k])} entries for {g} ground-truth events")
    for k in ("precision", "recall", "f1"):
        if cols[k].ndim != 2 or cols[k].shape[0] != t:
            raise ValueError(f"save_events: {k} must be ({t}, classes), got {cols[k].shape}")
    if switch_cost is not None:
        cols["switch_cost"] = np.asarray(float(switch_cost), np.float64)
    if transitions is not None:
        cols["transitions"] = check_transitions(transitions, cols["f1"].shape[1], "save_events")
    if posteriors is not None:
        if switch_cost is None and transitions is None:
            raise ValueError("save_events: posteriors are those of a path's HMM, give switch_cost or transitions")
        cols["posteriors"] = np.asarray(bool(posteriors), np.bool_)
    os.makedirs(os.path.dirname(os.path.abspath(file_path)), exist_ok=True)
    np.savez(file_path, **cols)


def load_events(file_path):
    """-> dict of ``save_events``' arrays (``EVENT_COLUMNS``)."""
    with np.load(file_path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    missing = [k for k in EVENT_COLUMNS if k not in d]
    if missing:
        raise ValueError(f"{file_path}: not a file of save_events (no {', '.join(missing)})")
    return d


def decode_split(dataset, logits, order=None, smooth=1, tious=(0.1, 0.3, 0.5), decoder=None, switch_cost=None, transitions=None,
                 posteriors=False):
    """The events of one evaluated split: ``logits`` (N, classes) fp32 ON THE GPU, row r the logits of sample ``order[r]`` (None:
    of sample r).  The positions are time-ordered on the host (``time_order``), decoded on the device (``engine.EventDecoder``; only
    the events come back), the ground truth is ``label_runs`` of the samples' labels, both are scored with ``EventPRF1``.
    ``switch_cost`` (None: per-frame arg-max of the smoothed scores) goes to the decoder and into the columns, and so does
    ``transitions`` (None: no transition matrix; (classes, classes), see ``EventDecoder.decode``).  ``posteriors`` (with one of the
    two, ``smooth`` 1): ``score`` and ``peak`` are of the posterior probability under the path's HMM, and the columns say so.
    -> ``(columns of save_events, EventPRF1)``."""
    if posteriors and switch_cost is None and transitions is None:
        raise ValueError("decode_split: posteriors are those of a path's HMM, give switch_cost or transitions")
    if posteriors and int(smooth) != 1:
        raise ValueError(f"decode_split: posteriors score a path of the unsmoothed scores, not together with smooth={smooth}")
    from .engine import EventDecoder
    from .metrics.events import EventPRF1
    rows, start, video, frame = time_order(dataset, order)
    order = np.arange(len(dataset._samples)) if order is None else np.asarray(order, np.int64).reshape(-1)
    decoder = decoder or EventDecoder(len(rows), logits.shape[1])
    path = {} if switch_cost is None else {"switch_cost": float(switch_cost)}    # (without it the call is the call it was)
    if transitions is not None:
        path["transitions"] = check_transitions(transitions, logits.shape[1], "decode_split")
    how = {"posteriors": True} if posteriors else {}                             # (without it the call is the call it was)
    ev = {k: v.cpu().numpy() for k, v in decoder.decode(logits, rows, start, smooth=smooth, **path, **how).items()}
    first, last = ev["first"].astype(np.int64), ev["last"].astype(np.int64)
    labels = np.asarray([dataset.classes.index(dataset._samples[int(i)][2]) for i in order[rows]], np.int64)
    gfirst, glast, gcls = label_runs(labels, start)
    pred = dict(video=video[first], first_frame=frame[first], last_frame=frame[last], cls=ev["cls"].astype(np.int64), score=ev["score"])
    gt = dict(video=video[gfirst], first_frame=frame[gfirst], last_frame=frame[glast], cls=gcls)
    metric = EventPRF1(dataset.classes, tious=tious)
    metric.update(pred, gt)
    prec, rec, f1 = metric.arrays()
    cols = dict(pred, peak=ev["peak"], first_sample=order[rows[first]], last_sample=order[rows[last]], gt_video=gt["video"],
                gt_first_frame=gt["first_frame"], gt_last_frame=gt["last_frame"], gt_cls=gt["cls"], smooth=int(smooth),
                tiou=np.asarray(metric.tious), precision=prec, recall=rec, f1=f1, **path, **how)
    return cols, metric


def event_table(cols, classes, limit=40):
    """The printed form of ``decode_split``'s columns: one line per predicted event (the first ``limit``), then the scores."""
    n = len(cols["video"])
    how = "smooth %d" % int(cols["smooth"]) if cols.get("switch_cost") is None else "switch cost %g" % float(cols["switch_cost"])
    if cols.get("transitions") is not None:
        how = "transition matrix"
    if cols.get("posteriors") is not None and bool(cols["posteriors"]):
        how += ", posterior scores"
    lines = ["Events: %d predicted, %d ground truth (%s)" % (n, len(cols["gt_video"]), how)]
    for i in range(min(n, limit)):
        lines.append("  %s\t%s\tframes %d-%d\tscore %.3f\tpeak %.3f" % (cols["video"][i], classes[int(cols["cls"][i])],
                                                                      cols["first_frame"][i], cols["last_frame"][i],
                                                                      cols["score"][i], cols["peak"][i]))
    if n > limit:
        lines.append("  ... %d more" % (n - limit))
    return "\n".join(lines)
