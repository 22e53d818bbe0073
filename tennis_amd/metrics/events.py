"""Event-level precision / recall / F1 at temporal-IoU thresholds (no counterpart in the reference, which scores frames only).

Events are (video, first_frame, last_frame, cls[, score]) with inclusive frame numbers.  Matching runs per tIoU threshold, per video
and class: the predictions are taken in descending ``score`` (a tie goes to the earlier ``first_frame``), each takes the still
unmatched ground-truth event of its video and class with the largest tIoU (a tie goes to the earlier one) and is a true positive if
that tIoU reaches the threshold, a false positive otherwise; unmatched ground truth counts as false negatives.
  tIoU: inter = max(0, min(l1, l2) - max(f1, f2) + 1), union = len1 + len2 - inter, on inclusive frame numbers.
Runs on the host: the events are few.
"""
import numpy as np


def tiou(f1, l1, f2, l2):
    """Temporal IoU of the inclusive frame ranges [f1, l1] and [f2, l2] (scalars or arrays)."""
    inter = np.maximum(0, np.minimum(l1, l2) - np.maximum(f1, f2) + 1)
    union = (l1 - f1 + 1) + (l2 - f2 + 1) - inter
    return inter / union


class EventPRF1:
    def __init__(self, classes, tious=(0.1, 0.3, 0.5), ignore=()):
        self.classes = list(classes)
        self.tious = tuple(float(t) for t in tious)
        self.ignore = tuple(ignore)
        unknown = [c for c in self.ignore if c not in self.classes]
        if unknown:
            raise ValueError(f"EventPRF1: ignore names unknown classes {unknown}")
        self.reset()

    def reset(self):
        n = len(self.classes)
        self.tp = np.zeros((len(self.tious), n), np.int64)
        self.fp = np.zeros_like(self.tp)
        self.fn = np.zeros_like(self.tp)

    def update(self, pred, gt):
        """``pred``: dict of equally long arrays ``video``, ``first_frame``, ``last_frame``, ``cls``, ``score``; ``gt``: the same
        without ``score``.  Adds one split's counts."""
        pv, gv = np.asarray(pred["video"]).astype(str), np.asarray(gt["video"]).astype(str)
        pf, pl, pc = (np.asarray(pred[k], np.int64) for k in ("first_frame", "last_frame", "cls"))
        gf, gl, gc = (np.asarray(gt[k], np.int64) for k in ("first_frame", "last_frame", "cls"))
        ps = np.asarray(pred["score"], np.float64)
        for v in sorted(set(pv) | set(gv)):
            for c in range(len(self.classes)):
                p = np.flatnonzero((pv == v) & (pc == c))
                g = np.flatnonzero((gv == v) & (gc == c))
                g = g[np.argsort(gf[g], kind="stable")]
                p = p[np.lexsort((pf[p], -ps[p]))]                     # descending score, then earlier first_frame
                for ti, thr in enumerate(self.tious):
                    free = np.ones(len(g), bool)
                    for i in p:
                        hit = False
                        if free.any():
                            cand = np.flatnonzero(free)
                            iou = tiou(pf[i], pl[i], gf[g[cand]], gl[g[cand]])
                            j = int(np.argmax(iou))                    # (first maximum: the earlier event)
                            if iou[j] >= thr:
                                free[cand[j]] = False
                                hit = True
                        if hit:
                            self.tp[ti, c] += 1
                        else:
                            self.fp[ti, c] += 1
                    self.fn[ti, c] += int(free.sum())

    def arrays(self):
        """(precision, recall, f1), each (len(tious), len(classes)) float64; 0 where the denominator is."""
        tp = self.tp.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            prec = np.where(tp + self.fp > 0, tp / (tp + self.fp), 0.0)
            rec = np.where(tp + self.fn > 0, tp / (tp + self.fn), 0.0)
            f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        return prec, rec, f1

    def get(self):
        """[(name, value)]: per threshold ``<class>_prec|rec|f1@t`` of every class and the micro average ``AVG_prec|rec|f1@t`` (counts
        summed over the classes not in ``ignore``)."""
        prec, rec, f1 = self.arrays()
        keep = [i for i, c in enumerate(self.classes) if c not in self.ignore]
        out = []
        for ti, t in enumerate(self.tious):
            for i, c in enumerate(self.classes):
                out += [(f"{c}_prec@{t:g}", prec[ti, i]), (f"{c}_rec@{t:g}", rec[ti, i]), (f"{c}_f1@{t:g}", f1[ti, i])]
            tp, fp, fn = (float(a[ti, keep].sum()) for a in (self.tp, self.fp, self.fn))
            p = tp / (tp + fp) if tp + fp > 0 else 0.0
            r = tp / (tp + fn) if tp + fn > 0 else 0.0
            out += [(f"AVG_prec@{t:g}", p), (f"AVG_rec@{t:g}", r), (f"AVG_f1@{t:g}", 2 * p * r / (p + r) if p + r > 0 else 0.0)]
        return out
