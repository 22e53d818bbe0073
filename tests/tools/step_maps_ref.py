"""Float64 references for the temporal activation maps (csrc/step_maps.hip, the ARG form of csrc/rnn_window.hip).

``head_sequence``: the whole hidden sequence ``h (S, T, 2H)`` of the bi-GRU / bi-LSTM head on materialised windows - the equations of
oracle/rnn_np.py (GRU gates [r, z, n], LSTM gates [i, f, g, o]), zero initial state, the reverse direction walking t downwards and
storing its state at the t it read.  ``first_max``: the first-maximum step and the pooled value per unit.  ``step_maps``: the maps
from given ``pooled`` and ``steps``; ``step_maps_abs`` the same sum of absolute terms and the bucket sizes (for error bounds)."""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def head_sequence(x, p, mode, rnn_prefix):
    """x (S, T, F) -> h (S, T, 2H) float64 = concat(forward, backward) states at every window position"""
    x = np.asarray(x, np.float64)
    S, T, _ = x.shape
    halves = []
    for d, rev in (("l0_", False), ("r0_", True)):
        wi, wh = (np.asarray(p[rnn_prefix + d + n], np.float64) for n in ("i2h_weight", "h2h_weight"))
        bi, bh = (np.asarray(p[rnn_prefix + d + n], np.float64) for n in ("i2h_bias", "h2h_bias"))
        hid = wh.shape[1]
        h, c = np.zeros((S, hid)), np.zeros((S, hid))
        seq = np.zeros((S, T, hid))
        for t in (range(T - 1, -1, -1) if rev else range(T)):
            gi, gh = x[:, t] @ wi.T + bi, h @ wh.T + bh
            if mode == "gru":
                r = _sig(gi[:, :hid] + gh[:, :hid])
                z = _sig(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])
                n = np.tanh(gi[:, 2 * hid:] + r * gh[:, 2 * hid:])
                h = (1 - z) * n + z * h
            else:
                g = gi + gh
                c = _sig(g[:, hid:2 * hid]) * c + _sig(g[:, :hid]) * np.tanh(g[:, 2 * hid:3 * hid])
                h = _sig(g[:, 3 * hid:]) * np.tanh(c)
            seq[:, t] = h
        halves.append(seq)
    return np.concatenate(halves, 2)


def first_max(h):
    """h (S, T, K) -> (steps (S, K) int64 the smallest t that holds the maximum, pooled (S, K))"""
    steps = np.argmax(h, axis=1)                 # numpy returns the first occurrence
    return steps, np.take_along_axis(h, steps[:, None, :], 1)[:, 0]


def margin(h):
    """h (S, T, K) -> (S, K): best minus second-best value over the steps (inf for T == 1)"""
    if h.shape[1] == 1:
        return np.full((h.shape[0], h.shape[2]), np.inf)
    top = np.sort(h, axis=1)
    return top[:, -1] - top[:, -2]


def step_maps(pooled, steps, w, window):
    """pooled (B, K), steps (B, K) int, w (C, K) -> tam (B, C, window) float64; steps outside [0, window) contribute nothing"""
    return _maps(np.asarray(pooled, np.float64)[:, None, :] * np.asarray(w, np.float64)[None], np.asarray(steps), window)


def step_maps_abs(pooled, steps, w, window):
    """-> (sum of |w * pooled| per bucket (B, C, window), bucket sizes (B, window))"""
    steps = np.asarray(steps)
    terms = np.abs(np.asarray(pooled, np.float64)[:, None, :] * np.asarray(w, np.float64)[None])
    sizes = np.stack([(steps == t).sum(1) for t in range(window)], 1)
    return _maps(terms, steps, window), sizes


def _maps(terms, steps, window):
    B, C, K = terms.shape
    out = np.zeros((B, C, window))
    for t in range(window):
        out[:, :, t] = (terms * (steps == t)[:, None, :]).sum(2)
    return out
