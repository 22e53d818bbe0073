"""Shapes and inputs of the operator tests of the training steps (tests/test_cpu_train_ops_ref.py pins the float64 references on
them, tests/test_gpu_train_ops.py holds the kernels to the references on them).  Every generator is deterministic, returns float32
(labels, lengths: int32) and builds the properties a case must have in, so that the assertions on them cannot depend on a seed:
a tied window, a closed ReLU, a zero scale.  NHWC throughout."""
import numpy as np

U = 2.0 ** -24                        # the unit roundoff of float32

# (B, H, W): non-square both ways, one pixel, one row, one column, more than one 256-thread block
IM2COL7_SHAPES = [(1, 2, 2), (2, 4, 6), (3, 6, 4), (1, 14, 10), (2, 32, 32)]
IM2COL3_SHAPES = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 2, 3), (1, 7, 7), (2, 14, 16)]
IM2COL3_C = (4, 32, 128)
POOL_SHAPES = IM2COL7_SHAPES
POOL_C = (1, 3, 64)
POOL_KINDS = ("ties", "equal", "negative", "random")
GAP_SHAPES = [(1, 1, 4), (5, 7, 33), (3, 49, 1024), (2, 256, 100)]          # (B, P, C)
BN_C = (1, 255, 256, 257, 1024)
POOLT_SHAPES = [(1, 1, 1), (3, 7, 5), (2, 16, 256), (5, 9, 300)]           # (B, T, F)
CE_SHAPES = [(1, 2), (63, 11), (64, 11), (65, 11), (7, 254), (3, 1000)]    # (B, C)
CE_KINDS = ("normal", "shift+80", "shift-80", "const1e4", "spread60", "equal")
DENSE_SHAPES = [(1, 1, 1), (64, 3, 5), (32, 11, 256), (2, 11, 1024), (5, 300, 7)]   # (B, C, K)
COLSUM_ROWS = (1, 15, 16, 17, 255, 256, 257, 4099)
COLSUM_COLS = (1, 63, 64, 65, 254)
COLSUM_LONG = (20000, 1, 1)                                                # (rows, cols, lda)
OPT_N = (1, 255, 256, 257, 100003)
ADAM_STEPS = (1, 2, 10 ** 6)
CLIP_SCALE = 0.37
STAGE_SHAPES = [(1, 1, 4), (2, 3, 12), (3, 5, 1200), (2, 4, 65544)]        # (B, T, frame_floats); 65544 / 4 > 64 * 256
TRANSPOSE_SHAPES = [(1, 1), (1, 7), (7, 1), (32, 1152), (129, 255)]


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def normal(shape, *key, scale=1.0):
    return (_rng(*key).standard_normal(shape) * scale).astype(np.float32)


def integers(shape, lo, hi, *key):
    """integers of [lo, hi] as float32"""
    return _rng(*key).integers(lo, hi + 1, shape).astype(np.float32)


# ---- im2col3's folded source -----------------------------------------------------------------------------------------------------

def fold_inputs(B, H, W, C, seed=0):
    """a (B, H, W, C), sc, sh (C): channel 0 has sc = 0 (its pre-activation is sh[0] > 0 everywhere), channel 1 a negative sc, and
    the sign of every other pre-activation is set by construction: a = (t - sh) / sc with |t| in [0.25, 2] and the sign of t
    alternating along (pixel + channel), so half of those ReLUs are closed whatever the seed."""
    r = _rng(3, B, H, W, C, seed)
    sc = (r.uniform(0.5, 2.0, C) * r.choice([-1.0, 1.0], C)).astype(np.float32)
    sh = r.uniform(-1.0, 1.0, C).astype(np.float32)
    sc[0], sh[0] = 0.0, 0.5
    sc[1] = -abs(sc[1])
    pix = np.arange(B * H * W).reshape(B, H, W, 1)
    sign = np.where((pix + np.arange(C)) % 2 == 0, 1.0, -1.0)
    t = r.uniform(0.25, 2.0, (B, H, W, C)) * sign
    a = np.where(sc != 0, (t - sh.astype(np.float64)) / np.where(sc != 0, sc, 1).astype(np.float64), r.standard_normal((B, H, W, C)))
    return a.astype(np.float32), sc, sh


def fold_preactivation(a, sc, sh):
    """float64 a sc + sh and the width 2u (|a sc| + |sh|) inside which one fmaf may put it on the other side of zero"""
    a, sc, sh = (np.asarray(v, dtype=np.float64) for v in (a, sc, sh))
    return a * sc + sh, 2 * U * (np.abs(a * sc) + np.abs(sh))


def fold_fractions(a, sc, sh):
    """(fraction of pre-activations below zero, above zero, elements whose sign one rounding could flip)"""
    pre, width = fold_preactivation(a, sc, sh)
    return float((pre < 0).mean()), float((pre > 0).mean()), int((np.abs(pre) <= width).sum())


# ---- pools -----------------------------------------------------------------------------------------------------------------------

def pool_input(kind, B, H, W, C, seed=0):
    if kind == "ties":
        a = integers((B, H, W, C), 0, 3, 5, B, H, W, C, seed)
        a[:, 0, 0, :] = 3.0                  # the first window of every frame holds its maximum twice,
        a[:, 1, 1, :] = 3.0                  # at its first and at its last pixel inside the frame
        return a
    if kind == "equal":
        return np.full((B, H, W, C), 2.5, np.float32)
    if kind == "negative":
        return -np.abs(normal((B, H, W, C), 6, B, H, W, C, seed)) - np.float32(0.125)
    return normal((B, H, W, C), 7, B, H, W, C, seed)


def tied_window_fraction(a):
    """fraction of the 3x3 stride 2 pad 1 windows of a (B, H, W, C) whose maximum is held by more than one pixel"""
    B, H, W, C = a.shape
    ap = np.pad(a.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-np.inf)
    Ho, Wo = H // 2, W // 2
    win = np.stack([ap[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :] for ky in range(3) for kx in range(3)], axis=3)
    return float(((win == win.max(axis=3, keepdims=True)).sum(axis=3) > 1).mean())


def poolt_input(kind, B, T, F, seed=0):
    if kind == "ties":
        x = integers((B, T, F), 0, 3, 8, B, T, F, seed)
        if T > 1:
            x[:, 0, ::2] = 3.0               # every other column holds its maximum at its first and its last step
            x[:, T - 1, ::2] = 3.0
        return x
    return normal((B, T, F), 9, B, T, F, seed)


def tied_column_fraction(x):
    return float(((x == x.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean())


# ---- BatchNorm fold / running statistics ------------------------------------------------------------------------------------------

def bn_inputs(C, seed=0):
    """mean (up to 50), var (0, 1e-12, 1, 1e6 in turn), gamma (negative, zero and positive), beta, running mean / var"""
    r = _rng(10, C, seed)
    mean = r.uniform(-50.0, 50.0, C).astype(np.float32)
    mean[C // 2] = 50.0
    var = np.array([0.0, 1e-12, 1.0, 1e6], np.float32)[(np.arange(C) + seed) % 4]
    gamma = r.standard_normal(C).astype(np.float32)
    gamma[::3] = -np.abs(gamma[::3]) - np.float32(0.1)
    gamma[1::5] = 0.0
    beta = r.standard_normal(C).astype(np.float32)
    rmean = r.standard_normal(C).astype(np.float32) * 10
    rvar = r.uniform(0.0, 4.0, C).astype(np.float32)
    return mean, var, gamma, beta, rmean, rvar


# ---- softmax cross-entropy --------------------------------------------------------------------------------------------------------

def ce_inputs(B, C, rot=0, seed=0):
    """logits (B, C) whose row b is of kind CE_KINDS[(b + rot) % 6], labels (B) that use every class where B >= C"""
    r = _rng(11, B, C, rot, seed)
    p = r.standard_normal((B, C))
    for b in range(B):
        kind = CE_KINDS[(b + rot) % len(CE_KINDS)]
        if kind == "shift+80":
            p[b] += 80.0
        elif kind == "shift-80":
            p[b] -= 80.0
        elif kind == "const1e4":
            p[b] = 1e4
        elif kind == "spread60":
            p[b] = r.uniform(-60.0, 60.0, C)
            at = int(r.integers(C))
            p[b, at], p[b, (at + 1) % C] = 60.0, -60.0              # exp(-120) underflows in float32
        elif kind == "equal":
            p[b] = 0.75
    labels = ((np.arange(B) * 7 + rot) % C).astype(np.int32)            # 7 is coprime to every C of CE_SHAPES
    return p.astype(np.float32), labels


# ---- optimisers -------------------------------------------------------------------------------------------------------------------

def opt_inputs(n, seed=0):
    """w, g, mom / m, v (n): gradients with exact zeros and magnitudes from 1e-12 to 1e6"""
    r = _rng(12, n, seed)
    g = (10.0 ** r.uniform(-12.0, 6.0, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    g[3::7] = 0.0
    if n > 2:
        g[1], g[2] = 1e-12, -1e6
    w = r.standard_normal(n).astype(np.float32)
    m = (r.standard_normal(n) * 0.1).astype(np.float32)
    v = (r.uniform(0.0, 1.0, n) ** 4).astype(np.float32)
    m[::5], v[::5] = 0.0, 0.0
    return w, g, m, v


# ---- frame staging ----------------------------------------------------------------------------------------------------------------

def stage_inputs(B, T, frame, rot=0, seed=0):
    """x (B, T, frame) with NaN in the slots at or past valid_len, valid_len (B) from {0, 1, T, T + 2} in turn"""
    x = normal((B, T, frame), 13, B, T, frame % 9973, seed)
    valid = np.array([0, 1, T, T + 2], np.int32)[(np.arange(B) + rot) % 4]
    for b in range(B):
        x[b, min(int(valid[b]), T):] = np.nan
    return x, valid
