"""float64 reference of the opt-in global-norm gradient clipping (``gluon.utils.clip_global_norm`` [EXT]) and of the two updates
that run behind it, carried over several steps from zero optimizer state:

    norm  = sqrt(sum over every trainable gradient element of (r g)^2)       r = rescale_grad (SGD), 1 (Adam)
    scale = min(1, max_norm / (norm + 1e-8))
    SGD:  mom = momentum mom - lr (r scale g + wd w);  w += mom              (MXNet sgd_mom_update)
    Adam: g' = scale g;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps)

Gradients and parameters are dicts of arrays (or anything ``np.asarray`` takes); one norm spans every entry of ``grads``.  Also the
error bound of the library's two-stage sum of squares, from the constants its debug header states."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def global_norm(grads, rescale: float = 1.0) -> float:
    """sqrt(sum (rescale g)^2) over every array of ``grads`` (a dict or a sequence), in float64"""
    arrays = grads.values() if isinstance(grads, dict) else grads
    return abs(float(rescale)) * math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in arrays))


def clip_scale(norm: float, max_norm: float) -> float:
    """min(1, max_norm / (norm + 1e-8)); a NaN norm gives NaN, an infinite one 0"""
    return float(np.minimum(1.0, np.float64(max_norm) / (np.float64(norm) + 1e-8)))


class ClippedSGD:
    """MXNet SGD with momentum over named float64 parameters, the gradient clipped to ``max_norm`` (None: not clipped)"""

    def __init__(self, params, lr, momentum, wd, rescale, max_norm=None):
        self.w = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
        self.mom = {k: np.zeros_like(v) for k, v in self.w.items()}
        self.lr, self.momentum, self.wd, self.rescale, self.max_norm = lr, momentum, wd, rescale, max_norm
        self.norms, self.scales = [], []

    def step(self, grads):
        norm = global_norm(grads, self.rescale)
        scale = 1.0 if self.max_norm is None else clip_scale(norm, self.max_norm)
        self.norms.append(norm)
        self.scales.append(scale)
        for k, g in grads.items():
            g = np.asarray(g, np.float64).reshape(self.w[k].shape)
            self.mom[k] = self.momentum * self.mom[k] - self.lr * (self.rescale * scale * g + self.wd * self.w[k])
            self.w[k] = self.w[k] + self.mom[k]
        return self.w


class ClippedAdam:
    """MXNet Adam (bias correction folded into the rate, no weight decay, rescale_grad 1) over named float64 parameters"""

    def __init__(self, params, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, max_norm=None):
        self.w = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.w.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.w.items()}
        self.lr, self.b1, self.b2, self.eps, self.max_norm, self.t = lr, beta1, beta2, epsilon, max_norm, 0
        self.norms, self.scales = [], []

    def step(self, grads):
        norm = global_norm(grads)
        scale = 1.0 if self.max_norm is None else clip_scale(norm, self.max_norm)
        self.norms.append(norm)
        self.scales.append(scale)
        self.t += 1
        lr_t = self.lr * math.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for k, g in grads.items():
            g = scale * np.asarray(g, np.float64).reshape(self.w[k].shape)
            self.m[k] = self.b1 * self.m[k] + (1.0 - self.b1) * g
            self.v[k] = self.b2 * self.v[k] + (1.0 - self.b2) * g * g
            self.w[k] = self.w[k] - lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps)
        return self.w


def kernel_constants() -> dict:
    """TN_GRAD_SUMSQ_BLOCK / _CHUNK / _GRID as include/tennis_hip_debug.h states them"""
    text = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    out = {}
    for name in ("BLOCK", "CHUNK", "GRID"):
        m = re.search(r"#define\s+TN_GRAD_SUMSQ_%s\s+(\d+)" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def sumsq_rel_bound(counts) -> float:
    """The bound on the relative error of the library's sum of squares over segments of ``counts`` floats, (L + log2(P) + 1) 2^-24:
    every term is a non-negative fp32 square (one rounding, the + 1; none where the square is fused into the add), a thread adds
    L of them serially - CHUNK / BLOCK per chunk it walks, ceil(chunks / GRID) chunks of the longest segment per segment, one head
    or tail float more per segment - and P = BLOCK thread partials meet in an fp32 tree of log2(P) levels.  The GRID workgroup
    results are added in double (2^-53 per add: nothing at this scale)."""
    c = kernel_constants()
    per_chunk = c["CHUNK"] // c["BLOCK"]
    L = 0
    for n in counts:
        if n > 0:
            chunks = -(-n // c["CHUNK"])
            L += per_chunk * (-(-chunks // c["GRID"])) + 1
    return (L + math.log2(c["BLOCK"]) + 1) * 2.0 ** -24
