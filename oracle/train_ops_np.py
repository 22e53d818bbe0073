"""ORACLE (test infrastructure only) - float64 NumPy definitions of the small operators that carry a training step from one GEMM
to the next (csrc/finetune.hip ft_*, csrc/train.hip), one function per operator, written from the operators' definitions:

  im2col / col2im, pools, global average   gluon nn.Conv2D / MaxPool2D(3, 2, 1) / AvgPool2D(2, 2) / GlobalAvgPool2D of DenseNet-121
                                           on NHWC activations, column order (ky, kx, c)  (models/vision/definitions.py) [EXT]
  BatchNorm fold, running statistics       gluon nn.BatchNorm(momentum=0.9, epsilon=1e-5) [EXT]
  max over time                            CNNRNN's temp_pool (definitions.py:94-110); MXNet routes the gradient of a max to ONE element
  softmax cross-entropy                    gluon.loss.SoftmaxCrossEntropyLoss, sparse labels, per sample (train.py:324) [EXT]
  sgd_mom_update, adam_update              gluon.Trainer 'sgd' / 'adam' (train.py:298-299, train_gnmt.py:310,337) [EXT]
  frame staging                            Pad() of a clip behind its valid length (utils/captioning.py:33)

Ties: a pooled maximum that several elements share sends its gradient to the FIRST of them in scan order ((ky, kx) for the
spatial pool, t for the pool over time) - the documented rule of the kernels; tests/test_cpu_train_ops_ref.py says where torch
differs.  Every function takes array-likes, computes in float64 and returns float64 (indices int64).
Pinned against float64 torch by tests/test_cpu_train_ops_ref.py.  Only tests/ may import this module.
"""
from __future__ import annotations

import numpy as np

BN_EPS = 1e-5
BN_MOMENTUM = 0.9


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _pad_hw(a, p, value=0.0):
    return np.pad(a, ((0, 0), (p, p), (p, p), (0, 0)), constant_values=value)


def im2col(a, k, stride, pad):
    """a (B, H, W, C) -> (B * Ho * Wo, k * k * C), columns (ky, kx, c), zero padding"""
    a = _f64(a)
    B, H, W, C = a.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ap = _pad_hw(a, pad)
    col = np.empty((B, Ho, Wo, k, k, C))
    for ky in range(k):
        for kx in range(k):
            col[:, :, :, ky, kx, :] = ap[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride, :]
    return col.reshape(B * Ho * Wo, k * k * C)


def im2col7(x):
    """7x7 stride 2 pad 3 of (B, H, W, 3), H and W even -> (B H/2 W/2, 147)"""
    return im2col(x, 7, 2, 3)


def bn_relu(a, sc, sh):
    """relu(a * sc[c] + sh[c]) over the last axis"""
    return np.maximum(_f64(a) * _f64(sc) + _f64(sh), 0.0)


def im2col3(a, sc=None, sh=None):
    """3x3 pad 1 of (B, H, W, C) -> (B H W, 9 C); sc / sh: of relu(a sc + sh), the padding zero AFTER it"""
    return im2col(_f64(a) if sc is None else bn_relu(a, sc, sh), 3, 1, 1)


def col2im3(dcol, B, H, W, C):
    """adjoint of im2col3: dcol (B H W, 9 C) -> (B, H, W, C)"""
    d = _f64(dcol).reshape(B, H, W, 3, 3, C)
    da = np.zeros((B, H + 2, W + 2, C))
    for ky in range(3):
        for kx in range(3):
            da[:, ky:ky + H, kx:kx + W, :] += d[:, :, :, ky, kx, :]
    return da[:, 1:-1, 1:-1, :]


def _maxpool_windows(a):
    """(B, Ho, Wo, 9, C): the 3x3 stride 2 pad 1 windows in (ky, kx) order, -inf where a window leaves the frame"""
    a = _f64(a)
    B, H, W, C = a.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ap = _pad_hw(a, 1, -np.inf)
    return np.stack([ap[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :] for ky in range(3) for kx in range(3)], axis=3)


def maxpool(a):
    """3x3 stride 2 pad 1 of (B, H, W, C) -> (B, Ho, Wo, C); the padding never wins"""
    return _maxpool_windows(a).max(axis=3)


def maxpool_bwd(a, dy):
    """dy (B, Ho, Wo, C) -> da (B, H, W, C): each window's gradient to its first maximum in (ky, kx) order"""
    a = _f64(a)
    B, H, W, C = a.shape
    first = _maxpool_windows(a).argmax(axis=3)            # argmax returns the first of equal maxima
    dy = _f64(dy)
    Ho, Wo = dy.shape[1:3]
    da = np.zeros((B, H + 2, W + 2, C))
    for ky in range(3):
        for kx in range(3):
            da[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :] += np.where(first == ky * 3 + kx, dy, 0.0)
    return da[:, 1:-1, 1:-1, :]


def avgpool2(z):
    """2x2 stride 2 of (B, H, W, C), H and W even"""
    z = _f64(z)
    return 0.25 * (z[:, 0::2, 0::2] + z[:, 0::2, 1::2] + z[:, 1::2, 0::2] + z[:, 1::2, 1::2])


def avgpool2_bwd(dy):
    """dy (B, Ho, Wo, C) -> (B, 2 Ho, 2 Wo, C)"""
    return 0.25 * np.repeat(np.repeat(_f64(dy), 2, axis=1), 2, axis=2)


def gap(a):
    """a (B, P, C) -> (B, C), the mean over P"""
    return _f64(a).mean(axis=1)


def gap_bwd(df, P):
    """df (B, C) -> (B, P, C)"""
    df = _f64(df)
    return np.repeat(df[:, None, :] / P, P, axis=1)


def bn_fold(mean, var, gamma, beta):
    """-> sc = gamma / sqrt(var + eps), sh = beta - mean * sc"""
    sc = _f64(gamma) / np.sqrt(_f64(var) + BN_EPS)
    return sc, _f64(beta) - _f64(mean) * sc


def bn_running(rmean, rvar, mean, var):
    """-> the running statistics after one step"""
    return (BN_MOMENTUM * _f64(rmean) + (1.0 - BN_MOMENTUM) * _f64(mean),
            BN_MOMENTUM * _f64(rvar) + (1.0 - BN_MOMENTUM) * _f64(var))


def pool_max_arg(x):
    """x (B, T, F) -> max over T (B, F) and the first step that attains it"""
    x = _f64(x)
    return x.max(axis=1), x.argmax(axis=1)


def scatter_pool_grad(dpooled, arg, T):
    """dpooled, arg (B, F) -> (B, T, F): dpooled at step arg, zeros elsewhere"""
    dpooled, arg = _f64(dpooled), np.asarray(arg)
    return np.where(np.arange(T)[None, :, None] == arg[:, None, :], dpooled[:, None, :], 0.0)


def log_sum_exp(logits):
    """-> (row maximum, log of the sum of exp(logit - maximum)); their sum is the log-sum-exp"""
    p = _f64(logits)
    m = p.max(axis=1)
    return m, np.log(np.exp(p - m[:, None]).sum(axis=1))


def softmax_ce(logits, labels):
    """-> per-sample loss (B) and d(sum of the losses)/dlogits = softmax - onehot (B, C)"""
    p, labels = _f64(logits), np.asarray(labels, dtype=np.int64)
    m, ls = log_sum_exp(p)
    rows = np.arange(p.shape[0])
    loss = (m - p[rows, labels]) + ls
    d = np.exp(p - (m + ls)[:, None])
    d[rows, labels] -= 1.0
    return loss, d


def dense_bwd(dlogits, pooled, wd):
    """logits = pooled wd^T + bd -> dwd (C, K), dbd (C), dpooled (B, K)"""
    d, x, w = _f64(dlogits), _f64(pooled), _f64(wd)
    return d.T @ x, d.sum(axis=0), d @ w


def colsum(A):
    return _f64(A).sum(axis=0)


def sgd_momentum(w, g, mom, lr, momentum, wd, rescale, scale=1.0):
    """MXNet sgd_mom_update on (scale * rescale) g -> (w, mom)"""
    w, g, mom = _f64(w), _f64(g), _f64(mom)
    mom = momentum * mom - lr * (rescale * scale * g + wd * w)
    return w + mom, mom


def adam_rate(lr, beta1, beta2, step):
    """the rate with the bias correction of the 1-based update count folded in"""
    return lr * np.sqrt(1.0 - np.power(float(beta2), float(step))) / (1.0 - np.power(float(beta1), float(step)))


def adam(w, g, m, v, lr_t, beta1, beta2, epsilon, scale=1.0):
    """MXNet adam_update on scale * g at the folded rate lr_t -> (w, m, v)"""
    w, g, m, v = _f64(w), scale * _f64(g), _f64(m), _f64(v)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return w - lr_t * m / (np.sqrt(v) + epsilon), m, v


def stage_frames(x, valid_len):
    """x (B, T, frame) -> the same with zeros in the slots t >= valid_len[b], whatever x holds there"""
    x = _f64(x)
    keep = np.arange(x.shape[1])[None, :] < np.asarray(valid_len)[:, None]
    return np.where(keep[:, :, None], x, 0.0)


def transpose(src):
    return _f64(src).T.copy()
