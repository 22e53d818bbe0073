"""float64 reference of the class activation maps (csrc/class_maps.hip, tn_densenet121_forward_class_maps).

The network ends in BN -> ReLU -> AvgPool2D(7) -> Flatten -> Dense, so with A = relu(scale * map + shift):
  cam[b,c,y,x] = (1/49) * sum_k Wd[c, k*PH*PW + (y//7)*PW + (x//7)] * A[b,y,x,k]        0 <= y < 7*PH, 0 <= x < 7*PW
  logit[b,c]   = bias[c] + sum_{y,x} cam[b,c,y,x]
Rows and columns past 7*PH / 7*PW belong to no pool window and to no cell."""
import numpy as np


def _windows(m, scale, shift, wd, PH, PW):
    m = np.asarray(m, np.float64)
    b, h, w, c = m.shape
    assert 7 * PH <= h and 7 * PW <= w, (m.shape, PH, PW)
    wd = np.asarray(wd, np.float64)
    classes = wd.shape[0]
    assert wd.shape == (classes, c * PH * PW), (wd.shape, c, PH, PW)
    return m, np.asarray(scale, np.float64), np.asarray(shift, np.float64), wd.reshape(classes, c, PH, PW), b, classes


def cam_f64(m, scale, shift, wd, PH, PW):
    """m (B,H,W,C) NHWC, scale / shift (C), wd (classes, C*PH*PW) in NCHW-flatten order -> cam (B, classes, 7*PH, 7*PW) float64"""
    m, s, t, w4, b, classes = _windows(m, scale, shift, wd, PH, PW)
    out = np.zeros((b, classes, 7 * PH, 7 * PW))
    for ph in range(PH):
        for pw in range(PW):
            a = np.maximum(m[:, 7 * ph:7 * ph + 7, 7 * pw:7 * pw + 7, :] * s + t, 0.0)
            out[:, :, 7 * ph:7 * ph + 7, 7 * pw:7 * pw + 7] = np.einsum("byxk,ck->bcyx", a, w4[:, :, ph, pw]) / 49.0
    return out


def cam_scale_f64(m, scale, shift, wd, PH, PW):
    """S of the kernel's error bound, per cell: (1/49) * sum_k |Wd| * (|scale * v| + |shift|) -> (B, classes, 7*PH, 7*PW)"""
    m, s, t, w4, b, classes = _windows(m, scale, shift, wd, PH, PW)
    out = np.zeros((b, classes, 7 * PH, 7 * PW))
    for ph in range(PH):
        for pw in range(PW):
            a = np.abs(m[:, 7 * ph:7 * ph + 7, 7 * pw:7 * pw + 7, :] * s) + np.abs(t)
            out[:, :, 7 * ph:7 * ph + 7, 7 * pw:7 * pw + 7] = np.einsum("byxk,ck->bcyx", a, np.abs(w4[:, :, ph, pw])) / 49.0
    return out


def logits_f64(m, scale, shift, wd, bias, PH, PW):
    """The head as the network computes it, in float64: BN + ReLU, 7 x 7 average windows, NCHW flatten, Dense -> (B, classes)"""
    m = np.asarray(m, np.float64)
    b, _, _, c = m.shape
    a = np.maximum(m * np.asarray(scale, np.float64) + np.asarray(shift, np.float64), 0.0)
    pooled = a[:, :7 * PH, :7 * PW, :].reshape(b, PH, 7, PW, 7, c).mean(axis=(2, 4))                   # (B,PH,PW,C)
    feat = pooled.transpose(0, 3, 1, 2).reshape(b, -1)
    return feat @ np.asarray(wd, np.float64).T + np.asarray(bias, np.float64)


def oracle_head_input(params32, frames_u8):
    """What the fp32 oracle (oracle/torch_ref.py, CPU) averages in its head for these NHWC uint8 frames: relu(bn(stage4)) as NHWC
    float32 (B, H, W, 1024), and its features (B, F).  The oracle has no tap of its own: the input of its AvgPool2D(7) is recorded
    while it runs."""
    import torch
    from unittest import mock
    import oracle.torch_ref as TR
    from tennis_amd import weights as W
    seen = []
    pool = TR.F.avg_pool2d

    def recording(x, k, *a, **kw):
        if k == 7:
            seen.append(x.detach().clone())
        return pool(x, k, *a, **kw)

    net = TR.TorchDenseNet121(params32)
    with mock.patch.object(TR.F, "avg_pool2d", recording):
        feat = net(torch.from_numpy(W.normalize_to_nchw_f32(frames_u8))).numpy()
    assert len(seen) == 1
    return np.ascontiguousarray(seen[0].numpy().transpose(0, 2, 3, 1)), feat


def oracle_cam(params32, frames_u8, wd, PH, PW):
    """The maps of the fp32 oracle's own activations, in float64 -> (cam (B, classes, 7 PH, 7 PW), features (B, F))"""
    a, feat = oracle_head_input(params32, frames_u8)
    c = a.shape[-1]
    return cam_f64(a, np.ones(c), np.zeros(c), wd, PH, PW), feat


def synthetic_case(seed, B, H, W, C, PH, PW, classes):
    """A map with both signs around the ReLU threshold, some channels with scale = 0, and large values planted where no cell is.
    -> dict(m float32 (B,H,W,C), scale, shift (C) float32, wd (classes, C*PH*PW) float32, bias (classes) float32)"""
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 1.5, (B, H, W, C)).astype(np.float32)
    m[:, 7 * PH:] = 1000.0
    m[:, :, 7 * PW:] = 1000.0
    scale = (rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.4, -1.0, 1.0)).astype(np.float32)
    scale[rng.random(C) < 0.15] = 0.0
    scale[0] = 0.0
    shift = rng.normal(0, 0.3, C).astype(np.float32)
    wd = rng.normal(0, 0.5, (classes, C * PH * PW)).astype(np.float32)
    bias = rng.normal(0, 0.5, classes).astype(np.float32)
    return dict(m=m, scale=scale, shift=shift, wd=wd, bias=bias)
