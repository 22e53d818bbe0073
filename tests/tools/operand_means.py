"""(test infrastructure)  fp64 oracle of the encoder's calibration statistics (``tn_densenet121_input_means``).

The reference graph (DenseNet-121 ``.features``, as oracle/torch_ref.py states it) evaluated in float64 on the CPU, on exactly the
parameters the encoder is given, and for each of the 119 convolutions behind the stem the per-frame mean over all pixels of the
operand that convolution's folded weights multiply, in the units include/tennis_hip.h defines:
  * a dense layer's 1x1: ``clamp(x, lo, hi)`` with ``(lo, hi)`` from ``weights.bn_relu_clamp_fold(params, bn)``;
  * its 3x3: ``relu(bn2(bottleneck))``;
  * a transition: ``relu(bn(x))`` over all pixels of the block's map, before the 2x2 average (an odd map's last row / column
    counts).
Keys are the conv weight names ``engine.DenseNet121Features.input_means`` returns."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tennis_amd import weights as W

_MEAN = np.array([0.485, 0.456, 0.406])
_STD = np.array([0.229, 0.224, 0.225])


def normalize_f64(frames_u8: np.ndarray) -> torch.Tensor:
    """NHWC uint8 frames -> the reference's ToTensor + Normalize in float64, NCHW"""
    x = (np.asarray(frames_u8, np.float64) / 255.0 - _MEAN) / _STD
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


@torch.no_grad()
def operand_means(params: dict, frames_u8: np.ndarray, prefix: str = "densenet0_", relu_means: dict | None = None) -> dict:
    """``{conv weight name: (n_frames, cin) float64}``: per frame, the mean operand of every convolution behind the stem.
    ``relu_means``, if given, receives for every dense 1x1 the per-frame mean of ``relu(bn(x))`` from the same graph (the quantity
    ``sw * clamp-mean + tc`` stands for)."""
    p = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in params.items() if k.startswith(prefix)}

    def bn(x, name):
        n = prefix + name
        scale = p[n + "_gamma"] / torch.sqrt(p[n + "_running_var"] + W.BN_EPS)
        shift = p[n + "_beta"] - p[n + "_running_mean"] * scale
        return x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

    def frame_mean(a):
        return a.mean((2, 3)).numpy()

    out = {}
    x = F.conv2d(normalize_f64(frames_u8), p[prefix + "conv0_weight"], stride=2, padding=3)
    x = F.max_pool2d(F.relu(bn(x, "batchnorm0")), 3, 2, 1)
    outer = 1
    for st, nl in enumerate(W.BLOCK_CONFIG, 1):
        for li in range(nl):
            b1, b2 = f"stage{st}_batchnorm{2 * li}", f"stage{st}_batchnorm{2 * li + 1}"
            c1, c3 = f"{prefix}stage{st}_conv{2 * li}_weight", f"{prefix}stage{st}_conv{2 * li + 1}_weight"
            lo, hi, _, _ = W.bn_relu_clamp_fold(params, prefix + b1)
            lo = torch.from_numpy(lo.astype(np.float64)).view(1, -1, 1, 1)
            hi = torch.from_numpy(hi.astype(np.float64)).view(1, -1, 1, 1)
            out[c1] = frame_mean(torch.minimum(torch.maximum(x, lo), hi))
            a = F.relu(bn(x, b1))
            if relu_means is not None:
                relu_means[c1] = frame_mean(a)
            a = F.relu(bn(F.conv2d(a, p[c1]), b2))
            out[c3] = frame_mean(a)
            x = torch.cat([x, F.conv2d(a, p[c3], padding=1)], 1)
        if st != len(W.BLOCK_CONFIG):
            a = F.relu(bn(x, f"batchnorm{outer}"))
            out[f"{prefix}conv{outer}_weight"] = frame_mean(a)
            x = F.avg_pool2d(F.conv2d(a, p[f"{prefix}conv{outer}_weight"]), 2, 2)
            outer += 1
    return out


CENTRED = (3, 17, 40, 58)      # stem channels given a large mean in every consumer (the library's stem centre m_c becomes 1.0)
M_C = 1.0


def with_degenerate_channels(params: dict, prefix: str = "densenet0_") -> dict:
    """Parameter set (b) of tests/test_gpu_calibration_stats.py: a copy of ``params`` in which the stem channels ``CENTRED`` have
    running_mean ``M_C`` in every block-1 consumer (six dense layers' BN1 and the first transition's BatchNorm), and in the consumer
    of dense layer 2 those channels' clamps are degenerate or reversed: channel 3 gamma 0 (a constant), channel 17 a positive scale
    whose threshold lies past +65504 and channel 58 a negative one past -65504 (both always clipped), channel 40 a negative gamma.
    One channel of block 2 takes a negative gamma as well.  Only BatchNorm parameters change: the conv weights stay fp16 numbers
    once folded (a sign flip keeps them so, a degenerate channel's weights are never rounded)."""
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in params.items()}
    ch = list(CENTRED)
    for bn in [f"stage1_batchnorm{2 * l}" for l in range(W.BLOCK_CONFIG[0])] + ["batchnorm1"]:
        q[prefix + bn + "_running_mean"][ch] = M_C
    bn = prefix + "stage1_batchnorm4"
    q[bn + "_gamma"][3] = 0.0
    q[bn + "_gamma"][17], q[bn + "_beta"][17] = 1e-3, -100.0
    q[bn + "_gamma"][58], q[bn + "_beta"][58] = -1e-3, -100.0
    q[bn + "_gamma"][40] *= -1.0
    q[prefix + "stage2_batchnorm0_gamma"][5] *= -1.0
    return q
