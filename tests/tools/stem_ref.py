"""Float64 reference of the stem (conv 7x7/2 + BatchNorm + ReLU + MaxPool 3x3/2, csrc/stem_pool.hip, csrc/stem.hip + maxpool_kernel)
and an integer-exact restatement of its dithered rounding - numpy / torch-CPU only.

``stem_exact`` is the operator on the operands as the library DEFINES them (csrc/common.h "the stem's operand"), not as it computes
them: conv0's weights as the fp16 numbers ``fp16(w * stem_wfactor)`` (or hi + lo), the input as it is staged (``x - 255 mean_c`` of
a uint8 frame - the integer ``x - q_c`` plus the constant the library keeps in the BatchNorm shift -, ``fp16(v * 255 std_c)`` of a
normalised one), out-of-frame taps equal to the normalised zero, and everything behind that - sum, BatchNorm from its raw
parameters, max pool with -inf padding, ReLU, minus m_c - in float64.  Nothing of the library's folding (bias constant of the integer
staging, floor of the centred output, fragment order) is restated here: a wrong constant there shows as a difference.

``dither_emulate`` restates ``dither_pack`` and its key bit for bit.

The tests' cases (``STEM_CASES``), parameters (``stem_params``) and frames (``stem_frames``) live here as well: the CPU test of the
exclusion share and the GPU tests have to see the same inputs."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

LAYOUT_NCHW_F32, LAYOUT_NHWC_F16, LAYOUT_NHWC_U8 = 0, 1, 2
MEAN = np.array([0.485, 0.456, 0.406], np.float64)
STD = np.array([0.229, 0.224, 0.225], np.float64)
WSCALE = 64.0                                                # kStemWScale
WFACTOR32 = (WSCALE / (255.0 * STD)).astype(np.float32)      # stem_wfactor
UNSCALE32 = (255.0 * STD).astype(np.float32)                 # stem_unscale
BN_EPS = np.float64(np.float32(1e-5))


# ---- the operands -------------------------------------------------------------------------------------------------------------
def stem_weights(w0: np.ndarray, exact: bool) -> np.ndarray:
    """(64,3,7,7) fp32 -> the numbers the matrix pipe multiplies, float64: fp16(w * wfactor_c), or hi + lo with lo = fp16(w' - hi)"""
    ws = (w0.astype(np.float32) * WFACTOR32.reshape(1, 3, 1, 1)).astype(np.float32)
    hi = ws.astype(np.float16)
    if not exact:
        return hi.astype(np.float64)
    lo = (ws - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64)


def stem_operand(x: np.ndarray, layout: int) -> np.ndarray:
    """the input in `layout` -> (B,3,H,W) float64 of x - 255 mean_c as staged (0 = the normalised zero)"""
    if layout == LAYOUT_NHWC_U8:
        assert x.dtype == np.uint8 and x.shape[-1] == 3
        return np.ascontiguousarray((x.astype(np.float64) - 255.0 * MEAN).transpose(0, 3, 1, 2))
    if layout == LAYOUT_NHWC_F16:
        assert x.dtype == np.float16 and x.shape[-1] == 3
        v = (x.astype(np.float32) * UNSCALE32).astype(np.float32).astype(np.float16)
        return np.ascontiguousarray(v.astype(np.float64).transpose(0, 3, 1, 2))
    assert layout == LAYOUT_NCHW_F32 and x.dtype == np.float32 and x.shape[1] == 3
    return (x * UNSCALE32.reshape(1, 3, 1, 1)).astype(np.float32).astype(np.float16).astype(np.float64)


def stem_exact(w0, gamma, beta, mean, var, m_c, exact, layout, x):
    """-> (ref, A, pre), each (B,Hp,Wp,64) float64: the stored map relu(maxpool(bn(conv))) - m_c; the magnitude
    A = |s| sum |w| |x| of the output's largest window member (what the accumulation slack is proportional to); and the pooled
    value in front of the ReLU, pre (ref = max(pre, 0) - m_c)."""
    w = torch.from_numpy(stem_weights(np.asarray(w0), bool(exact)))
    op = torch.from_numpy(stem_operand(x, layout))
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + BN_EPS)
    t = np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * s
    s = s / WSCALE
    conv = F.conv2d(op, w, stride=2, padding=3)                                        # zero padding of x - 255 mean_c
    mag = F.conv2d(op.abs(), w.abs(), stride=2, padding=3) * torch.from_numpy(np.abs(s)).reshape(1, 64, 1, 1)
    y = conv * torch.from_numpy(s).reshape(1, 64, 1, 1) + torch.from_numpy(t).reshape(1, 64, 1, 1)
    pre = F.max_pool2d(y, 3, 2, padding=1)                                             # pads with -inf
    A = F.max_pool2d(mag, 3, 2, padding=1)
    pre = pre.permute(0, 2, 3, 1).contiguous().numpy()
    A = A.permute(0, 2, 3, 1).contiguous().numpy()
    return finish(pre, m_c), A, pre


def finish(pre, m_c):
    """ReLU and centring of a pooled value"""
    r = np.maximum(pre, 0.0)
    return r if m_c is None else r - np.asarray(m_c, np.float64)


def maxpool_ref(x: np.ndarray) -> np.ndarray:
    """(B,H,W,C) -> MaxPool2D(3, 2, pad 1) with -inf padding, float64"""
    t = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64).transpose(0, 3, 1, 2)))
    return F.max_pool2d(t, 3, 2, padding=1).permute(0, 2, 3, 1).contiguous().numpy()


# ---- tolerances (derived: docs/numerics.md "The stem and head kernels on their own") ----------------------------------------------
def slack(A):
    """fp32 accumulation of 147 products plus the BatchNorm fma: 160 * 2^-24 * A"""
    return 160.0 * 2.0 ** -24 * A


def ulp16(v):
    """spacing of fp16 at |v| (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


# ---- the dither -----------------------------------------------------------------------------------------------------------------
def dither_field(row, col, channel):
    """the 13-bit number dither_pack adds below the fp16 mantissa at (pooled row, pooled column, channel): a multiplicative hash of
    (row, column, channel >> 3), two bits further on per channel of the group"""
    row, col, channel = (np.asarray(a).astype(np.uint64) for a in (row, col, channel))
    M = np.uint64(0xFFFFFFFF)
    h = (row * np.uint64(0x85EBCA77) + col * np.uint64(0x9E3779B1) + (channel >> np.uint64(3)) * np.uint64(0xC2B2AE3D)) & M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & M
    h ^= h >> np.uint64(12)
    return ((h >> (np.uint64(2) * (channel & np.uint64(7)))) & np.uint64(0x1FFF)).astype(np.uint32)


def f32_to_f16_rtz(bits: np.ndarray) -> np.ndarray:
    """fp32 bit patterns -> fp16 bit patterns, rounded towards zero (v_cvt_pkrtz_f16_f32; finite inputs, fp16 subnormals kept)"""
    bits = bits.astype(np.uint32)
    sign = ((bits >> np.uint32(16)) & np.uint32(0x8000)).astype(np.uint32)
    e = ((bits >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    man = (bits & np.uint32(0x7FFFFF)).astype(np.int64)
    normal = ((e - 112) << 10) | (man >> 13)
    sh = np.clip(126 - e, 14, 40)                                   # subnormal half: the implicit one shifted in
    sub = (man | 0x800000) >> sh
    out = np.where(e >= 113, normal, np.where(e == 0, 0, sub))
    out = np.where(e > 142, 0x7BFF, out)                            # past the fp16 range: the largest finite half
    return (sign | out.astype(np.uint32)).astype(np.uint16)


def dither_emulate(v32, row, col, channel) -> np.ndarray:
    """float32 values at (pooled row, pooled column, channel) (broadcast against each other) -> the float16 dither_pack stores: the
    13-bit field added to the fp32 BIT PATTERN (towards larger magnitude), the sum truncated to fp16"""
    v32 = np.asarray(v32, np.float32)
    bits = v32.view(np.uint32) + dither_field(row, col, channel)
    return f32_to_f16_rtz(np.broadcast_to(bits, np.broadcast(v32, row, col, channel).shape)).view(np.float16)


def grid(shape):
    """(row, col, channel) index arrays broadcastable to a (B,Hp,Wp,C) map"""
    _, hp, wp, c = shape
    return np.arange(hp).reshape(1, hp, 1, 1), np.arange(wp).reshape(1, 1, wp, 1), np.arange(c).reshape(1, 1, 1, c)


def emulate_map(pre, m_c, delta=0.0):
    """the emulated stored map of a pooled pre-ReLU value moved by `delta` (the accumulation error sits in front of the ReLU: an output
    the ReLU holds at its floor with room to spare is exact)"""
    v = finish(pre + delta, m_c).astype(np.float32)
    return dither_emulate(v, *grid(v.shape))


def decided(pre, A, m_c):
    """-> (emulated map, mask of the outputs whose emulated half does not change when the value moves by +- its slack)"""
    sl = slack(A)
    lo, mid, hi = emulate_map(pre, m_c, -sl), emulate_map(pre, m_c), emulate_map(pre, m_c, sl)
    return mid, (lo == mid) & (hi == mid)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# (name, H, W, layout, exact, fused).  The fused kernel has 12 instantiations, layout x fetch path (vector: W % 8 == 0 and W >= 80)
# x weights; each appears at an interior-heavy size (>= 224: most tiles take the unmasked conv) and a border-heavy one (64 / 80 /
# 120 x 200: every tile, or most, is a border tile).  226 / 236 / 64: element path; 224 / 232 / 512 / 80 / 120 x 200: vector path.
_L = {"u8": LAYOUT_NHWC_U8, "f16": LAYOUT_NHWC_F16, "f32": LAYOUT_NCHW_F32}
STEM_CASES = []
for _lay in ("u8", "f16", "f32"):
    for _ex in (False, True):
        for _h, _w in {"u8": ((224, 224), (80, 80), (226, 226), (64, 64)), "f16": ((232, 232), (80, 80), (236, 236), (64, 64)),
                       "f32": ((224, 224), (80, 80), (226, 226), (64, 64))}[_lay]:
            STEM_CASES.append((f"fused_{_lay}_{'exact' if _ex else 'rounded'}_{_h}x{_w}", _h, _w, _L[_lay], _ex, True))
STEM_CASES += [
    ("fused_u8_rounded_120x200", 120, 200, _L["u8"], False, True),          # non-square: H and W are separate
    ("fused_f16_rounded_232x224", 232, 224, _L["f16"], False, True),
    ("fused_f32_exact_120x200", 120, 200, _L["f32"], True, True),
    ("fused_u8_rounded_512x512", 512, 512, _L["u8"], False, True),
    ("fused_u8_rounded_236x236", 236, 236, _L["u8"], False, True),
    ("fused_f32_rounded_232x232", 232, 232, _L["f32"], False, True),
    ("unfused_u8_224x224", 224, 224, _L["u8"], False, False),
    ("unfused_u8_64x64", 64, 64, _L["u8"], False, False),
    ("unfused_f16_226x226", 226, 226, _L["f16"], False, False),
    ("unfused_f32_80x80", 80, 80, _L["f32"], False, False),
    ("unfused_f16_120x200", 120, 200, _L["f16"], False, False),
]
UNCENTRED = {"fused_u8_rounded_226x226", "fused_f16_exact_80x80", "fused_f32_rounded_224x224", "fused_u8_exact_64x64",
             "fused_f16_rounded_236x236", "unfused_f16_226x226"}              # m_c = null


def stem_params(name: str):
    """seeded conv0 weights and batchnorm0 parameters of a case (not the model's) -> dict(w0, gamma, beta, mean, var, m_c).

    Both signs of gamma; channels 3, 19, 40, 7, 28, 55 with gamma = +-1e-4; running_var 1e-5 in those and in channel 12, 50 in
    channels 5, 33; m_c of both signs up to |m_c| = 4, or None (UNCENTRED).

    Two choices keep the share of outputs the +- slack rule leaves undecided under its 5 % cap (test_cpu_stem_ref): the weights are
    small against the BatchNorm shift (sigma 0.003: A ~ 0.5 |gamma| / sqrt(var) against outputs of order 1, and still a signal of some
    hundred fp16 ulps), and the channels with gamma = +-1e-4 get running_var = 1e-5, weights 27 times as large and |beta|, |mean|,
    |m_c| <= 0.9.  The second is about what the slack does NOT contain: the library's folded shift (t, t - m_c, and for uint8 input t plus
    the constant of the integer staging) is an fp32 number, up to 3 * 2^-24 max(|t|, |t - m_c|) from the float64 one, while the slack
    is proportional to A.  With gamma = 1e-4, a variance of order one and the common weights A is 1e-4 on a frame of 128s, and the
    rounded shift alone moves a few outputs per case across a dither threshold (seen on the device: two of 1 M).  As chosen, A is 0.035
    or more on every frame, and 160 * 2^-24 * A = 3.4e-7 covers 3 * 2^-24 * 1.84 = 3.3e-7; the channel is still the near-constant
    relu(beta) - m_c (signal 0.05) the centring exists for."""
    rng = np.random.default_rng(hash_name(name))
    w0 = rng.normal(0, 0.003, (64, 3, 7, 7)).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, 64) * np.where(rng.random(64) < 0.3, -1.0, 1.0)).astype(np.float32)
    beta = rng.normal(0.6, 0.5, 64).astype(np.float32)
    mean = rng.normal(0, 0.3, 64).astype(np.float32)
    var = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    m_c = (rng.uniform(0.05, 4.0, 64) * np.where(rng.random(64) < 0.5, -1.0, 1.0)).astype(np.float32)
    m_c[[10, 20]] = [4.0, -4.0]
    var[12] = 1e-5
    var[[5, 33]] = 50.0
    for i, c in enumerate((3, 19, 40, 7, 28, 55)):
        gamma[c] = 1e-4 if i % 2 == 0 else -1e-4
        var[c] = 1e-5
        w0[c] *= 27.0
        beta[c] = np.clip(beta[c], -0.9, 0.9); mean[c] = np.clip(mean[c], -0.9, 0.9); m_c[c] = np.clip(m_c[c], -0.9, 0.9)
    return dict(w0=w0, gamma=gamma, beta=beta, mean=mean, var=var, m_c=None if name in UNCENTRED else m_c)


def hash_name(name: str) -> int:
    import zlib
    return zlib.crc32(name.encode())


def stem_frames(h: int, w: int, seed: int = 5) -> np.ndarray:
    """(5,h,w,3) uint8: uniform noise; constant 0; constant 255; 128 inside a one-pixel ring of 0 (top, bottom) and 255 (left, right);
    single-pixel impulses at the four corners, the four edge midpoints and the centre of a frame of 128"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    f = np.empty((5, h, w, 3), np.uint8)
    f[0] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    f[1] = 0
    f[2] = 255
    f[3] = 128
    f[3, 0] = 0; f[3, -1] = 0; f[3, :, 0] = 255; f[3, :, -1] = 255
    f[4] = 128
    for k, (iy, ix) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1),
                                  (h // 2, w // 2))):
        f[4, iy, ix] = ((255, 0, 255), (0, 255, 0), (255, 255, 0))[k % 3]
    return f


CONSTANT_FRAMES = (1, 2)      # of stem_frames


def layout_input(u8: np.ndarray, layout: int) -> np.ndarray:
    """the frames as the kernel is handed them in `layout`: uint8 NHWC, or ToTensor + Normalize as fp16 NHWC / fp32 NCHW"""
    if layout == LAYOUT_NHWC_U8:
        return np.ascontiguousarray(u8)
    v = ((u8.astype(np.float32) / np.float32(255.0)) - MEAN.astype(np.float32)) / STD.astype(np.float32)
    if layout == LAYOUT_NHWC_F16:
        return np.ascontiguousarray(v.astype(np.float16))
    return np.ascontiguousarray(v.astype(np.float32).transpose(0, 3, 1, 2))


def case_reference(case):
    """-> (params, input in the case's layout, ref, A, pre) of one of STEM_CASES"""
    name, h, w, layout, exact, fused = case
    p = stem_params(name)
    x = layout_input(stem_frames(h, w), layout)
    ref, A, pre = stem_exact(p["w0"], p["gamma"], p["beta"], p["mean"], p["var"], p["m_c"], exact, layout, x)
    return p, x, ref, A, pre
