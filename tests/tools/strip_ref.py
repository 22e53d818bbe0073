"""Float64 reference of the strip-streaming fused dense layer (csrc/dense_strip_impl.h, dense_strip_body.h), the componentwise
bound the device is held to, an fp32 model of the kernel's arithmetic and the two input generators - numpy only.

``reference`` is the layer on the operands as the library DEFINES them (docs/kernels.md "strip-streaming form",
csrc/dense_strip.hip::pack_w1_strip), everything in float64 unless stated:

    a1    = clip(x, lo, hi)                                  exact: no arithmetic
    w1h   = float16(float32(w1) * float32(s2))               the packer's own rounding
    t_eff = float16(t2) + float16(t2 - float16(t2))          the two halves of the shift k-step
    bott  = a1 @ w1h.T + t_eff
    a2    = relu(bott)
    y     = conv3x3(a2, w3), zero padding behind the activation; w3 holds fp16 numbers

The device rounds a2 and y to fp16 once each; the reference rounds neither.  Nothing of the kernel's layout (fragment order, strip
pairs, row chunks, window registers) is restated: a product that is dropped, doubled or taken from the wrong place is a difference.

``bound`` is derived, not measured.  u = 2^-11 (half an fp16 ulp, relative), e = 2^-24 (fp32's unit roundoff):

    db(p, c) = (K + 17) e (sum_k |a1| |w1h| + |t_eff|)
               fp32 accumulation of exact fp16 products: K products and the three of the shift k-step (shift_hi, shift_lo, mask), held
               by K / 16 + 1 chained MFMAs; (n - 1) e sum |terms| bounds any summation order of n terms, and K + 17 leaves 15 terms of
               room, which also covers |shift_hi| + |shift_lo| <= (1 + 2^-10) |t_eff|
    da(p, c) = u (a2 + db) + db + 2^-25
               ReLU is 1-Lipschitz, one rounding to fp16 of a value of at most a2 + db; 2^-25 is half an fp16 subnormal step
    E(p, o)  = u |y| + (1 + u) [sum_{tap, c} |w3| da + (1152 + 3) e sum |w3| (a2 + da)] + 2^-25
               the operand's error through the sum, the fp32 accumulation of 1152 products in three column accumulators that are
               added last, one rounding to fp16 of the sum (u times the sum's own error is the (1 + u))

The test statistic is max |y_dev - y| / E, which has to be <= 1.

Outside the bound's reach (listed, not worked around): the low half of the shift dropped (|shift_lo| <= 2^-11 |t2| is below u a2
wherever the ReLU passes the value); a rounding of a2 or y other than to nearest that stays within u; which of the two lanes'
halves of a 128-byte line a super-step reads when both hold the same numbers.

``model`` is an fp32 restatement of the kernel's arithmetic - accumulation k-step by k-step in float32, the two fp16 roundings, the
three column accumulators summed last - with one defect at a time switched on (tests/test_cpu_strip_ref.py: the model stays inside
the bound, every defect leaves it)."""
from __future__ import annotations

import numpy as np

U16 = 2.0 ** -11
E32 = 2.0 ** -24
F16_MAX = np.float32(65504.0)

# dense_strip_supported: W in {56, 28, 64} x K = 64 ... 320 and W = 128 x K = 64 ... 288
SUPPORTED = [(w, k) for w in (56, 28, 64, 128) for k in range(64, (288 if w == 128 else 320) + 1, 32)]
assert len(SUPPORTED) == 35


def rows_per_wave(w: int) -> int:
    """DSGeom::ROWS: output rows of one wave's chunk"""
    return 28 if w == 56 else 7 if w == 28 else w // 4


def smallest_ldc(k: int) -> int:
    """the next multiple of 64 >= K + 32"""
    return (k + 32 + 63) // 64 * 64


def case_ldc(k: int) -> int:
    """the row pitch the GPU tests use: the smallest legal one for odd K / 32 (the output fills the line's other half), one line more
    otherwise"""
    return smallest_ldc(k) + (0 if (k // 32) % 2 else 64)


# ---- the operands ---------------------------------------------------------------------------------------------------------------
def folded_weights(w1, s2) -> np.ndarray:
    """(128,K) fp32, (128,) fp32 -> float16(float32(w1) * float32(s2)) as float64"""
    return (np.asarray(w1, np.float32) * np.asarray(s2, np.float32)[:, None]).astype(np.float32).astype(np.float16).astype(np.float64)


def shift_halves(t2):
    """(128,) fp32 -> (shift_hi, shift_lo) as float64: fp16(t), fp16(t - fp16(t)) with the difference taken in float32"""
    t = np.asarray(t2, np.float32)
    hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _conv3x3(a, w):
    """(B,H,W,C) x (O,C,3,3) -> (B,H,W,O), zero padding, in the arrays' own precision"""
    b, h, wd, c = a.shape
    p = np.zeros((b, h + 2, wd + 2, c), a.dtype)
    p[:, 1:-1, 1:-1] = a
    y = np.zeros((b, h, wd, w.shape[0]), a.dtype)
    for dy in range(3):
        for dx in range(3):
            y += p[:, dy:dy + h, dx:dx + wd] @ w[:, :, dy, dx].T
    return y


def reference(inp):
    """inputs of one case (``noisy`` / ``integer``) -> (y, E): the float64 layer output (B,W,W,32) and its componentwise bound"""
    x = inp["x"].astype(np.float64)
    k = x.shape[-1]
    a1 = np.clip(x, inp["lo"].astype(np.float64), inp["hi"].astype(np.float64))
    w1h = folded_weights(inp["w1"], inp["s2"])
    hi, lo = shift_halves(inp["t2"])
    t_eff = hi + lo
    bott = a1 @ w1h.T + t_eff
    mag = np.abs(a1) @ np.abs(w1h).T + np.abs(t_eff)
    a2 = np.maximum(bott, 0.0)
    w3 = inp["w3"].astype(np.float64)
    y = _conv3x3(a2, w3)
    db = (k + 17) * E32 * mag
    da = U16 * (a2 + db) + db + 2.0 ** -25
    through = _conv3x3(da + (1152 + 3) * E32 * (a2 + da), np.abs(w3))
    bound = U16 * np.abs(y) + (1.0 + U16) * through + 2.0 ** -25
    return y, bound


def ratio(got, y, bound) -> float:
    """max |got - y| / E"""
    return float((np.abs(np.asarray(got, np.float64) - y) / bound).max())


# ---- the fp32 model of the kernel's arithmetic ---------------------------------------------------------------------------------
def _h(v):
    return v.astype(np.float16).astype(np.float32)


def model(inp, drop_tap=None, drop_k=None, seam_row=None, pad_col=False):
    """-> (B,W,W,32) float32 holding fp16 numbers: what a kernel that does the defined arithmetic in the kernel's precision stores.

    One defect at a time:
      drop_tap = (o, c, dy, dx)  that product is missing from output channel o
      drop_k = k                 input channel k of the 1x1 is missing
      seam_row = r               the 3x3 of chunk row r sees, as the bottleneck row above it, row r instead of row r - 1 (the halo row
                                 above a chunk seam taken from below it)
      pad_col = True             the padding column left of the frame holds column 0's bottleneck instead of zeros (the mask of the
                                 shift k-step missing in that lane)"""
    x = inp["x"].astype(np.float32)
    b, h, w, k = x.shape
    a1 = np.clip(x, inp["lo"], inp["hi"]).astype(np.float32)
    w1h = folded_weights(inp["w1"], inp["s2"]).astype(np.float32)
    if drop_k is not None:
        w1h = w1h.copy()
        w1h[:, drop_k] = 0.0
    hi, lo = (v.astype(np.float32) for v in shift_halves(inp["t2"]))
    acc = np.zeros((b, h, w, 128), np.float32)
    for q in range(k // 16):                                   # one 16-channel k-step per MFMA
        acc += a1[..., 16 * q:16 * q + 16] @ w1h[:, 16 * q:16 * q + 16].T
    acc += (hi + lo).astype(np.float32)                        # the shift k-step
    a2 = _h(np.maximum(acc, np.float32(0.0)))
    w3 = inp["w3"].astype(np.float32)
    if drop_tap is not None:
        o, c, dy, dx = drop_tap
        w3 = w3.copy()
        w3[o, c, dy, dx] = 0.0
    p = np.zeros((b, h + 2, w + 2, 128), np.float32)
    p[:, 1:-1, 1:-1] = a2
    if pad_col:
        p[:, 1:-1, 0] = a2[:, :, 0]
    cols = []
    for dx in range(3):                                        # one accumulator per kernel column
        c3 = np.zeros((b, h, w, 32), np.float32)
        for dy in range(3):
            rows = p[:, dy:dy + h, dx:dx + w]
            if seam_row is not None and dy == 0:
                rows = rows.copy()
                rows[:, seam_row] = p[:, seam_row + 1, dx:dx + w]      # bottleneck row seam_row itself
            for t in range(8):
                c3 += rows[..., 16 * t:16 * t + 16] @ w3[:, 16 * t:16 * t + 16, dy, dx].T
        cols.append(c3)
    return _h((cols[1] + cols[0]) + cols[2])


# ---- the inputs -----------------------------------------------------------------------------------------------------------------
def clamp_consts(rng, k):
    """(lo, hi) of BN1 + ReLU in the kernels' form (csrc/calib_host.hip::bn_relu_clamp_fold), the distribution of
    tests/test_gpu_kernels.py::_clamp_consts: positive scales (lo = threshold, hi = 65504), negative ones (lo = -65504, hi =
    threshold) and constant channels (lo = hi = 0)"""
    thr = rng.normal(0, 0.6, k).astype(np.float16).astype(np.float32)
    kind = rng.random(k)
    lo = np.where(kind < 0.82, thr, -F16_MAX).astype(np.float32)
    hi = np.where(kind < 0.82, F16_MAX, thr).astype(np.float32)
    lo[kind > 0.97] = 0.0
    hi[kind > 0.97] = 0.0
    return lo, hi


def seam_lines(w: int):
    """-> (rows, columns) next to a place where the kernel changes owner: the frame borders; the strip seams (columns 13 | 14 and
    every 14 from there); the chunk seams between waves (every DSGeom::ROWS rows) - at W = 128 / 64 the workgroup seams are among
    these two -; the partly empty last strip pair of a width that is no multiple of 28 (columns 112 ... 127 / 56 ... 63)"""
    rows, cols = {0, w - 1}, {0, w - 1}
    for c in range(14, w, 14):
        cols |= {c - 1, c}
    r = rows_per_wave(w)
    for y in range(r, w, r):
        rows |= {y - 1, y}
    if w % 28:
        cols |= set(range(w // 28 * 28, w))
    return sorted(rows), sorted(cols)


def noisy(w: int, k: int, b: int, seed: int):
    """The distribution of tests/test_gpu_kernels.py::test_dense_strip (Gaussian activations, clamp constants of all three kinds,
    Gaussian weights) with |x| in [20, 60] of random sign planted, in every channel, on the rows and columns of ``seam_lines``: a halo
    row or column taken from the wrong neighbour, or a padding lane that is not zero, is an O(1) error there, not an average one.
    -> dict(x (B,W,W,K) fp16, lo, hi, w1 (128,K), s2, t2, w3 (32,128,3,3) fp16-valued; fp32)"""
    rng = np.random.default_rng([seed, w, k, b])
    x = rng.normal(0, 1.5, (b, w, w, k)).astype(np.float32)
    big = (rng.uniform(20.0, 60.0, x.shape) * np.where(rng.random(x.shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    rows, cols = seam_lines(w)
    m = np.zeros((w, w), bool)
    m[rows, :] = True
    m[:, cols] = True
    x[:, m] = big[:, m]
    lo, hi = clamp_consts(rng, k)
    return dict(x=x.astype(np.float16), lo=lo, hi=hi,
                w1=rng.normal(0, np.sqrt(2.0 / k), (128, k)).astype(np.float32),
                s2=rng.uniform(0.5, 1.5, 128).astype(np.float32), t2=rng.normal(0, 0.3, 128).astype(np.float32),
                w3=_h(rng.normal(0, np.sqrt(2.0 / 1152), (32, 128, 3, 3)).astype(np.float32)))


def integer(w: int, k: int, b: int, seed: int):
    """Every value exact at every rounding: x in {0, 1} behind a clamp that passes it (lo = 0, hi = 65504), s2 = 1, w1 in
    {-1, 0, 1} with exactly 16 non-zeros per row (a run of 16 channels starting at 11 n mod K: every input channel is hit by at least
    two rows), t2 an integer in [-8, 8] (|bott| <= 24), w3 in {-1, 0, 1} with position p = 128 tap + c non-zero in output channel
    p mod 32 alone (36 non-zeros per output: |y| <= 36 * 24 = 864 < 2048, an integer fp16 holds).  Same keys as ``noisy``."""
    rng = np.random.default_rng([seed, w, k, b, 1])
    x = rng.integers(0, 2, (b, w, w, k)).astype(np.float16)
    w1 = np.zeros((128, k), np.float32)
    for n in range(128):
        w1[n, (11 * n + np.arange(16)) % k] = rng.choice([-1.0, 1.0], 16)
    w3 = np.zeros((32, 128, 3, 3), np.float32)
    sign = rng.choice([-1.0, 1.0], (3, 3, 128))
    for dy in range(3):
        for dx in range(3):
            for c in range(128):
                w3[(128 * (3 * dy + dx) + c) % 32, c, dy, dx] = sign[dy, dx, c]
    return dict(x=x, lo=np.zeros(k, np.float32), hi=np.full(k, F16_MAX, np.float32), w1=w1, s2=np.ones(128, np.float32),
                t2=rng.integers(-8, 9, 128).astype(np.float32), w3=w3)


GENERATORS = {"noisy": noisy, "integer": integer}
