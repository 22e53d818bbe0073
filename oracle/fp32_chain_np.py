"""The fp32 encoder mode's convolution kernel (tennis_amd/csrc/dense_fp32.hip, conv_fp32_kernel) restated in exact fp32 steps -
numpy only.  Every step of the kernel is one order-defined fp32 operation: the uint8 normalisation on load, relu_bn (an fmaf), the
transition's ((v00 + v01) + (v10 + v11)) * 0.25f, the k-ascending multiply-add chain with one accumulator per output, the stem's
epilogue.  ``conv_fp32_chain`` computes what a correctly rounded fused chain gives, bit for bit, and beside it the float64 result and
sum |a||b| of tests/test_gpu_fp32x3_mode.py::_case, so both references of a test come from one place.

``fmaf32`` is the float32 fma without ``math.fma`` or long double: the float64 product of two float32 numbers is exact (48 bits), the
float64 sum p + c is rounded once, TwoSum gives that rounding's exact error, and rounding the float64 sum to float32 is then the
fma's rounding except where the float64 sum sits exactly on a float32 tie while the true sum does not: there the sign of the error
decides, not ties-to-even.  (Where the float64 sum is no tie, the true sum is on the same side of every float32 midpoint - midpoints
are float64 numbers and rounding is monotonic.)

A case is the dict of tests/test_gpu_fp32x3_mode.py::_case: kind, B, Ho, Wo, K, layout, x, ldx, H, W, w (K, N), N, s, t, es, et.
"""
import numpy as np

STEM, C1X1, C3X3, TRANS = 0, 1, 2, 3
F32_MIN_NORMAL = 2.0 ** -126
MEAN32 = np.array([0.485, 0.456, 0.406], np.float32)          # weights.IMAGENET_MEAN / _STD in float32
STD32 = np.array([0.229, 0.224, 0.225], np.float32)
_LOW29 = np.uint64(0x1FFFFFFF)
_HALF29 = np.uint64(0x10000000)


def _fma_parts(a, b, c):
    """(float32 result, float64 product, float64 sum) of a * b + c, all broadcast"""
    a64, b64, c64 = (np.atleast_1d(np.asarray(v, np.float32)).astype(np.float64) for v in (a, b, c))
    p = a64 * b64                                              # exact: 24 + 24 bits
    s = p + c64
    r = s.astype(np.float32)                                   # round to nearest even of the float64 sum
    # candidates for the repair: the float64 sum on a float32 tie (its low 29 mantissa bits are 1 0...0 in the normal range),
    # or in float32's subnormal range, where the tie sits elsewhere - both rare, handled one by one below
    bits = np.ascontiguousarray(s).view(np.uint64)
    cand = ((bits & _LOW29) == _HALF29) | ((np.abs(s) < F32_MIN_NORMAL) & (s != 0))
    if cand.any():
        p, c64 = np.broadcast_to(p, s.shape), np.broadcast_to(c64, s.shape)
        sc, pc, cc, rc = s[cand], p[cand], c64[cand], r[cand]
        bb = sc - pc
        err = (pc - (sc - bb)) + (cc - bb)                     # TwoSum: p + c = s + err exactly
        d = sc - rc.astype(np.float64)                         # exact
        with np.errstate(over="ignore"):
            other = np.nextafter(rc, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = (d != 0) & (np.abs(d) == np.abs(other.astype(np.float64) - sc))
        # the true sum s + err is past the midpoint, on the other neighbour's side, when err points the way d does
        flip = tie & (np.sign(err) == np.sign(d))
        rc = np.where(flip, other, rc)
        r = r.copy()
        r[cand] = rc
    return r, p, s


def fmaf32(a, b, c):
    """the correctly rounded float32 fma of float32 arrays (broadcast)"""
    r, _, _ = _fma_parts(a, b, c)
    return r.reshape(np.broadcast(a, b, c).shape)


def relu_bn(x, s, t):
    """the kernel's relu_bn: max(fmaf(x, s, t), 0)"""
    return np.maximum(fmaf32(x, s, t), np.float32(0))


def _act64(x, s, t):
    return np.maximum(x.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64), 0.0)


def stem_input_nchw(c):
    """the stem's input as the kernel's loader widens it: (B, 3, H, W) float32"""
    x, layout = c["x"], c["layout"]
    if layout == 2:                                            # NHWC uint8: (u / 255 - mean) / std, each step rounded once
        u = x.astype(np.float32)
        v = ((u / np.float32(255.0)) - MEAN32) / STD32
        assert v.dtype == np.float32
        return np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    if layout == 1:                                            # NHWC fp16, widened exactly
        return np.ascontiguousarray(x.astype(np.float32).transpose(0, 3, 1, 2))
    return np.ascontiguousarray(x, dtype=np.float32)


def operand_a(c, pad_before_activation=False, flat_average=False):
    """-> (A32 (M, K) float32 exactly as load_a forms it, A64 (M, K) float64 as _case forms it).  The two switches build the
    defects the CPU test shows the chain to separate: the 3x3's padding applied before the activation, the transition's average
    summed left to right."""
    kind, B, Ho, Wo, K = c["kind"], c["B"], c["Ho"], c["Wo"], c["K"]
    H, W = c["H"], c["W"]
    if kind == STEM:
        x32 = stem_input_nchw(c)
        xp = np.zeros((B, 3, H + 6, W + 6), np.float32)        # zeros outside the frame
        xp[:, :, 3:3 + H, 3:3 + W] = x32
        cols = [xp[:, ch, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] for ch in range(3) for ky in range(7) for kx in range(7)]
        a32 = np.stack(cols, axis=-1).reshape(-1, 147)         # k = c 49 + ky 7 + kx
        return a32, a32.astype(np.float64)
    x, s, t = c["x"], c["s"], c["t"]
    if kind == C1X1:
        a32 = relu_bn(x[..., :K], s, t).reshape(-1, K)
        return a32, _act64(x[..., :K], s, t).reshape(-1, K)
    if kind == C3X3:
        taps = [(ky, kx) for ky in range(3) for kx in range(3)]

        def im2col(act, dtype):
            ap = np.zeros((B, H + 2, W + 2, 128), dtype)
            if pad_before_activation:
                ap[:, 1:1 + H, 1:1 + W] = x
                ap = act(ap)
            else:
                ap[:, 1:1 + H, 1:1 + W] = act(x)               # zero padding AFTER the activation
            return np.concatenate([ap[:, ky:ky + H, kx:kx + W] for ky, kx in taps], axis=-1).reshape(-1, 1152)   # k = tap 128 + c
        return im2col(lambda v: relu_bn(v, s, t), np.float32), im2col(lambda v: _act64(v, s, t), np.float64)
    # transition: relu_bn of the four pixels, ((v00 + v01) + (v10 + v11)) * 0.25f; a last odd row / column is never read
    r = relu_bn(x[..., :K], s, t)
    v00, v01 = r[:, 0:2 * Ho:2, 0:2 * Wo:2], r[:, 0:2 * Ho:2, 1:2 * Wo:2]
    v10, v11 = r[:, 1:2 * Ho:2, 0:2 * Wo:2], r[:, 1:2 * Ho:2, 1:2 * Wo:2]
    if flat_average:
        a32 = (((v00 + v01) + v10) + v11) * np.float32(0.25)
    else:
        a32 = ((v00 + v01) + (v10 + v11)) * np.float32(0.25)
    assert a32.dtype == np.float32
    r64 = _act64(x[..., :K], s, t)
    a64 = 0.25 * (r64[:, 0:2 * Ho:2, 0:2 * Wo:2] + r64[:, 0:2 * Ho:2, 1:2 * Wo:2] + r64[:, 1:2 * Ho:2, 0:2 * Wo:2] + r64[:, 1:2 * Ho:2, 1:2 * Wo:2])
    return a32.reshape(-1, K), a64.reshape(-1, K)


def _subnormal(v):
    v = np.abs(v)
    return bool(((v != 0) & (v < F32_MIN_NORMAL)).any())


def chain(a32, w, order="fused"):
    """(M, K) x (K, N) float32 -> ((M, N) float32, subnormal flag).  order: "fused" - acc = fmaf32(A[:, k], W[k], acc), k ascending
    from 0, what the kernel claims; and the near misses a test must tell from it: "unfused" (the product rounded to float32 before
    the add), "descending" (k from K - 1 down), "pairs" (the two products of a k pair summed first, then added to the accumulator)."""
    a32, w = np.asarray(a32, np.float32), np.asarray(w, np.float32)
    K = a32.shape[1]
    acc = np.zeros((a32.shape[0], w.shape[1]), np.float32)
    sub = False
    ks = range(K - 1, -1, -1) if order == "descending" else range(K)
    if order in ("fused", "descending"):
        for k in ks:
            acc, p, _ = _fma_parts(a32[:, k, None], w[None, k, :], acc)
            sub = sub or _subnormal(p) or _subnormal(acc)
    elif order == "unfused":
        for k in ks:
            acc = acc + a32[:, k, None] * w[None, k, :]
    elif order == "pairs":
        if K % 2:                                              # (the stem's 147: the kernel's zero padding supplies the partner)
            a32, w = np.pad(a32, ((0, 0), (0, 1))), np.pad(w, ((0, 1), (0, 0)))
        for k in range(0, a32.shape[1], 2):
            pair = fmaf32(a32[:, k + 1, None], w[None, k + 1, :], a32[:, k, None] * w[None, k, :])
            acc = acc + pair
    else:
        raise ValueError(order)
    assert acc.dtype == np.float32
    return acc, sub


def float64_reference(c, a64):
    """-> (acc64, sab): the product and sum |a||b| in float64, as _case has them"""
    w64 = c["w"].astype(np.float64)
    if c["kind"] == STEM:                                      # _case's loop, tap by tap
        B, Ho, Wo, N = c["B"], c["Ho"], c["Wo"], c["N"]
        y = np.zeros((B, Ho, Wo, N))
        sab = np.zeros_like(y)
        a = a64.reshape(B, Ho, Wo, 147)
        for k in range(147):
            y += a[..., k, None] * w64[k]
            sab += np.abs(a[..., k])[..., None] * np.abs(w64[k])
        return y.reshape(-1, N), sab.reshape(-1, N)
    return a64 @ w64, np.abs(a64) @ np.abs(w64)


def float64_output(c, acc64, sab, rel):
    """-> (y64, bound): the launch's float64 result and the componentwise bound `rel` sum |a||b| - for the stem through the epilogue
    relu(fma(acc, es, et)): the product's bound times |es| plus the fma's one rounding (2^-24 relative)"""
    if c["es"] is None:
        return acc64, rel * sab
    es64, et64 = c["es"].astype(np.float64), c["et"].astype(np.float64)
    pre = acc64 * es64 + et64
    return np.maximum(pre, 0.0), rel * sab * np.abs(es64) + 2.0 ** -24 * np.abs(pre)


def conv_fp32_chain(c):
    """-> dict(y: the kernel's output (M, N) float32 if it is the fused k-ascending chain, acc64 / sab: the float64 product and
    sum |a||b|, subnormal: whether a product, a partial sum or an operand of the chain is a nonzero float32 subnormal)"""
    a32, a64 = operand_a(c)
    acc, sub = chain(a32, c["w"])
    sub = sub or _subnormal(a32) or _subnormal(c["w"])
    if c["es"] is not None:
        acc, p, _ = _fma_parts(acc, c["es"], c["et"])
        sub = sub or _subnormal(p) or _subnormal(acc)
        acc = np.maximum(acc, np.float32(0))
    acc64, sab = float64_reference(c, a64)
    return dict(y=acc, acc64=acc64, sab=sab, subnormal=sub)


# ---- operands: the recipe of tests/test_gpu_fp32x3_mode.py, with the output channels and the input extents free ---------------------
def _bn(rng, n):
    s = (3.0 * rng.uniform(0.8, 1.2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    t = (0.5 * rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return s, t


def make_case(kind, B, Ho, Wo, K, N, rng, layout=0, H=None, W=None):
    """x ~ N(0, 1), |s| ~ 3, |t| ~ 0.5 with both signs, w = 0.05 N(0, 1).  1x1 / transition: the activation buffer has ldx = K + 32
    channels and those past K are NaN.  Stem: H = 2 Ho, W = 2 Wo - 1 unless given (one even and one odd extent)."""
    c = dict(kind=kind, B=B, Ho=Ho, Wo=Wo, K=K, N=N, layout=layout, es=None, et=None, s=None, t=None)
    if kind == STEM:
        H, W = H or 2 * Ho, W or 2 * Wo - 1
        assert (H - 1) // 2 + 1 == Ho and (W - 1) // 2 + 1 == Wo and K == 147
        if layout == 2:
            x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        else:
            x = (3.0 * rng.standard_normal((B, 3, H, W)) + 0.5).astype(np.float32)
            if layout == 1:
                x = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float16)
        c["es"], c["et"] = _bn(rng, N)
        ldx = 0
    elif kind == C3X3:
        H, W, ldx = Ho, Wo, 128
        assert K == 1152
        x = rng.standard_normal((B, H, W, 128)).astype(np.float32)
        c["s"], c["t"] = _bn(rng, 128)
    else:
        H, W = (Ho, Wo) if kind == C1X1 else (H or 2 * Ho, W or 2 * Wo)
        ldx = K + 32
        x = rng.standard_normal((B, H, W, ldx)).astype(np.float32)
        x[..., K:] = np.nan
        c["s"], c["t"] = _bn(rng, K)
    c.update(x=x, ldx=ldx, H=H, W=W, w=(0.05 * rng.standard_normal((K, N))).astype(np.float32))
    return c
