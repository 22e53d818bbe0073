"""Float64 reference of the transition and layer-wise kernels - conv1x1_kernel<MI, POOL, NB, EX, ONCE> (csrc/conv1x1.hip),
trans_ws_kernel<NK, BM, NB> (csrc/trans_ws.hip), conv3x3_kernel<V, EX> (csrc/conv3x3.hip) -, the componentwise bound the device is held
to, an fp32 model of the kernels' arithmetic with one defect at a time, the input generators, the table of instantiations with the
dispatch rules restated, and the list of cases tests/test_gpu_layerwise_instantiations.py runs - numpy only, built on
tests/tools/strip_ref.py and tile_ref.py.

``reference(inp) -> (y, E16, y32, E32)``, everything in float64; nothing of the kernels' tiling is restated:

    conv1x1, no pool   a = clip(x, lo, hi) with `clamp` (exact: no arithmetic), else a = relu(x s + t) (device: one fp32 fma, one
                       rounding to fp16);  y = a @ w.T + bias
    conv1x1, pool      a = the mean of the four relu(x s + t) of AvgPool2D(2, 2) with floor (an odd map's last row and column are
                       dropped), NOT rounded (device: four fp32 fmas, three fp32 additions, a multiplication by 0.25, then the split
                       hi = fp16(m), lo = fp16(m - hi), and both are multiplied);  y = a @ w.T (+ bias)
    exact mode         w = hi + lo, two fp16 arrays of independent content (row pitch 2 Kp, Kp = K rounded up to 64)
    conv3x3            a = relu(x s + t) (device: rounded once to fp16); y = conv3x3(a, w), zero padding behind the activation, every
                       frame on its own; exact mode: w = hi + lo

y32 is y (the device stores the fp32 accumulator besides its fp16 rounding); E32 bounds |y32_dev - y|, E16 bounds |y_dev - y|.

The bound is derived, never measured.  u = 2^-11 (half an fp16 ulp, relative), e = 2^-24 (fp32's unit roundoff):

    operand, no pool   da = u a + e |x s + t| + 2^-25      the fma's one rounding, the rounding to fp16 (ReLU is 1-Lipschitz), and half
                                                           an fp16 subnormal step - which for a normal number is room, and covers the
                                                           cross term u e |x s + t| < 2^-25 of every |x s + t| < 1024;  clamp: da = 0
    operand, pool      dm = 0.25 (e sum_s |x_s s + t| + 3 e sum_s relu_s)      the four fma roundings and the three additions, each
                                                           addition's result being at most the whole sum; the 0.25 is exact
                       da = dm + u^2 (a + dm) + 2^-25      the subtraction m - hi is exact (hi is m's neighbour), |lo| <= u |m|, the u^2
                                                           term is the rounding of lo alone, 2^-25 half a subnormal step of lo
    accumulation       (n + 16) e sum_k |w| (a + da)       fp32 accumulation of exact products in ANY order is within (n - 1) e sum |terms|
                                                           to first order; 17 terms of room for the chained MFMAs' own accumulator
                                                           additions and the second order (n e < 2^-12 here: less than one term).
                                                           The sum runs over |w_hi| + |w_lo| in exact mode.  n = products per output:
                                                           K; 2 K with pool (hi and lo operand); 2 Kp in exact mode, 4 K exact + pool;
                                                           1152 conv3x3, 2304 exact conv3x3
    conv3x3            the same accumulation term: the kernel sums four partial sums of 288 (576) products with three fp32 additions,
                       which is ONE summation order of the 1152 (2304) products - the three joins are among the n - 1 additions the
                       term counts, so the + 16 needs no enlarging
    E32 = sum_k |w| da + accumulation + e |y| (bias: one more fp32 addition) + one fp32 ulp of y
    E16 = u |y| + (1 + u) E32 + 2^-25

The statistic is max |dev - ref| / E <= 1, reported separately for y and y32.

Near or outside the bound's reach on real-valued inputs (listed, not worked around; tests/test_cpu_layerwise_ref.py records the figures):
the lo half of the pooled operand missing - |lo| <= u a is of the size the output's own rounding allows, and the `noisy` inputs see it
(1.3 to 22 times the bound in y, 1.8 to 46 in y32) only through the planted channels, whose large lo halves add up in one direction;
the bias added behind the rounding, a second rounding that shows only where enough outputs carry a bias against the sum's sign; a
one-row map has no tap in the conv3x3's fourth partial sum.  The `integer` inputs see the first in every case, the second in the pooled
case (quarter-integers beyond fp16's precision).

``model(inp, defect)`` is an fp32 restatement of the arithmetic - the fma, the roundings, the hi / lo split, accumulation k-step by
k-step with hi then lo - with one defect at a time."""
from __future__ import annotations

import numpy as np

from .strip_ref import E32, F16_MAX, U16, _conv3x3, _h, clamp_consts, ratio  # noqa: F401
from .tile_ref import _w3_map, split_hi_lo

SENTINEL = 300.0        # behind K in x, around the output columns of y, behind N in y32: never read, never written
STALE = -77.0           # inside the output columns: has to be overwritten
EXACT = 1 << 17
YOFF = 40


# ---- the instantiations and the dispatch -------------------------------------------------------------------------------------------
# template argument lists as data: conv1x1_kernel<MI, POOL, NB, EX, ONCE>, trans_ws_kernel<NK, BM, NB>, conv3x3_kernel<V, EX>
INSTANTIATIONS = ([("conv1x1_kernel", (mi, False, 128, ex, False)) for mi in (4, 2, 1) for ex in (False, True)] +
                  [("conv1x1_kernel", (2, True, nb, True, False)) for nb in (256, 128)] +
                  [("conv1x1_kernel", (2, True, nb, False, once)) for nb in (256, 128) for once in (True, False)] +
                  [("trans_ws_kernel", t) for t in ((16, 64, 512), (0, 64, 512), (8, 128, 256), (0, 128, 256))] +
                  [("conv3x3_kernel", t) for t in ((1, True), (0, False), (1, False))])
assert len(set(INSTANTIATIONS)) == len(INSTANTIATIONS) == 12 + 4 + 3


def trans_ws_supported(a) -> bool:
    """trans_ws.hip::trans_ws_supported restated"""
    return bool(a["pool"] and not a["exact"] and not a["bias"] and a["N"] in (512, 256) and a["K"] % 128 == 0 and a["H"] % 2 == 0 and a["W"] % 2 == 0 and
                a["H"] >= 2 and a["W"] >= 2 and a["M"] % ((a["H"] // 2) * (a["W"] // 2)) == 0)


def instantiation_of(a, nt_mb: int = 128):
    """the instantiation launch_conv1x1 / launch_trans_ws / launch_conv3x3 pick for the launch arguments a (``launch_args``); nt_mb: the
    non-temporal threshold of the process (TN_TRANS_NT_MB, 128 by default)"""
    if a["op"] == "conv3x3":
        return "conv3x3_kernel", (1, True) if a["exact"] else (0, False) if a["variant"] == 9 else (1, False)
    if a["wfrag"] and trans_ws_supported(a):
        if a["N"] == 512:
            return "trans_ws_kernel", (16 if a["K"] == 16 * 64 else 0, 64, 512)
        return "trans_ws_kernel", (8 if a["K"] == 8 * 64 else 0, 128, 256)
    if a["pool"]:
        wide = a["N"] % 256 == 0
        nt = a["N"] // (256 if wide else 128)
        if a["exact"]:
            return "conv1x1_kernel", (2, True, 256 if wide else 128, True, False)
        stream = nt == 1 and a["M"] * 4 * a["ldx"] * 2 > (nt_mb << 20)
        return "conv1x1_kernel", (2, True, 256 if wide else 128, False, stream)
    mi = 4 if a["M"] >= 128 * 512 else 2 if a["M"] >= 64 * 512 else 1
    return "conv1x1_kernel", (mi, False, 128, bool(a["exact"]), False)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _case(op, inst, gen, **kw):
    c = dict(op=op, inst=inst, gen=gen, K=128, N=32, exact=False, bias=False, clamp=False, variant=0, nt_mb=128, B=1, H=0, W=0)
    c.update(kw)
    if op in ("pool", "ws"):
        c["M"] = c["B"] * (c["H"] // 2) * (c["W"] // 2)
    elif op == "c3":
        c["M"] = c["B"] * c["H"] * c["W"]
    shape = "M%d" % c["M"] if op == "c1" else "%dx%dx%d" % (c["B"], c["H"], c["W"])
    c["id"] = "-".join([op, shape] + (["K%d" % c["K"], "N%d" % c["N"]] if op != "c3" else ["v%d" % c["variant"]]) +
                       [n for n in ("exact", "bias", "clamp") if c[n]] + (["once"] if c["nt_mb"] == 0 else []) + [gen])
    return c


def kp_of(k: int) -> int:
    return (k + 63) // 64 * 64


def ldx_of(c) -> int:
    return 128 if c["op"] == "c3" else c["K"] + 64


def launch_args(c):
    return dict(op="conv3x3" if c["op"] == "c3" else "conv1x1", pool=c["op"] in ("pool", "ws"), exact=c["exact"], bias=c["bias"], N=c["N"], K=c["K"],
                H=c["H"], W=c["W"], M=c["M"], ldx=ldx_of(c), wfrag=c["op"] == "ws", variant=c["variant"])


def _cases():
    out = []
    for gen in ("noisy", "integer"):
        # conv1x1, no pool: every MI with the ragged last tile; K = 96: a dead half k-tile (exact: Kp = 128); bias x clamp x exact x N
        for mi, m in ((4, 128 * 512 + 5), (2, 64 * 512 + 7), (1, 300)):
            out += [_case("c1", ("conv1x1_kernel", (mi, False, 128, False, False)), gen, M=m, K=64, N=128),
                    _case("c1", ("conv1x1_kernel", (mi, False, 128, False, False)), gen, M=m, K=96, N=256, bias=True, clamp=True),
                    _case("c1", ("conv1x1_kernel", (mi, False, 128, True, False)), gen, M=m, K=96, N=128, exact=True, bias=True),
                    _case("c1", ("conv1x1_kernel", (mi, False, 128, True, False)), gen, M=m, K=64, N=256 if mi == 1 else 128, exact=True, clamp=True)]
        out += [_case("c1", ("conv1x1_kernel", (1, False, 128, False, False)), gen, M=1, K=64, N=128, bias=True),
                _case("c1", ("conv1x1_kernel", (1, False, 128, True, False)), gen, M=1, K=96, N=128, exact=True, clamp=True),
                _case("c1", ("conv1x1_kernel", (1, False, 128, False, False)), gen, M=300, K=992, N=128, bias=True),
                _case("c1", ("conv1x1_kernel", (1, False, 128, True, False)), gen, M=300, K=992, N=128, exact=True)]
        # conv1x1, pool (the tiled transition kernel)
        w256, w128 = ("conv1x1_kernel", (2, True, 256, False, False)), ("conv1x1_kernel", (2, True, 128, False, False))
        out += [_case("pool", w256, gen, N=512, K=256, B=3, H=14, W=14),                    # NT = 2
                _case("pool", w256, gen, N=256, K=128, B=2, H=10, W=12),                    # NT = 1
                _case("pool", w128, gen, N=384, K=96, B=2, H=15, W=15),                     # NT = 3, the odd map, K % 64 == 32
                _case("pool", w128, gen, N=128, K=64, B=1, H=6, W=6),                       # M = 9: one real pixel tile in a group of eight
                _case("pool", w256, gen, N=1024, K=64, B=1, H=6, W=6),                      # NT = 4
                _case("pool", w128, gen, N=128, K=64, B=3, H=28, W=28, bias=True),          # M = 588: ten pixel tiles, a second group of eight
                _case("pool", ("conv1x1_kernel", (2, True, 256, True, False)), gen, N=256, K=128, B=3, H=14, W=14, exact=True),
                _case("pool", ("conv1x1_kernel", (2, True, 128, True, False)), gen, N=128, K=128, B=2, H=15, W=15, exact=True)]
        # the warp-specialised transition kernel
        for inst, n, k, maps in (((16, 64, 512), 512, 1024, ((14, 14), (32, 32))),
                                 ((0, 64, 512), 512, 128, ((2, 2), (14, 14))), ((0, 64, 512), 512, 256, ((10, 12), (30, 30))),
                                 ((8, 128, 256), 256, 512, ((28, 28), (30, 30))),
                                 ((0, 128, 256), 256, 128, ((14, 14), (2, 2), (10, 12)))):
            out += [_case("ws", ("trans_ws_kernel", inst), gen, N=n, K=k, B=3, H=h, W=w) for h, w in maps]
        # conv3x3
        for inst, variant, exact in (((1, False), 0, False), ((0, False), 9, False), ((1, True), 0, True)):
            out += [_case("c3", ("conv3x3_kernel", inst), gen, B=b, H=h, W=w, variant=variant, exact=exact)
                    for b, h, w in ((3, 7, 7), (1, 9, 13), (2, 14, 14), (2, 1, 5), (1, 2, 240))]
    return out


def _once_cases():
    """the two non-temporal instantiations: reached with TN_TRANS_NT_MB=0, which a process reads once - run in a child"""
    return [_case("pool", ("conv1x1_kernel", (2, True, nb, False, True)), gen, N=n, K=k, B=2, H=h, W=w, nt_mb=0)
            for gen in ("noisy", "integer") for nb, n, k, h, w in ((256, 256, 128, 10, 12), (128, 128, 64, 15, 15))]


CASES = _cases()
ONCE_CASES = _once_cases()
ALL_CASES = CASES + ONCE_CASES
assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)


# ---- where the kernels change owner (for the plants of `noisy`; nothing of this enters `reference`) ---------------------------------
def seam_rows(c):
    """output rows (pixels, pooled pixels) next to a place where a kernel changes owner: conv1x1 - the first and the last row of every
    32-row unit of a pixel tile, and row M - 1; trans_ws - per frame the last row of each of its ceil(P / BM) equal tiles, the first of
    the next, and both sides of the 32-row fragment boundaries inside a tile; pool - besides, the pooled pixels of a frame's last pooled
    row and column"""
    m = c["M"]
    rows = {0, m - 1} | {r for r in range(31, m, 32)} | {r for r in range(32, m, 32)}
    if c["op"] in ("pool", "ws"):
        ho, wo = c["H"] // 2, c["W"] // 2
        p = ho * wo
        for b in range(c["B"]):
            rows |= {b * p + (ho - 1) * wo + x for x in range(wo)} | {b * p + y * wo + wo - 1 for y in range(ho)}
        if c["op"] == "ws":
            bm = 64 if c["N"] == 512 else 128
            tpf = (p + bm - 1) // bm
            pt = (p + tpf - 1) // tpf
            for b in range(c["B"]):
                for p0 in range(0, p, pt):
                    for q in (p0 - 1, p0, p0 + pt - 1):
                        rows.add(b * p + min(max(q, 0), p - 1))
                    for q in range(p0 + 32, min(p0 + pt, p), 32):
                        rows |= {b * p + q - 1, b * p + q}
    return np.array(sorted(r for r in rows if 0 <= r < m))


def _plant_mask(c):
    """bool mask over x's pixels (and channels, conv1x1) of where `noisy` plants |x| in [20, 60]"""
    k = c["K"]
    if c["op"] == "c1":
        mk = np.zeros((c["M"], k), bool)
        mk[seam_rows(c)] = True
        mk[:, [0, k - 1]] = True
        mk[:, k - 8:] = True                                                     # the last 8-channel chunk before K
        return mk
    b, h, w = c["B"], c["H"], c["W"]
    if c["op"] == "c3":
        mk = np.zeros((b, h, w), bool)
        mk[:, [0, h - 1]] = True
        mk[:, :, [0, w - 1]] = True
        flat = mk.reshape(-1)
        for m0 in range(128, flat.size, 128):                                    # both sides of every 128-pixel tile seam
            flat[[m0 - 1, m0]] = True
        return np.broadcast_to(mk[..., None], (b, h, w, 128)).copy()
    ho, wo = h // 2, w // 2
    mk = np.zeros((b, h, w), bool)
    r = seam_rows(c)
    fb, py, px = r // (ho * wo), (r % (ho * wo)) // wo, r % wo
    for dy in (0, 1):
        for dx in (0, 1):
            mk[fb, 2 * py + dy, 2 * px + dx] = True
    mk[:, 2 * ho:] = True                                                        # an odd map's dropped row and column
    mk[:, :, 2 * wo:] = True
    mk = np.broadcast_to(mk[..., None], (b, h, w, k)).copy()
    mk[..., [0, k - 1]] = True
    return mk


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def _runs(rng, n, k, count, stride):
    """(n, k) in {-1, 0, 1}: row i has `count` non-zeros, a run from stride i mod k, as many +1 as -1"""
    w = np.zeros((n, k), np.float32)
    for i in range(n):
        w[i, (stride * i + np.arange(count)) % k] = rng.permutation(np.repeat([-1.0, 1.0], count // 2))
    return w


def _bn_consts(rng, k):
    """BatchNorm constants of both signs, some channels dead behind the ReLU"""
    s = (rng.uniform(0.5, 1.5, k) * np.where(rng.random(k) < 0.3, -1.0, 1.0)).astype(np.float32)
    t = rng.normal(0, 0.3, k).astype(np.float32)
    dead = rng.random(k) < 0.04
    s[dead], t[dead] = np.float32(0.01), np.float32(-90.0)
    return s, t


def x_shape(c):
    return (c["M"], c["K"]) if c["op"] == "c1" else (c["B"], c["H"], c["W"], 128 if c["op"] == "c3" else c["K"])


def noisy(c, seed: int = 0):
    """The distributions of tests/test_gpu_kernels.py (Gaussian activations of sigma 1.5, Gaussian weights of variance 2 / fan-in) with
    BatchNorm constants of both signs and dead channels - `clamp`: strip_ref.clamp_consts, all three kinds - and |x| in [20, 60] of random
    sign planted where ``_plant_mask`` says"""
    rng = np.random.default_rng([seed, c["M"], c["K"], c["N"], c["H"], c["W"], int(c["exact"]), int(c["clamp"])])
    shape = x_shape(c)
    k = shape[-1]
    x = rng.normal(0, 1.5, shape).astype(np.float32)
    big = (rng.uniform(20.0, 60.0, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    mk = _plant_mask(c)
    x[mk] = big[mk]
    s, t = clamp_consts(rng, k) if c["clamp"] else _bn_consts(rng, k)
    inp = dict(op=c["op"], clamp=c["clamp"], x=x.astype(np.float16), s=s, t=t)
    wshape, fan = ((32, 128, 3, 3), 1152) if c["op"] == "c3" else ((c["N"], k), k)
    w = rng.normal(0, np.sqrt(2.0 / fan), wshape).astype(np.float32)
    if c["exact"]:
        inp["w"], inp["w_lo"] = split_hi_lo(w)
    else:
        inp["w"] = _h(w)
    if c["bias"]:
        inp["bias"] = rng.normal(0, 0.5, c["N"]).astype(np.float32)
    return inp


def integer(c, seed: int = 0):
    """Every rounding exact, so the device has to return the float64 values bit for bit (y32) and their round-to-nearest-even halves (y).
    no pool: x in {0, 1}, s = 1 with integer t in [-1, 3] (or, `clamp`, lo = 0 and hi = 65504: a clamp that passes), w in {-1, 0, 1} with
      16 non-zeros per row (a balanced run from 11 n mod K), integer bias in [-8, 8]; exact mode: a lo array of its own, 8 non-zeros per row
      (a run from 7 n mod K).
    pool: integer x in [0, 480], s = 1, integer t in [512, 527]: every relu(x + t) lies in [512, 1008], the sum of four is exact in fp32 and
      the mean is a quarter-integer in [512, 1024) - 12 significant bits, so lo = +-0.25 whenever the sum is odd; in every channel
      k % 4 == 0 the top left source pixel is moved by one where needed to MAKE it odd.  w in {-1, 0, 1} with 8 non-zeros per row (a balanced
      run from 5 n mod K: it holds two channels k % 4 == 0, so every output sums at least two operands with lo != 0); exact mode: a lo
      array with 4 non-zeros per row (a run from 3 n mod K).  |y| < 6 * 512: quarter-integers, exact in fp32 in any order.
    conv3x3: x in {0, 1}, s = 1, t in [0, 2]; tile_ref._w3_map, both maps in exact mode (|y| <= 72 * 3)."""
    rng = np.random.default_rng([seed, c["M"], c["K"], c["N"], c["H"], c["W"], int(c["exact"]), int(c["clamp"]), 1])
    shape = x_shape(c)
    k = shape[-1]
    inp = dict(op=c["op"], clamp=c["clamp"])
    if c["op"] in ("pool", "ws"):
        b, h, w = shape[:3]
        ho, wo = h // 2, w // 2
        x = rng.integers(0, 480, shape).astype(np.int64)
        even = _pooled(x).sum(axis=(2, 4)) % 2 == 0
        even[..., np.arange(k) % 4 != 0] = False
        x[:, 0:2 * ho:2, 0:2 * wo:2] += even           # the top left source pixel of every pooled pixel
        inp.update(x=x.astype(np.float16), s=np.ones(k, np.float32), t=rng.integers(512, 528, k).astype(np.float32))
        inp["w"] = _runs(rng, c["N"], k, 8, 5)
        if c["exact"]:
            inp["w_lo"] = _runs(rng, c["N"], k, 4, 3)
    elif c["op"] == "c1":
        inp["x"] = rng.integers(0, 2, shape).astype(np.float16)
        if c["clamp"]:
            inp.update(s=np.zeros(k, np.float32), t=np.full(k, F16_MAX, np.float32))
        else:
            inp.update(s=np.ones(k, np.float32), t=rng.integers(-1, 4, k).astype(np.float32))
        inp["w"] = _runs(rng, c["N"], k, 16, 11)
        if c["exact"]:
            inp["w_lo"] = _runs(rng, c["N"], k, 8, 7)
    else:
        inp.update(x=rng.integers(0, 2, shape).astype(np.float16), s=np.ones(k, np.float32), t=rng.integers(0, 3, k).astype(np.float32))
        inp["w"] = _w3_map(rng, False)
        if c["exact"]:
            inp["w_lo"] = _w3_map(rng, True)
    if c["bias"]:
        inp["bias"] = rng.integers(-8, 9, c["N"]).astype(np.float32)
    return inp


GENERATORS = {"noisy": noisy, "integer": integer}


def make(c, seed: int = 0):
    return GENERATORS[c["gen"]](c, seed)


# ---- reference and bound --------------------------------------------------------------------------------------------------------------
def _pooled(v):
    """(B,H,W,K) -> the four sources of every pooled pixel (B,Ho,2,Wo,2,K): AvgPool2D(2, 2) with floor"""
    b, h, w, k = v.shape
    return v[:, :h // 2 * 2, :w // 2 * 2].reshape(b, h // 2, 2, w // 2, 2, k)


def operand(inp):
    """-> (a, da) in float64: the GEMM's left operand as defined and the bound of the device's error in it; conv1x1: (rows, K)"""
    x = inp["x"].astype(np.float64)
    s, t = inp["s"].astype(np.float64), inp["t"].astype(np.float64)
    if inp["clamp"]:
        a = np.clip(x, s, t)
        return a, np.zeros_like(a)
    z = x * s + t
    r = np.maximum(z, 0.0)
    if inp["op"] in ("pool", "ws"):
        a = 0.25 * _pooled(r).sum(axis=(2, 4))
        dm = 0.25 * (E32 * _pooled(np.abs(z)).sum(axis=(2, 4)) + 3 * E32 * _pooled(r).sum(axis=(2, 4)))
        da = dm + U16 * U16 * (a + dm) + 2.0 ** -25
        return a.reshape(-1, x.shape[-1]), da.reshape(-1, x.shape[-1])
    return r, U16 * r + E32 * np.abs(z) + 2.0 ** -25


def products(inp) -> int:
    """n: the products summed per output"""
    if inp["op"] == "c3":
        return 2304 if "w_lo" in inp else 1152
    k = inp["x"].shape[-1]
    pool = inp["op"] in ("pool", "ws")
    if "w_lo" in inp:
        return 4 * k if pool else 2 * kp_of(k)
    return 2 * k if pool else k


def reference(inp):
    """-> (y, E16, y32, E32), float64; conv1x1: (M, N), conv3x3: (B,H,W,32) (y32 is y: the kernel has no fp32 output, E32 is the error
    in front of the rounding)"""
    a, da = operand(inp)
    w = inp["w"].astype(np.float64)
    wa = np.abs(w)
    if "w_lo" in inp:
        w = w + inp["w_lo"].astype(np.float64)
        wa = wa + np.abs(inp["w_lo"].astype(np.float64))
    n = products(inp)
    if inp["op"] == "c3":
        y = _conv3x3(a, w)
        e32 = _conv3x3(da + (n + 16) * E32 * (a + da), wa)
    else:
        y = a @ w.T
        e32 = (da + (n + 16) * E32 * (np.abs(a) + da)) @ wa.T
        if "bias" in inp:
            y = y + inp["bias"].astype(np.float64)
            e32 = e32 + E32 * np.abs(y)
    e32 = e32 + np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
    return y, U16 * np.abs(y) + (1.0 + U16) * e32 + 2.0 ** -25, y, e32


# ---- the buffers of a case ------------------------------------------------------------------------------------------------------------
def x_buffer(c, inp):
    """x with row pitch ldx = K + 64 and SENTINEL in the channels behind K (conv3x3: the dense (M, 128) map itself)"""
    x = inp["x"]
    if c["op"] == "c3":
        return x
    buf = np.full(x.shape[:-1] + (ldx_of(c),), SENTINEL, np.float16)
    buf[..., :x.shape[-1]] = x
    return buf


def y_buffers(c):
    """-> (y (M, yoff + N + 24) fp16: SENTINEL outside [yoff, yoff + N), STALE inside; y32 (M, N + 8) fp32 likewise, columns [0, N))"""
    n = c["N"]
    y = np.full((c["M"], YOFF + n + 24), SENTINEL, np.float16)
    y[:, YOFF:YOFF + n] = STALE
    y32 = np.full((c["M"], n + 8), SENTINEL, np.float32)
    y32[:, :n] = STALE
    return y, y32


def weight_rows(inp):
    """the 1x1 weights as the kernel reads them: [N][K] fp16, exact mode [N][2 Kp] = [hi | lo] with SENTINEL in the padding columns
    (never read: the kernel stops at K)"""
    w = inp["w"]
    if "w_lo" not in inp:
        return w.astype(np.float16)
    n, k = w.shape
    kp = kp_of(k)
    out = np.full((n, 2 * kp), SENTINEL, np.float16)
    out[:, :k] = w
    out[:, kp:kp + k] = inp["w_lo"]
    return out


def behind(buf, kp: int, k: int):
    """what a read of K channels from channel Kp onward finds at every pixel of the x buffer (running on into the next pixel's row where
    the pitch ends; zeros behind the last pixel): the operand of ``model``'s no_wrap defect, in x's own shape"""
    ld = buf.shape[-1]
    flat = np.concatenate([buf.reshape(-1), np.zeros(kp + k, buf.dtype)])
    idx = (np.arange(buf.size // ld) * ld + kp)[:, None] + np.arange(k)[None, :]
    return flat[idx].reshape(buf.shape[:-1] + (k,))


def frag_order(w16):
    """numpy restatement of the fragment order of the warp-specialised kernel's weights: [N][K] -> [K / 16][N / 32][64 lanes][8], lane l
    holding row l & 31 and k offset 8 (l >> 5)"""
    n, k = w16.shape
    v = w16.reshape(n // 32, 32, k // 16, 2, 8)                 # [ct][row][g][half][j]
    return np.ascontiguousarray(v.transpose(2, 0, 3, 1, 4)).reshape(-1)      # [g][ct][half][row][j]: lane = 32 half + row


# ---- the fp32 model of the kernels' arithmetic ---------------------------------------------------------------------------------------
DEFECTS = ("no_lo", "drop_tail", "double_tail", "no_wrap", "pool_neighbour", "pool_next_frame", "bias_after", "clamp_as_bn", "frame_border",
           "lo_at_hi", "drop_partial")


def _fma(x, s, t):
    return (x.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)).astype(np.float32)       # one rounding


def _model_operand(inp, x, defect):
    """-> (hi, lo | None) float32 (rows, K) from activations x in the input's own shape"""
    s, t = inp["s"], inp["t"]
    k = x.shape[-1]
    if inp["op"] in ("pool", "ws"):
        b, h, w, _ = x.shape
        ho, wo = h // 2, w // 2
        m = np.arange(b * ho * wo)
        fb, py, px = m // (ho * wo), (m % (ho * wo)) // wo, m % wo
        if defect == "pool_next_frame":
            fb = (fb + 1) % b
        base = (fb * h + 2 * py) * w + 2 * px
        offs = (0, 1, w + 1, w + 2) if defect == "pool_neighbour" else (0, 1, w, w + 1)
        flat = x.reshape(-1, k)
        acc = np.zeros((m.size, k), np.float32)
        for o in offs:
            acc = acc + np.maximum(_fma(flat[np.minimum(base + o, len(flat) - 1)], s, t), np.float32(0.0))
        mean = np.float32(0.25) * acc
        hi = _h(mean)
        return hi, (None if defect == "no_lo" else _h(mean - hi))
    x = x.reshape(-1, k)
    if inp["clamp"] and defect != "clamp_as_bn":
        return np.clip(x.astype(np.float32), s, t), None
    return _h(np.maximum(_fma(x, s, t), np.float32(0.0))), None


def model(inp, defect=None, buf=None):
    """-> (y, y32) float32 (y holding fp16 numbers): what a kernel that does the defined arithmetic in the kernels' precision stores.
    buf: the x buffer of the case (``x_buffer``), needed by `no_wrap`.  One defect at a time:
      no_lo            the lo half of the pooled operand is not multiplied
      drop_tail        the last 32-channel k-step of a K % 64 == 32 layer is missing (exact mode: of both passes); double_tail: done twice
      no_wrap          exact mode: the lo-weight pass reads activation channels Kp + k of the buffer instead of wrapping to channel k
      pool_neighbour   the two source pixels of row 2 py + 1 are taken one column further on
      pool_next_frame  the four source pixels are taken from the next frame
      bias_after       the bias is added to the rounded fp16 result
      clamp_as_bn      the clamp constants are applied as scale and shift
      frame_border     conv3x3: tap validity from m / W without the % H - a tap across a frame border inside the batch is not zeroed
      lo_at_hi         conv3x3, exact: the lo image is read at the hi image's offset
      drop_partial     conv3x3: the last of the four partial sums is missing"""
    assert defect is None or defect in DEFECTS
    if inp["op"] == "c3":
        return _model_c3(inp, defect)
    k = inp["x"].shape[-1]
    hi, lo = _model_operand(inp, inp["x"], defect)
    passes = [(inp["w"].astype(np.float32), hi, lo)]
    if "w_lo" in inp:
        h2, l2 = hi, lo
        if defect == "no_wrap":
            h2, l2 = _model_operand(inp, behind(buf, kp_of(k), k), None)
        passes.append((inp["w_lo"].astype(np.float32), h2, l2))
    acc = np.zeros((hi.shape[0], inp["w"].shape[0]), np.float32)
    for wv, ah, al in passes:                                                     # exact mode: the hi-weight pass, then the lo-weight pass
        for q in range(k // 32):                                                  # one 32-channel k-step per MFMA: operand hi, then lo
            tail = k % 64 == 32 and q == k // 32 - 1
            for _ in range(0 if tail and defect == "drop_tail" else 2 if tail and defect == "double_tail" else 1):
                acc += ah[:, 32 * q:32 * q + 32] @ wv[:, 32 * q:32 * q + 32].T
                if al is not None:
                    acc += al[:, 32 * q:32 * q + 32] @ wv[:, 32 * q:32 * q + 32].T
    bias = inp.get("bias", np.float32(0.0))
    y32 = (acc + bias).astype(np.float32)
    return (_h(_h(acc) + bias) if defect == "bias_after" else _h(y32)), y32


def _model_c3(inp, defect):
    x = inp["x"]
    b, h, w, _ = x.shape
    a = _h(np.maximum(_fma(x, inp["s"], inp["t"]), np.float32(0.0)))
    if defect == "frame_border":
        a = a.reshape(1, b * h, w, 128)
    p = np.zeros((a.shape[0], a.shape[1] + 2, w + 2, 128), np.float32)
    p[:, 1:-1, 1:-1] = a
    wh = inp["w"].astype(np.float32)
    wl = (wh if defect == "lo_at_hi" else inp["w_lo"].astype(np.float32)) if "w_lo" in inp else None
    parts = [np.zeros(a.shape[:3] + (32,), np.float32) for _ in range(4)]
    for s in range(72):                                                           # k-step s: tap s >> 3, channels 16 (s & 7) ...; 18 per wave
        (dy, dx), ch = divmod(s >> 3, 3), 16 * (s & 7)
        rows = p[:, dy:dy + a.shape[1], dx:dx + w, ch:ch + 16]
        parts[s // 18] += rows @ wh[:, ch:ch + 16, dy, dx].T
        if wl is not None:
            parts[s // 18] += rows @ wl[:, ch:ch + 16, dy, dx].T
    y = (parts[0] + parts[1]) + parts[2]
    if defect != "drop_partial":
        y = y + parts[3]
    y = y.reshape(b, h, w, 32)
    return _h(y), y
