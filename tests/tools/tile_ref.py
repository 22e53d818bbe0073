"""Float64 reference of the fused dense layer as the TILE kernel defines it (csrc/dense_layer_big.hip, dense_layer_kernel<W, ROUT, BM,
BK, PP, CHAIN, EX>), the componentwise bound the device is held to, an fp32 model of the kernel's arithmetic with one defect at a
time, the input generators and the table of instantiations - numpy only, built on tests/tools/strip_ref.py.

``reference``: unlike the strip kernel the tile kernel does not fold BN2 into the weights.  Everything in float64 unless stated:

    a1   = clip(x, lo, hi)                       exact: no arithmetic (s1, t1 carry lo, hi)
    bott = a1 @ w1.T                             w1 holds fp16 numbers; exact mode: w1 = hi + lo, two fp16 arrays
    z    = bott * s2 + t2                        (device: one fp32 fma)
    a2   = relu(z)                               (device: rounded to fp16 once, then packed max with 0)
    y    = conv3x3(a2, w3), zero padding behind the activation; exact mode: w3 = hi + lo

The device rounds a2 and y to fp16 once each; the reference rounds neither and restates nothing of the tile layout, wave split,
swizzles or rings: a product that is dropped, doubled or taken from the wrong place is a difference.

``E`` is derived, not measured.  u = 2^-11, e = 2^-24, n = K (exact mode: 2 Kp, Kp = K rounded up to BK), n3 = 1152 (exact: 2304):

    db(p, c) = (n + 16) e sum_k |a1| |w1|        fp32 accumulation of exact fp16 products in any order is within (n - 1) e sum |terms|;
                                                 + 17 terms of room for the chained MFMAs' own accumulator additions (exact mode: the
                                                 sum runs over |hi| + |lo|)
    dz(p, c) = |s2| db (1 + e) + e |z|           the fp32 fma of BN2: the operand's error scaled, one rounding of the result
    da(p, c) = u (a2 + dz) + dz + 2^-25          ReLU is 1-Lipschitz; one rounding to fp16 of a value of at most a2 + dz; 2^-25 is half
                                                 an fp16 subnormal step
    E(p, o)  = u |y| + (1 + u) [sum_{tap, c} |w3| da + (n3 + 16) e sum |w3| (a2 + da)] + 2^-25
                                                 the operand's error through the 3x3, the fp32 accumulation of n3 products in ONE
                                                 accumulator per output in any order, one rounding to fp16 of the sum

The statistic is max |y_dev - y| / E <= 1.

Outside the bound's reach (listed, not worked around): a rounding of a2 or y other than to nearest that stays within u; a
perturbation of the bottleneck below u a2; on real-valued inputs a single missing 3x3 product of an average weight (E sums u |w3| a2
over all n3 products, so only products of weights well above average stand out - the `integer` inputs see every one); in exact mode
the lo image of the 3x3 missing altogether (|lo| <= u |hi|: as large as the rounding of a2; the `integer` inputs see it).

``model`` is an fp32 restatement of the kernel's arithmetic - accumulation k-step by k-step over 32 channels per MFMA, the fma, the
two fp16 roundings, in exact mode the hi pass and then the lo pass - with one defect at a time (tests/test_cpu_tile_ref.py)."""
from __future__ import annotations

import numpy as np

from .strip_ref import E32, F16_MAX, U16, _conv3x3, _h, clamp_consts, ratio  # noqa: F401  (shared with the strip reference)

# DLGeom<W, ROUT, BM, BK> restated: map size -> (ROUT output rows of a tile, BK channels of a k-tile, KMAX input channels); BM, the
# flattened phase-A rows of a tile, is 512 / 512 / 256 / 384 / 384 / 384 and at 7 x 7 64 (4 x 2 wave split) or 128 (8 x 1)
GEOM = {56: (7, 32, 256), 28: (14, 32, 512), 14: (14, 64, 1024), 7: (7, 64, 1024), 64: (4, 32, 1024), 32: (8, 32, 1024), 16: (16, 32, 1024)}
BMS = {56: (512,), 28: (512,), 14: (256,), 7: (64, 128), 64: (384,), 32: (384,), 16: (384,)}


def rout(h): return GEOM[h][0]
def bk_of(h): return GEOM[h][1]
def kmax(h): return GEOM[h][2]


def kp_of(h: int, k: int) -> int:
    """K rounded up to BK: the half pitch of the exact-mode 1x1 weights [128][2 Kp] = [hi | lo]"""
    bk = bk_of(h)
    return (k + bk - 1) // bk * bk


def smallest_ldc(k: int) -> int:
    """K + 32 rounded up to 8 (K % 32 == 0: K + 32 itself)"""
    return (k + 32 + 7) // 8 * 8


def case_ldc(k: int) -> int:
    """the smallest legal row pitch for odd K / 32, one 128-byte line more otherwise"""
    return smallest_ldc(k) + (0 if (k // 32) % 2 else 64)


# ---- where the kernel changes owner -----------------------------------------------------------------------------------------------
def wave_starts(h: int, bm: int):
    """first flattened phase-A row of each wave's share of a tile (dense_layer_kernel: mrow0): BM / 8 rows per wave; at 28 x 28
    (REBAL: 28 real 16-row fragments in a 32-fragment tile) waves 0-3 own 64 rows and waves 4-7 own 48; at BM = 64 (7 x 7, NSPLIT) four
    16-row groups (each computed by two waves, one per channel half)"""
    if bm == 64:
        return [16 * i for i in range(4)]
    if h == 28:
        return [64 * i for i in range(4)] + [256 + 48 * i for i in range(4)]
    return [bm // 8 * i for i in range(8)]


def seam_lines(h: int):
    """-> (rows, cols, pixels): the rows and columns, and the single pixels (row, column), next to a place where the tile kernel changes
    owner.
      rows    the frame borders and both sides of every row-tile seam (every ROUT rows: 7 @ 56, 14 @ 28, 4 @ 64, 8 @ 32; none inside the
              whole-frame tiles of 16 / 14 / 7)
      cols    the frame borders (columns 0 and W - 1 sit next to the materialised padding slots 0 and W + 1 of a tile row)
      pixels  per tile (first output row r0; its phase-A rows start at image row max(r0 - 1, 0) and are flattened m = row * W + column):
              the last pixel of one wave's share and the first of the next (``wave_starts``, for every BM the map size runs with);
              and per tile the output slots srel = (row - r0) (W + 2) + column + 1 on both sides of every multiple of 16 - the 16-slot
              fragments of phase B - where that slot is a pixel and not padding"""
    r, w = rout(h), h
    rows, cols, px = {0, h - 1}, {0, w - 1}, set()
    for y in range(r, h, r):
        rows |= {y - 1, y}
    for r0 in range(0, h, r):
        rlo, rhi = max(r0 - 1, 0), min(r0 + r + 1, h)
        ma = (rhi - rlo) * w
        for bm in BMS[h]:
            for m0 in wave_starts(h, bm):
                for m in (m0 - 1, m0):
                    if 0 < m0 < ma and 0 <= m < ma:
                        px.add((rlo + m // w, m % w))
        for s16 in range(16, r * (w + 2), 16):
            for s in (s16 - 1, s16):
                rr, xs = divmod(s, w + 2)
                if 1 <= xs <= w and rr < r:
                    px.add((r0 + rr, xs - 1))
    return sorted(rows), sorted(cols), sorted(px)


def seam_mask(h: int):
    rows, cols, px = seam_lines(h)
    m = np.zeros((h, h), bool)
    m[rows, :] = True
    m[:, cols] = True
    for r, c in px:
        m[r, c] = True
    return m


# ---- reference and bound ------------------------------------------------------------------------------------------------------------
def is_exact(inp) -> bool:
    return "w1_lo" in inp


def reference(inp, h=None, bound=True):
    """inputs of one layer -> (y, E): the float64 output (B,H,W,32) and its componentwise bound (None with bound=False).  h: the map size
    whose BK pads the exact mode's K (default: the input's own)"""
    x = inp["x"].astype(np.float64)
    k = x.shape[-1]
    h = x.shape[1] if h is None else h
    ex = is_exact(inp)
    a1 = np.clip(x, inp["lo"].astype(np.float64), inp["hi"].astype(np.float64))
    w1 = inp["w1"].astype(np.float64)
    w1a = np.abs(w1)
    w3 = inp["w3"].astype(np.float64)
    w3a = np.abs(w3)
    if ex:
        w1a = w1a + np.abs(inp["w1_lo"].astype(np.float64))
        w1 = w1 + inp["w1_lo"].astype(np.float64)
        w3a = w3a + np.abs(inp["w3_lo"].astype(np.float64))
        w3 = w3 + inp["w3_lo"].astype(np.float64)
    n = 2 * kp_of(h, k) if ex else k
    n3 = 2304 if ex else 1152
    s2, t2 = inp["s2"].astype(np.float64), inp["t2"].astype(np.float64)
    bott = a1 @ w1.T
    z = bott * s2 + t2
    a2 = np.maximum(z, 0.0)
    y = _conv3x3(a2, w3)
    if not bound:
        return y, None
    db = (n + 16) * E32 * (np.abs(a1) @ w1a.T)
    dz = np.abs(s2) * db * (1.0 + E32) + E32 * np.abs(z)
    da = U16 * (a2 + dz) + dz + 2.0 ** -25
    through = _conv3x3(da + (n3 + 16) * E32 * (a2 + da), w3a)
    return y, U16 * np.abs(y) + (1.0 + U16) * through + 2.0 ** -25


# ---- the fp32 model of the kernel's arithmetic --------------------------------------------------------------------------------------
def model(inp, h=None, drop_tap=None, drop_k=None, seam_row=None, pad_col=None, edge_row=None, no_wrap=None):
    """-> (B,H,W,32) float32 holding fp16 numbers: what a kernel that does the defined arithmetic in the kernel's precision stores.

    One defect at a time:
      drop_tap = (o, c, dy, dx[, half])  that product is missing from output channel o (exact mode: of image half 0 = hi, 1 = lo)
      drop_k = k                 input channel k of the 1x1 (exact mode: of its hi half) is missing
      seam_row = r               the 3x3 of output row r sees, as the bottleneck row above it, row r instead of row r - 1 (the halo row
                                 above a row-tile seam taken from the wrong side)
      pad_col = 0 | 1            a padding column (slot 0 / slot W + 1 of a tile row) holds the neighbouring column's bottleneck, not zeros
      edge_row = 0 | 1           the tile row above the first / below the last image row (top_pad / last tile) holds that image row's
                                 bottleneck, not zeros
      no_wrap = behind           exact mode: the lo pass reads its activations from channel Kp onward instead of wrapping to channel 0;
                                 behind (B,H,W,K) is what the buffer holds in channels [Kp, Kp + K)"""
    x = inp["x"].astype(np.float32)
    b, hh, w, k = x.shape
    h = hh if h is None else h
    ex = is_exact(inp)
    a1 = np.clip(x, inp["lo"], inp["hi"]).astype(np.float32)
    w1 = inp["w1"].astype(np.float32)
    if drop_k is not None:
        w1 = w1.copy()
        w1[:, drop_k] = 0.0
    acc = np.zeros((b, hh, w, 128), np.float32)
    passes = [(a1, w1)]
    if ex:
        a1_lo = a1 if no_wrap is None else np.clip(no_wrap.astype(np.float32), inp["lo"], inp["hi"]).astype(np.float32)
        passes.append((a1_lo, inp["w1_lo"].astype(np.float32)))
    else:
        assert no_wrap is None
    for av, wv in passes:                                      # exact mode: the hi pass, then the lo pass
        for q in range(k // 32):                               # one 32-channel k-step per MFMA
            acc += av[..., 32 * q:32 * q + 32] @ wv[:, 32 * q:32 * q + 32].T
    z = (acc.astype(np.float64) * inp["s2"].astype(np.float64) + inp["t2"].astype(np.float64)).astype(np.float32)   # the fma: one rounding
    a2 = np.maximum(_h(z), np.float32(0.0))
    w3s = [inp["w3"].astype(np.float32)] + ([inp["w3_lo"].astype(np.float32)] if ex else [])
    if drop_tap is not None:
        o, c, dy, dx = drop_tap[:4]
        half = drop_tap[4] if len(drop_tap) > 4 else 0
        w3s[half] = w3s[half].copy()
        w3s[half][o, c, dy, dx] = 0.0
    p = np.zeros((b, hh + 2, w + 2, 128), np.float32)
    p[:, 1:-1, 1:-1] = a2
    if pad_col is not None:
        if pad_col == 0:
            p[:, 1:-1, 0] = a2[:, :, 0]
        else:
            p[:, 1:-1, w + 1] = a2[:, :, w - 1]
    if edge_row is not None:
        if edge_row == 0:
            p[:, 0, 1:-1] = a2[:, 0]
        else:
            p[:, hh + 1, 1:-1] = a2[:, hh - 1]
    y = np.zeros((b, hh, w, 32), np.float32)
    for w3 in w3s:                                             # one accumulator per output: nine taps (exact: and nine more)
        for dy in range(3):
            for dx in range(3):
                rows = p[:, dy:dy + hh, dx:dx + w]
                if seam_row is not None and dy == 0:
                    rows = rows.copy()
                    rows[:, seam_row] = p[:, seam_row + 1, dx:dx + w]
                for t in range(4):
                    y += rows[..., 32 * t:32 * t + 32] @ w3[:, 32 * t:32 * t + 32, dy, dx].T
    return _h(y)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def split_hi_lo(w):
    """fp32 -> (hi, lo) fp16 numbers as float32: hi = fp16(w), lo = fp16(w - hi)"""
    w = np.asarray(w, np.float32)
    hi = _h(w)
    return hi, _h((w - hi).astype(np.float32))


def noisy_params(rng, k: int, exact: bool):
    """one layer's parameters in the distribution of tests/test_gpu_kernels.py::test_dense_layer_fused (clamp constants of all three kinds)"""
    lo, hi = clamp_consts(rng, k)
    w1 = rng.normal(0, np.sqrt(2.0 / k), (128, k)).astype(np.float32)
    w3 = rng.normal(0, np.sqrt(2.0 / 1152), (32, 128, 3, 3)).astype(np.float32)
    d = dict(lo=lo, hi=hi, s2=rng.uniform(0.5, 1.5, 128).astype(np.float32), t2=rng.normal(0, 0.3, 128).astype(np.float32))
    if exact:
        d["w1"], d["w1_lo"] = split_hi_lo(w1)
        d["w3"], d["w3_lo"] = split_hi_lo(w3)
    else:
        d["w1"], d["w3"] = _h(w1), _h(w3)
    return d


def noisy_x(rng, h: int, k: int, b: int):
    x = rng.normal(0, 1.5, (b, h, h, k)).astype(np.float32)
    big = (rng.uniform(20.0, 60.0, x.shape) * np.where(rng.random(x.shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    m = seam_mask(h)
    x[:, m] = big[:, m]
    return x.astype(np.float16)


def noisy(h: int, k: int, b: int, seed: int, exact: bool = False):
    """Gaussian activations and weights with |x| in [20, 60] of random sign planted, in every channel, wherever ``seam_lines`` says the
    kernel changes owner: a halo row taken from the wrong tile, a padding slot that is not zero or a fragment handed to the wrong wave is
    an O(1) error there.  -> dict(x (B,H,H,K) fp16, lo, hi, w1 (128,K), s2, t2, w3 (32,128,3,3) [, w1_lo, w3_lo]; fp32, weights fp16-valued)"""
    rng = np.random.default_rng([seed, h, k, b, int(exact)])
    x = noisy_x(rng, h, k, b)
    return dict(x=x, **noisy_params(rng, k, exact))


def _sparse_rows(rng, k, count, stride):
    w1 = np.zeros((128, k), np.float32)
    for n in range(128):
        w1[n, (stride * n + np.arange(count)) % k] = rng.permutation(np.repeat([-1.0, 1.0], count // 2))     # balanced: no dead channel
    return w1


def _w3_map(rng, lo_map: bool):
    w3 = np.zeros((32, 128, 3, 3), np.float32)
    sign = rng.choice([-1.0, 1.0], (3, 3, 128))
    dy, dx, c = np.meshgrid(np.arange(3), np.arange(3), np.arange(128), indexing="ij")
    p = 128 * (3 * dy + dx) + c
    w3[(p + p // 32) % 32 if lo_map else p % 32, c, dy, dx] = sign
    return w3


def integer_params(rng, k: int, exact: bool, unit_clamp_from=None):
    """one layer's parameters of the `integer` cases; unit_clamp_from = c: channels >= c are clamped to [0, 1] (chains)"""
    lo, hi = np.zeros(k, np.float32), np.full(k, F16_MAX, np.float32)
    if unit_clamp_from is not None:
        hi[unit_clamp_from:] = 1.0
    d = dict(lo=lo, hi=hi, s2=np.ones(128, np.float32), w1=_sparse_rows(rng, k, 16, 11), w3=_w3_map(rng, False))
    if exact:
        d["w1_lo"] = _sparse_rows(rng, k, 8, 7)
        d["w3_lo"] = _w3_map(rng, True)
        d["t2"] = rng.integers(-2, 5, 128).astype(np.float32)
    else:
        d["t2"] = rng.integers(-2, 9, 128).astype(np.float32)
    return d


def integer(h: int, k: int, b: int, seed: int, exact: bool = False):
    """Every value exact at every rounding: x in {0, 1} behind a clamp that passes it, s2 = 1, integer t2.
    Every row of w1 has as many +1 as -1 and t2 >= -2, so that no bottleneck channel is dead behind the ReLU (bott has mean t2 and a
    standard deviation of 2 ... 2.5): a product missing anywhere changes some output.
    Non-exact: as strip_ref.integer - w1 in {-1, 0, 1} with 16 non-zeros per row (a run from 11 n mod K), t2 in [-2, 8] (|bott| <= 24),
    every (tap, channel) position p = 128 tap + c non-zero in output channel p mod 32 alone: |y| <= 36 * 24 = 864.
    Exact: the kernel's contract is that it is handed two fp16 arrays and sums both, so hi and lo get INDEPENDENT patterns - w1 hi as
    above, w1 lo 8 non-zeros per row (a run from 7 n mod K), t2 in [-2, 4] (|bott| <= 28); w3 hi as above, w3 lo with position p in
    output channel (p + p // 32) mod 32: 72 non-zeros per output, |y| <= 72 * 28 = 2016 < 2048."""
    rng = np.random.default_rng([seed, h, k, b, 1, int(exact)])
    x = rng.integers(0, 2, (b, h, h, k)).astype(np.float16)
    return dict(x=x, **integer_params(rng, k, exact))


def chain_integer(h: int, k0: int, n: int, b: int, seed: int, exact: bool = False):
    """-> (x (B,H,H,K0) fp16 in {0, 1}, [layer parameters] * n): as ``integer`` with clamp constants lo = 0, hi = 1 on every channel a
    layer of the chain produces, so each layer sees {0, 1} again and the whole chain is exact"""
    rng = np.random.default_rng([seed, h, k0, n, b, 2, int(exact)])
    x = rng.integers(0, 2, (b, h, h, k0)).astype(np.float16)
    return x, [integer_params(rng, k0 + 32 * l, exact, unit_clamp_from=k0) for l in range(n)]


def chain_noisy(h: int, k0: int, n: int, b: int, seed: int, exact: bool = False):
    """-> (x, [layer parameters] * n): ``noisy`` activations and n layers' parameters"""
    rng = np.random.default_rng([seed, h, k0, n, b, 3, int(exact)])
    x = noisy_x(rng, h, k0, b)
    return x, [noisy_params(rng, k0 + 32 * l, exact) for l in range(n)]


def chain_reference(x, layers):
    """float64 chain on the `chain_integer` inputs (exact, so the stored fp16 outputs are the float64 ones) -> (B,H,H,K0 + 32 n)"""
    buf = x.astype(np.float64)
    for p in layers:
        y, _ = reference(dict(x=buf, **p), h=x.shape[1], bound=False)
        buf = np.concatenate([buf, y], axis=-1)
    return buf


# ---- the instantiations -------------------------------------------------------------------------------------------------------------
EXACT = 1 << 17


def single_ks(h: int, exact: bool):
    """the K of a single-layer instantiation: every K with 1, 2, 3 or 4 k-tiles, a mid-range K % 64 == 0 and one K % 64 == 32 (at
    BK = 64 the dead half-stage - in exact mode in the middle of the loop), KMAX - 32 and KMAX"""
    bk, km = bk_of(h), kmax(h)
    ks = set(range(32, 4 * bk + 1, 32)) | {km - 32, km}
    ks |= {160, 192} if km == 256 else {km // 2 + 64, km // 2 + 96}
    return sorted(ks)


def chain_min_k0(h: int, variant: int, exact: bool) -> int:
    """the smallest K0 launch_dense_layer_big accepts for a chain of two or more layers: the k-tiles the kernel requests ahead for the
    next layer - two, three with the software-pipelined loop of 7 x 7 (PP 4) - go out before the current layer's output is stored, so
    they have to lie inside the channels the current layer read: primed * BK <= K0"""
    pp4 = h == 7 and not exact and not (variant & (32 | 512))
    return (3 if pp4 else 2) * bk_of(h)


def chain_shapes(h: int, variant: int, exact: bool):
    """(K0, n): the network's own chain of that map, a short chain ending at KMAX - 32, a chain that crosses the small k-tile counts from
    the smallest K0 accepted"""
    net = {14: (256, 24), 16: (512, 16), 7: (512, 16)}[h]
    return [net, (960, 2), (chain_min_k0(h, variant, exact), 6)]


def _inst():
    rows = []
    single = {56: (56, 7, 512, 32), 28: (28, 14, 512, 32), 14: (14, 14, 256, 64), 64: (64, 4, 384, 32), 32: (32, 8, 384, 32), 16: (16, 16, 384, 32)}
    for h, g in single.items():
        rows.append(dict(h=h, variant=0, exact=False, chained=False, targs=g + (2, False, False)))
        rows.append(dict(h=h, variant=8, exact=False, chained=False, targs=g + (0, False, False)))
        rows.append(dict(h=h, variant=0, exact=True, chained=False, targs=g + (2, False, True)))
    rows += [dict(h=7, variant=0, exact=False, chained=False, targs=(7, 7, 64, 64, 4, False, False)),
             dict(h=7, variant=512, exact=False, chained=False, targs=(7, 7, 128, 64, 2, False, False)),
             dict(h=7, variant=512 | 8, exact=False, chained=False, targs=(7, 7, 128, 64, 0, False, False)),
             dict(h=7, variant=0, exact=True, chained=False, targs=(7, 7, 128, 64, 2, False, True)),
             dict(h=14, variant=0, exact=False, chained=True, targs=(14, 14, 256, 64, 2, True, False)),
             dict(h=16, variant=0, exact=False, chained=True, targs=(16, 16, 384, 32, 2, True, False)),
             dict(h=7, variant=0, exact=False, chained=True, targs=(7, 7, 64, 64, 4, True, False)),
             dict(h=7, variant=512, exact=False, chained=True, targs=(7, 7, 64, 64, 2, True, False)),
             dict(h=7, variant=32, exact=False, chained=True, targs=(7, 7, 128, 64, 2, True, False)),
             dict(h=14, variant=0, exact=True, chained=True, targs=(14, 14, 256, 64, 2, True, True)),
             dict(h=16, variant=0, exact=True, chained=True, targs=(16, 16, 384, 32, 2, True, True)),
             dict(h=7, variant=0, exact=True, chained=True, targs=(7, 7, 64, 64, 2, True, True))]
    for r in rows:
        r["ks"] = chain_shapes(r["h"], r["variant"], r["exact"]) if r["chained"] else single_ks(r["h"], r["exact"])
        r["id"] = "%d%s%s-v%d" % (r["h"], "-chain" if r["chained"] else "", "-exact" if r["exact"] else "", r["variant"])
    return rows


INSTANTIATIONS = _inst()
assert len(INSTANTIATIONS) == 30 and len({r["targs"] for r in INSTANTIATIONS}) == 30


# ---- the concat buffer of a case ----------------------------------------------------------------------------------------------------
SENTINEL = np.float16(300.0)       # behind the output channels: never read by a correct kernel's arithmetic, never written
STALE = np.float16(-77.0)          # in the output channels: has to be overwritten


def buffer(x, ldc: int, nout: int = 32):
    """(B,H,H,K) fp16 -> the (B,H,H,ldc) concat buffer: input | STALE where the nout output channels go | SENTINEL"""
    k = x.shape[-1]
    buf = np.full(x.shape[:3] + (ldc,), SENTINEL, np.float16)
    buf[..., :k] = x
    buf[..., k:k + nout] = STALE
    return buf


def behind(buf, kp: int, k: int):
    """what a read of K channels from channel Kp onward finds at every pixel of the buffer (running on into the next pixel's row where
    the pitch ends; zeros behind the last pixel): the operand of ``model``'s no_wrap defect"""
    flat = np.concatenate([buf.reshape(-1), np.zeros(kp + k, buf.dtype)])
    ldc = buf.shape[-1]
    idx = (np.arange(buf.size // ldc) * ldc + kp)[:, None] + np.arange(k)[None, :]
    return flat[idx].reshape(buf.shape[:3] + (k,))
