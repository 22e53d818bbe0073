"""Float64 reference of one layer of a dense block as the three WHOLE-BLOCK kernels define it (csrc/dense_block7.hip, dense_block14.hip,
dense_block28.hip), the componentwise bound the device is held to, an fp32 model of each kernel's arithmetic with one defect at a time,
the input generators and the shape lists with the reason for every row - numpy only, built on tests/tools/strip_ref.py and tile_ref.py.

``reference``: the operands as tn_dbg_block{7,14,28}_create folds them; everything in float64 unless stated:

    a1    = clip(x, lo, hi)                                  exact: no arithmetic
    w1h   = float16(float32(w1) * float32(s2))               the fold of *_create, rounded by the packers (strip_ref.folded_weights)
    t_eff = float16(t2) + float16(t2 - float16(t2))          14 x 14, 28 x 28: the two halves of the shift k-step (StreamWriter::put_shift)
          = t2                                               7 x 7: the fp32 shift added on the reduced tile (pack_block7: tab)
    bott  = a1 @ w1h.T + t_eff
    a2    = relu(bott)
    y     = conv3x3(a2, w3), zero padding behind the activation; w3 holds fp16 numbers

The device rounds a2 and y to fp16 once each; the reference rounds neither and restates nothing of units, rings, tiles, wave splits or
channel permutations.  A block is judged layer by layer from the device's own final buffer: layer l reads channels [0, K_l) as the
device left them and its output is compared with channels [K_l, K_l + 32).

``E``, derived, not measured.  u = 2^-11, e = 2^-24; any summation order of n terms in fp32 is within (n - 1) e sum |terms|:

    db(p, c) = (n1 + 16) e (sum_k |a1| |w1h| + |t_eff|)
        7 x 7    n1 = K + 1: K products in four per-wave partial sums (the K ranges of pack_block7), the three fp32 additions of the LDS
                 reduction and the fp32 addition of t2 - one summation tree over K + 1 terms
        14 x 14  n1 = 64 ceil((K - 32) / 64) + 32 + 16: the super-steps from memory INCLUDING the zero-weighted pad half of a clipped last
                 one, the two forwarded k-steps of the tail, the shift k-step (16 wide: shift_hi, shift_lo, mask and 13 zeros)
        28 x 28  n1 = 64 ceil(K / 64) + 16: the shift k-step first, then the super-steps including the pad
        and 16 terms of room each for the chained MFMAs' own accumulator additions and |shift_hi| + |shift_lo| <= (1 + 2^-10) |t_eff|
    da(p, c) = u (a2 + db) + db + 2^-25                      ReLU is 1-Lipschitz; one rounding to fp16; 2^-25: half an fp16 subnormal step
    E(p, o)  = u |y| + (1 + u) [sum_{tap, c} |w3| da + n3 e sum |w3| (a2 + da)] + 2^-25
        14 x 14, 28 x 28   n3 = 1152 + 3: three column accumulators of 384 products, added last by the two DPP shifts
        7 x 7              n3 = 1152 + 4: four per-wave partial sums of 288 products, added to a zero in fp32 through LDS

The statistic is max |y_dev - y| / E <= 1.

Outside the bound's reach (listed, not worked around): on real-valued inputs a single missing product of an average weight; the low
half of the shift (|shift_lo| <= 2^-11 |t2| is below u a2 wherever the ReLU passes the value); a rounding of a2 or y other than to
nearest that stays within u.  The `chain_integer` inputs see the first; nothing here sees the other two.

``model`` is an fp32 restatement of each kernel's arithmetic - float32 accumulation k-step by k-step in the kernel's split, the two fp16
roundings, the partial sums added last in the kernel's order - with one defect at a time (tests/test_cpu_block_ref.py)."""
from __future__ import annotations

import numpy as np

from .strip_ref import E32, F16_MAX, U16, _conv3x3, _h, folded_weights, ratio, shift_halves  # noqa: F401
from .tile_ref import SENTINEL, STALE, _sparse_rows, buffer, noisy_params  # noqa: F401  (same operand definitions)

SIZES = (7, 14, 28)
BATCH = {7: 3, 14: 2, 28: 2}
RING7 = 6          # dense_block7.hip: kRingDepth
NR = 5             # dense_stream.h: kNR, slots of the unit ring
MIN_K0 = {7: 64 * (RING7 + 1), 14: 256, 28: 128}


# ---- what the launchers accept --------------------------------------------------------------------------------------------------
def supported(h: int, k0: int, nl: int) -> bool:
    """dense_block{7,14,28}_supported restated"""
    if k0 % 32 or nl < 1 or k0 < MIN_K0[h]:
        return False
    if h == 28:
        return k0 + 32 * (nl - 1) <= 512          # K of the last layer; kPlanes = 36 holds its output and the pad
    return k0 + 32 * nl <= 1024                   # 7 x 7: the LDS-resident concat buffer; 14 x 14: kScrChannels, the frame's scratch


def launchable(h: int, k0: int, nl: int, ldc: int, b: int) -> bool:
    return supported(h, k0, nl) and ldc % (8 if h == 7 else 64) == 0 and k0 + 32 * nl <= ldc and b > 0


def max_nl(h: int, k0: int) -> int:
    return (512 - k0) // 32 + 1 if h == 28 else (1024 - k0) // 32


def accepted_k0(h: int):
    return [k for k in range(MIN_K0[h], 1025, 32) if supported(h, k, 1)]


def smallest_ldc(h: int, k0: int, nl: int) -> int:
    """K0 + 32 nl rounded up to 64; at 7 x 7 to 8 (which it already is a multiple of)"""
    end = k0 + 32 * nl
    return end if h == 7 else (end + 63) // 64 * 64


def case_ldc(h: int, k0: int, nl: int) -> int:
    """the smallest legal pitch in half of the cases (odd K0 / 32), 64 more in the others"""
    return smallest_ldc(h, k0, nl) + (0 if (k0 // 32) % 2 else 64)


# ---- the loop structure restated from the packers (for the coverage argument) ------------------------------------------------------
def wave_ranges7(k: int):
    """pack_block7: G = K / 16 k-steps split over the four waves -> [(g0, nA)] * 4"""
    g = k // 16
    gbase, grem = divmod(g, 4)
    return [(w * gbase + min(w, grem), gbase + (1 if w < grem else 0)) for w in range(4)]


def tail_variant7(na: int) -> int:
    """dense_block7_kernel: which of the RING7 straight-line tails ends a wave's K loop of nA steps"""
    b = 0
    while b + 2 * RING7 + 1 <= na:
        b += RING7
    return na - 1 - b - RING7


def nsu(h: int, k: int) -> int:
    """super-step units of one layer (one pass at 28 x 28): 14 x 14 reads K - 32 channels from memory, 28 x 28 all K"""
    return (k - 32 + 63) // 64 if h == 14 else (k + 63) // 64


def clipped(h: int, k: int) -> bool:
    """the last super-step is half empty (zero weights and clamp constants over a pad half that is read from the scratch)"""
    return (k - 32 if h == 14 else k) % 64 == 32


def units(h: int, k0: int, nl: int) -> int:
    """dense_block14_units / dense_block28_units"""
    if h == 14:
        return 4 + sum(nsu(14, k0 + 32 * l) + 1 + 6 for l in range(nl))
    return 1 + 4 + sum(4 * (nsu(28, k0 + 32 * l) + 6) for l in range(nl))


def stage_starts(h: int, k0: int, nl: int):
    """[(layer, unit index at which the layer - at 28 x 28: each of its four passes - starts)]"""
    out, u = [], 0 if h == 14 else 1
    for l in range(nl):
        k = k0 + 32 * l
        for _ in range(1 if h == 14 else 4):
            out.append((l, u))
            u += nsu(h, k) + (7 if h == 14 else 6)
    assert u + 4 == units(h, k0, nl)
    return out


# ---- where a kernel changes owner ---------------------------------------------------------------------------------------------------
def seam_mask(h: int, wave_seams: bool = True):
    """(h, h) bool: the pixels next to a place where the kernel changes owner.
      7 x 7    the frame borders; pixels 31 | 32 (the two 32-slot pixel tiles of an MFMA's N) and pixel 48 (slots 49 - 63 are padding)
      14 x 14  the frame borders; rows 3 | 4, 7 | 8, 11 | 12 (wave w owns rows 4 w ... 4 w + 3); rows 12, 13 (wave 3's last real rows, next to
               rows 14 / 15 that do not exist); columns 0 and 13 (next to the padding slots 0 and 15)
      28 x 28  the frame borders; rows 7 | 8, 15 | 16, 23 | 24 (pass seams, which the rolling tile carries across); rows 26, 27 (next to rows
               28 - 31 that do not exist); columns 0 and 27 (next to slots 0 and 29 and the two slotless lanes); with wave_seams the row
               pairs 8 p + 2 w + 1 | 8 p + 2 w + 2 between the waves of a pass - together with the others that is EVERY row, so ``noisy``
               plants them in frame 0 only and keeps the contrast in the other frames"""
    m = np.zeros((h, h), bool)
    m[[0, h - 1], :] = True
    m[:, [0, h - 1]] = True
    if h == 7:
        for p in (31, 32, 48):
            m[p // 7, p % 7] = True
    elif h == 14:
        m[[3, 4, 7, 8, 11, 12, 13], :] = True
    else:
        m[[7, 8, 15, 16, 23, 24, 26, 27], :] = True
        if wave_seams:
            for p in range(4):
                for w in range(3):
                    m[[r for r in (8 * p + 2 * w + 1, 8 * p + 2 * w + 2) if r < h], :] = True
    return m


def channel_seams(h: int, k0: int, nl: int):
    """input channels (< K0) on both sides of a place where the K loop of the block's FIRST TWO layers changes owner (every K0 is a first
    layer in some row of the lists, so every position gets its turn; all 18 layers' seams would be a quarter of the channels):
      7 x 7    each wave's first k-step, channel 16 g0 (``wave_ranges7``)
      14 x 14  every 64-channel super-step boundary, and G = K - 32 where the tail takes over
      28 x 28  every 64-channel super-step boundary"""
    cs = set()
    for l in range(min(nl, 2)):
        k = k0 + 32 * l
        if h == 7:
            edges = [16 * g0 for g0, _ in wave_ranges7(k)[1:]]
        elif h == 14:
            edges = list(range(64, k - 32, 64)) + [k - 32]
        else:
            edges = list(range(64, k, 64))
        for c in edges:
            cs |= {c - 1, c}
    return sorted(c for c in cs if 0 <= c < k0)


# ---- reference and bound ------------------------------------------------------------------------------------------------------------
def t_eff(h: int, t2):
    if h == 7:
        return np.asarray(t2, np.float32).astype(np.float64)
    hi, lo = shift_halves(t2)
    return hi + lo


def term_counts(h: int, k: int):
    """(n1, n3) of the bound"""
    if h == 7:
        return k + 1, 1152 + 4
    if h == 14:
        return 64 * nsu(14, k) + 32 + 16, 1152 + 3
    return 64 * nsu(28, k) + 16, 1152 + 3


def reference(inp, h: int, bound: bool = True):
    """one layer's inputs (x (B,H,H,K) and the layer's parameters) -> (y, E) in float64; E is None with bound=False"""
    x = inp["x"].astype(np.float64)
    k = x.shape[-1]
    a1 = np.clip(x, inp["lo"].astype(np.float64), inp["hi"].astype(np.float64))
    w1h = folded_weights(inp["w1"], inp["s2"])
    t = t_eff(h, inp["t2"])
    bott = a1 @ w1h.T + t
    a2 = np.maximum(bott, 0.0)
    w3 = inp["w3"].astype(np.float64)
    y = _conv3x3(a2, w3)
    if not bound:
        return y, None
    n1, n3 = term_counts(h, k)
    db = (n1 + 16) * E32 * (np.abs(a1) @ np.abs(w1h).T + np.abs(t))
    da = U16 * (a2 + db) + db + 2.0 ** -25
    through = _conv3x3(da + n3 * E32 * (a2 + da), np.abs(w3))
    return y, U16 * np.abs(y) + (1.0 + U16) * through + 2.0 ** -25


def block_ratios(out, k0: int, layers, h: int):
    """the device's (or the model's) final buffer -> per layer max |y_dev - y| / E, each layer fed channels [0, K_l) of that buffer"""
    rs = []
    for l, p in enumerate(layers):
        k = k0 + 32 * l
        y, e = reference(dict(x=out[..., :k], **p), h)
        rs.append(float((np.abs(out[..., k:k + 32].astype(np.float64) - y) / e).max()))
    return rs


def chain_reference(x, layers, h: int):
    """float64 block on the `chain_integer` inputs (exact: the stored fp16 outputs are the float64 ones) -> (B,H,H,K0 + 32 nl)"""
    buf = x.astype(np.float64)
    for p in layers:
        y, _ = reference(dict(x=buf, **p), h, bound=False)
        buf = np.concatenate([buf, y], axis=-1)
    return buf


# ---- the fp32 model of each kernel's arithmetic -------------------------------------------------------------------------------------
def tail_order14(k: int):
    """the input channel of position (k-step ks, half hh, j) of the 14 x 14 tail unit: the order in which the previous layer's 3x3 leaves
    its 32 channels in registers (pack_block14: G + 16 (lane >> 5) + 8 ks + j)"""
    g = k - 32
    return [g + 16 * hh + 8 * ks + j for ks in range(2) for hh in range(2) for j in range(8)]


def model(inp, h: int, drop_tap=None, drop_k=None, drop_wave=None, seam_row=None, stale_row=None, pad_col=None, ghost_row=False,
          plain_forward=False, want_a2=False):
    """-> (B,H,H,32) float32 holding fp16 numbers (with want_a2: and the fp16 bottleneck (B,H,H,128)).

    One defect at a time:
      drop_tap = (o, c, dy, dx)  that 3x3 product is missing from output channel o
      drop_k = k                 input channel k of the 1x1 is missing
      drop_wave = w              7 x 7: wave w's K-range partial sum does not reach the reduction
      seam_row = r               the 3x3 of output row r sees, as the bottleneck row above it, row r instead of row r - 1 (14 x 14: the row
                                 above a wave seam taken from below it)
      stale_row = (r, prev)      28 x 28: bottleneck row r = 8 p - 1 as the pass that reads it from the rolling tile (output rows r and
                                 r + 1) finds it is still the previous layer's, prev (B,H,H,128)
      pad_col = 0 | 1            a padding column (left / right of the frame) holds the neighbouring column's bottleneck, not zeros
      ghost_row = True           the row below the frame (14 / 15 at 14 x 14, 28 ... 31 at 28 x 28, the zero slot at 7 x 7) holds what the
                                 unmasked lanes compute - the last real row's bottleneck - not zeros
      plain_forward = True       14 x 14: the tail's weights meet the forwarded channels in plain order G + 16 ks + 8 hh + j"""
    x = inp["x"].astype(np.float32)
    b, hh, w, k = x.shape
    assert hh == h and w == h
    a1 = np.clip(x, inp["lo"], inp["hi"]).astype(np.float32)
    w1h = folded_weights(inp["w1"], inp["s2"]).astype(np.float32)
    if drop_k is not None:
        w1h = w1h.copy()
        w1h[:, drop_k] = 0.0
    zero = lambda: np.zeros((b, hh, w, 128), np.float32)
    kstep = lambda acc, src, ch: acc + a1[..., src] @ w1h[:, ch].T        # one 16-channel MFMA k-step in float32
    if h == 7:
        parts = []
        for wv, (g0, na) in enumerate(wave_ranges7(k)):
            acc = zero()
            for g in range(g0, g0 + na):
                ch = slice(16 * g, 16 * g + 16)
                acc = kstep(acc, ch, ch)
            parts.append(zero() if drop_wave == wv else acc)
        acc = zero()
        for m in range(4):                                             # wave m keeps M-tile m: own + the rounds RD = 1, 2, 3 from wave (m - RD) & 3
            sl = slice(32 * m, 32 * m + 32)
            t = parts[m][..., sl]
            for rd in (1, 2, 3):
                t = t + parts[(m - rd) & 3][..., sl]
            acc[..., sl] = t
        acc = acc + np.asarray(inp["t2"], np.float32)
    else:
        hi, lo = (v.astype(np.float32) for v in shift_halves(inp["t2"]))
        shift = (hi + lo).astype(np.float32)                            # one MFMA: the two products are summed exactly, then rounded
        acc = zero()
        if h == 28:
            acc = acc + shift
        for q in range((k - 32 if h == 14 else k) // 16):
            ch = slice(16 * q, 16 * q + 16)
            acc = kstep(acc, ch, ch)
        if h == 14:
            order = tail_order14(k)
            for ks in range(2):
                ch = order[16 * ks:16 * ks + 16]
                src = list(range(k - 32 + 16 * ks, k - 16 + 16 * ks)) if plain_forward else ch
                acc = kstep(acc, src, ch)
            acc = acc + shift
    a2 = _h(np.maximum(acc, np.float32(0.0)))
    w3 = inp["w3"].astype(np.float32)
    if drop_tap is not None:
        o, c, dy, dx = drop_tap
        w3 = w3.copy()
        w3[o, c, dy, dx] = 0.0

    def padded(a):
        p = np.zeros((b, hh + 2, w + 2, 128), np.float32)
        p[:, 1:-1, 1:-1] = a
        if pad_col == 0:
            p[:, 1:-1, 0] = a[:, :, 0]
        elif pad_col == 1:
            p[:, 1:-1, w + 1] = a[:, :, w - 1]
        if ghost_row:
            p[:, hh + 1, 1:-1] = a[:, hh - 1]
        return p

    def conv(p):
        def taps(dy, dx):
            rows = p[:, dy:dy + hh, dx:dx + w]
            if seam_row is not None and dy == 0:
                rows = rows.copy()
                rows[:, seam_row] = p[:, seam_row + 1, dx:dx + w]
            return rows
        if h == 7:                                                     # wave wv: its own 32 bottleneck channels, all nine taps, two k-steps each
            y = np.zeros((b, hh, w, 32), np.float32)
            for wv in range(4):
                q = np.zeros((b, hh, w, 32), np.float32)
                for tap in range(9):
                    rows = taps(tap // 3, tap % 3)
                    for s in range(2):
                        ch = slice(32 * wv + 16 * s, 32 * wv + 16 * s + 16)
                        q = q + rows[..., ch] @ w3[:, ch, tap // 3, tap % 3].T
                y = y + q
            return _h(y)
        cols = []
        for dx in range(3):                                            # one accumulator per kernel column, kernel rows in the kernel's order
            c3 = np.zeros((b, hh, w, 32), np.float32)
            for dy in ((1, 0, 2) if h == 14 else (2, 1, 0)):
                rows = taps(dy, dx)
                for t in range(8):
                    ch = slice(16 * t, 16 * t + 16)
                    c3 = c3 + rows[..., ch] @ w3[:, ch, dy, dx].T
            cols.append(c3)
        return _h((cols[1] + cols[0]) + cols[2])

    y = conv(padded(a2))
    if stale_row is not None:
        r, prev = stale_row
        a2s = a2.copy()
        a2s[:, r] = prev[:, r]
        ys = conv(padded(a2s))
        y[:, [r, r + 1]] = ys[:, [r, r + 1]]
    return (y, a2) if want_a2 else y


def model_block(x, layers, h: int, defect_layer=None, **defect):
    """the model over a whole block -> the (B,H,H,K0 + 32 nl) float32 buffer of fp16 numbers; a defect is applied in `defect_layer` only"""
    buf = x.astype(np.float32)
    for l, p in enumerate(layers):
        y = model(dict(x=buf.astype(np.float16), **p), h, **(defect if l == defect_layer else {}))
        buf = np.concatenate([buf, y], axis=-1)
    return buf


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
def noisy(h: int, k0: int, nl: int, b: int, seed: int):
    """-> (x (B,H,H,K0) fp16, [layer parameters] * nl): the distribution of tests/test_gpu_kernels.py::test_dense_block* (Gaussian
    activations and weights, clamp constants of all three kinds) with |x| in [20, 60] of random sign planted in every one of the K0 input
    channels at the pixels of ``seam_mask``, and at every pixel in the channels of ``channel_seams``: a row, slot, wave's partial sum or
    ring slot handed to the wrong owner is an O(1) error there.  28 x 28: the wave seams inside a pass in frame 0 only (``seam_mask``)."""
    rng = np.random.default_rng([seed, h, k0, nl, b, 3])
    x = rng.normal(0, 1.5, (b, h, h, k0)).astype(np.float32)
    big = (rng.uniform(20.0, 60.0, x.shape) * np.where(rng.random(x.shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    for f in range(b):
        m = seam_mask(h, wave_seams=(f == 0))
        x[f][m] = big[f][m]
    cs = channel_seams(h, k0, nl)
    x[..., cs] = big[..., cs]
    return x.astype(np.float16), [noisy_params(rng, k0 + 32 * l, False) for l in range(nl)]


def _w3_balanced(rng, t2):
    """w3 in {-1, 0, 1}: position p = 128 tap + c non-zero in output channel p mod 32 alone (tile_ref's map).  The signs of the 36
    positions of an output channel alternate along the positions sorted by t2[c] (random ties and start): as many +1 as -1, and the
    mean of the output - sum sign * mean a2[c], a2[c] having a mean near max(t2[c], 0) - within a few units of 0 where its standard
    deviation is about 12.  tile_ref draws the signs independently; an output channel whose mean comes out at -40 is negative at every
    pixel, behind the next layer's clamp to [0, 1] a dead input, and a product dropped or mis-permuted there changes nothing."""
    w3 = np.zeros((32, 128, 3, 3), np.float32)
    dy, dx, c = (v.ravel() for v in np.meshgrid(np.arange(3), np.arange(3), np.arange(128), indexing="ij"))
    p = 128 * (3 * dy + dx) + c
    for o in range(32):
        idx = np.flatnonzero(p % 32 == o)
        order = idx[np.lexsort((rng.random(idx.size), t2[c[idx]]))]
        sign = np.where(np.arange(order.size) % 2 == int(rng.integers(2)), 1.0, -1.0)
        w3[o, c[order], dy[order], dx[order]] = sign
    return w3


def integer_block(h: int, k0: int, nl: int, b: int, seed: int):
    """`chain_integer`: -> (x (B,H,H,K0) fp16 in {0, 1}, [layer parameters] * nl).  s2 = 1, integer t2 in [-2, 8] (the low half of the
    shift is 0), w1 in {-1, 0, 1} with the sparsity of tile_ref.integer_params (16 non-zeros per row, a run from 11 n mod K, as many +1 as
    -1), every (tap, channel) position of w3 in exactly one output channel with signs that centre the output (``_w3_balanced``), clamp constants lo = 0,
    hi = 65504 on the K0 input channels and hi = 1 on every channel the block produces: every layer sees {0, 1} again, |bott| <= 24,
    |y| <= 36 * 24 = 864 < 2048, so every rounding of every layer is exact and the device has to return the integers bit for bit"""
    rng = np.random.default_rng([seed, h, k0, nl, 2])          # (frame 0 and the parameters do not depend on B)
    x = np.stack([np.random.default_rng([seed, h, k0, nl, 2, f]).integers(0, 2, (h, h, k0)) for f in range(b)]).astype(np.float16)
    layers = []
    for l in range(nl):
        k = k0 + 32 * l
        hi = np.full(k, F16_MAX, np.float32)
        hi[k0:] = 1.0
        t2 = rng.integers(-2, 9, 128).astype(np.float32)
        layers.append(dict(lo=np.zeros(k, np.float32), hi=hi, s2=np.ones(128, np.float32), t2=t2, w1=_sparse_rows(rng, k, 16, 11), w3=_w3_balanced(rng, t2)))
    return x, layers


def dirty(h: int, k0: int, b: int, seed: int):
    """(B,H,H,K0) fp16 of large finite values, +-Inf and NaN among ordinary ones: what a launch may leave behind in the scratch"""
    rng = np.random.default_rng([seed, h, k0, b, 5])
    x = rng.normal(0, 1.5, (b, h, h, k0)).astype(np.float32)
    kind = rng.random(x.shape)
    x[kind < 0.30] = 60000.0
    x[kind < 0.22] = -60000.0
    x[kind < 0.15] = np.inf
    x[kind < 0.10] = -np.inf
    x[kind < 0.05] = np.nan
    return x.astype(np.float16)


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
def required_rows(h: int):
    """the rows a list has to hold, restated from the rule (not from the list): [(K0, nl, reason)]"""
    ks = accepted_k0(h)
    rows = [(k, min(2, max_nl(h, k)), "K0 = %d as a FIRST layer behind the prologue's ring fill, then a real next layer%s" % (
        k, "" if max_nl(h, k) >= 2 else " (nl = 1: the last K0 has none)")) for k in ks]
    if h == 7:
        rows += [(448, 18, "every K the kernel accepts in one launch: every tail variant as an inner layer"), (512, 16, "the network's own block (224 x 224 input)")]
    elif h == 14:
        rows += [(256, 24, "the network's block of a 224 x 224 input"), (512, 16, "the network's block of a 448 x 448 input"),
                 (256, 1, "a block of one layer: the refills of a next layer that does not exist")]
    else:
        rows += [(128, 12, "the network's block (224 x 224 input)"), (128, 13, "every K the kernel accepts in one launch")]
    return rows


_FIRST7 = "first layer: the prologue's six-step ring fill, this K0's tail variants, then a real next layer (the last layer's zero-step refill)"
_FIRST = "first layer: the prologue's copy and ring fill at this K0's super-step count and ring parity, then a real next layer"
SHAPES = {  # h: [(K0, nl, why this row)]
    7: [(k, 2, _FIRST7) for k in range(448, 961, 32)] + [
        (992, 1, "the last K0: first and last layer at once"),
        (448, 18, "every K the kernel accepts in one launch: every tail variant as an inner layer"),
        (512, 16, "the network's own block")],
    14: [(k, 2, _FIRST) for k in range(256, 961, 32)] + [
        (992, 1, "the last K0: first and last layer at once, the highest scratch planes"),
        (256, 24, "the network's block of a 224 x 224 input: every ring-slot residue at a layer start"),
        (512, 16, "the network's block of a 448 x 448 input"),
        (256, 1, "a block of one layer: the refills of a next layer that does not exist")],
    28: [(k, 2, _FIRST) for k in range(128, 481, 32)] + [
        (512, 1, "the last K0: first and last layer at once"),
        (128, 12, "the network's block: two-super-step layers, where the ring wraps through two passes"),
        (128, 13, "every K the kernel accepts in one launch")],
}


def roles(nl: int, l: int):
    return {"first"} if l == 0 and nl > 1 else {"last"} if l == nl - 1 and nl > 1 else {"first", "last"} if nl == 1 else {"inner"}


def coverage_problems(h: int, shapes):
    """what a shape list [(K0, nl, ...)] leaves uncovered -> list of sentences (empty: covered)"""
    rows = [(r[0], r[1]) for r in shapes]
    bad = ["refused by the launcher: K0 = %d, nl = %d" % r for r in rows if not supported(h, *r)]
    bad += ["missing row K0 = %d, nl = %d: %s" % r for r in required_rows(h) if r[:2] not in rows]
    layers = [(k0 + 32 * l, role) for k0, nl in rows for l in range(nl) for role in roles(nl, l)]
    if h == 7:
        seen = {(w, tail_variant7(wave_ranges7(k)[w][1]), role) for k, role in layers for w in (0, 3)}
        bad += ["tail variant r = %d of wave %d never runs as a %s layer" % (r, w, role) for w in (0, 3) for r in range(RING7) for role in ("first", "inner", "last")
                if (w, r, role) not in seen]
        rem = {((k // 16) % 4, role) for k, role in layers}
        bad += ["G %% 4 = %d never occurs in a %s layer" % (g, role) for g in (0, 2) for role in ("first", "inner", "last") if (g, role) not in rem]
        return bad
    seen = {(nsu(h, k0 + 32 * l) % 2, clipped(h, k0 + 32 * l), "first" if l == 0 else "inner") for k0, nl in rows for l in range(nl)}
    for par in (0, 1):
        for cl in (False, True):
            for role in ("first", "inner"):
                if (par, cl, role) not in seen:
                    bad.append("%s super-step count with a %s last super-step never runs as %s layer" % ("odd" if par else "even", "clipped" if cl else "full", role))
    res = {u % NR for k0, nl in rows for l, u in stage_starts(h, k0, nl)}
    bad += ["no layer starts at a unit index = %d mod %d" % (r, NR) for r in range(NR) if r not in res]
    return bad


# ---- what has to be refused ---------------------------------------------------------------------------------------------------------
def refusals(h: int):
    """[(K0, nl, ldc, B, what the message has to name)]: refused with nothing launched.  The first five fail the kernel's predicate
    (at *_create already), the last three its launcher."""
    k = MIN_K0[h]
    size = "%d x %d" % (h, h)
    g = lambda k0, nl: (size, "K0 = %d" % k0, "nl = %d" % nl)
    good = smallest_ldc(h, k, 2) if h == 7 else (k + 64 + 63) // 64 * 64
    rows = [(k - 32, 2, 1024, 1, g(k - 32, 2)),                          # below the kernel's minimum: 416, 224, 96
            (k + 16, 2, 1024, 1, g(k + 16, 2)),                          # K0 % 32 != 0
            (k, 0, 1024, 1, g(k, 0))]                                    # nl = 0
    if h == 28:
        rows += [(512, 2, 1024, 1, g(512, 2))]                           # the last layer's K = 544
    else:
        rows += [(992, 2, 1088, 1, g(992, 2))]                           # K0 + 32 nl = 1056
    if h == 14:
        rows += [(256, 56, 2048, 1, g(256, 56))]                         # K0 + 32 nl = 2048: what the predicate admitted before it was tied to the scratch
    rows += [(k, 2, good - 64, 1, g(k, 2) + ("ldc = %d" % (good - 64),)),                                   # ldc < K0 + 32 nl
             (k, 2, good + (4 if h == 7 else 32), 1, g(k, 2) + ("ldc = %d" % (good + (4 if h == 7 else 32)),)),   # ldc % 8 / % 64 != 0
             (k, 2, good, 0, g(k, 2) + ("B = 0",))]
    return rows
