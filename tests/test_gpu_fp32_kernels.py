"""-m gpu: the fp32 encoder mode's kernels (TN_ENC_FP32, csrc/dense_fp32.hip), every instantiation alone.

conv_fp32_kernel through tn_dbg_conv_fp32x3(which = 1) at tile selector 1 (small: <1X1,1,2>, <3X3,1,1>, <TRANS,1,2>), 2 (large:
<1X1,1,4>, <3X3,2,1>, <TRANS,1,4>) and 0 (the launcher's rule; the stem is <STEM,1,2> at every selector), against
oracle/fp32_chain_np.py: the kernel restated in exact fp32 steps, one fused multiply-add per k in ascending order.  Per case: rows
past M and columns outside the window keep the poison, no NaN (the activation's channels past K are NaN), the three tiles give the
same bits, THE BITS ARE THE CHAIN'S, and against float64 the device is within twice the chain's own worst error (both in units of
sum |a||b|, measured on the spot: docs/numerics.md "The fp32 mode's kernels, every instantiation").  maxpool_fp32_kernel through
tn_dbg_maxpool_fp32, bit-equal to tests/tools/stem_ref.py::maxpool_ref.  The launcher's refusals, each followed by a good call.
What is measured goes into the parity report under "fp32_kernel_err_over_sum_abs"."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fp32_chain_np as FC
from tools import stem_ref as SR

pytestmark = pytest.mark.gpu
STEM, C1X1, C3X3, TRANS = 0, 1, 2, 3
POISON = -7777.0
PAD_ROWS = 300

CASES = [
    # kind, B, Ho, Wo, K, N, layout, ldy, yoff, (H, W) or None
    (C1X1, 1, 4, 4, 32, 128, 0, 128, 0, None),         # M = 16 < one MFMA tile; one k-stage: the prefetch branch is never taken
    (C1X1, 3, 7, 7, 64, 128, 0, 128, 0, None),         # M = 147: a ragged second row tile; tiles span frames
    (C1X1, 1, 23, 31, 96, 128, 0, 160, 32, None),      # non-square; 6 row tiles, the last ragged; 3 k-stages
    (C3X3, 2, 1, 1, 1152, 32, 0, 64, 32, None),        # every tap but the centre is padding
    (C3X3, 3, 7, 7, 1152, 32, 0, 160, 96, None),       # M = 147: one ragged 256-row tile (large) or two tiles (small)
    (C3X3, 2, 5, 9, 1152, 32, 0, 64, 0, None),         # non-square: a swapped H / W shows
    (C3X3, 1, 29, 29, 1152, 32, 0, 256, 224, None),    # several tiles, ragged, at both tile heights; the concat offset
    (TRANS, 3, 7, 7, 128, 128, 0, 160, 32, (14, 14)),  # tiles span frames
    (TRANS, 1, 29, 29, 64, 256, 0, 256, 0, (59, 59)),  # odd input: the last row and column are ignored; 2 / 4 column blocks
    (TRANS, 1, 7, 7, 1024, 512, 0, 512, 0, (14, 14)),  # the last transition's K and N; 32 k-stages; 4 / 8 column blocks
    (STEM, 3, 7, 7, 147, 64, 0, 64, 0, (14, 13)),      # NCHW f32; K padded to 160; even and odd input extents
    (STEM, 1, 29, 29, 147, 64, 2, 96, 32, None),       # NHWC uint8: normalise on load
    (STEM, 2, 7, 7, 147, 64, 1, 64, 0, None),          # NHWC fp16
]
_id = lambda c: "kind%d-B%d-%dx%d-K%d-N%d-l%d-ldy%d-off%d" % c[:9]


def _make(case):
    kind, B, Ho, Wo, K, N, layout, ldy, yoff, hw = case
    H, W = hw if hw else (None, None)
    c = FC.make_case(kind, B, Ho, Wo, K, N, np.random.default_rng(500 + 11 * kind + 3 * Ho + Wo + K + N), layout, H, W)
    assert B * Ho * Wo * K * N <= 3.2e7                         # the CPU chain stays at a second or two
    return c


def _launch(c, tile, ldy, yoff, y=None, which=1):
    """one launch into a poisoned (M + 300, ldy) buffer -> (rc, the buffer on the host)"""
    from tennis_amd import _lib
    ctx = _lib.default_context()
    M = c["B"] * c["Ho"] * c["Wo"]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, s, t, es, et = (dev(c[k]) for k in ("x", "s", "t", "es", "et"))
    if y is None:
        y = torch.full((M + PAD_ROWS, ldy), POISON, dtype=torch.float32, device="cuda")
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    w = np.ascontiguousarray(c["w"])
    rc = ctx.lib.tn_dbg_conv_fp32x3(ctx.handle, which, c["kind"], tile, c["layout"], ptr(x), c["ldx"], c["K"], ptr(s), ptr(t),
                                    w.ctypes.data_as(C.c_void_p), c["N"], ptr(es), ptr(et), ptr(y), ldy, yoff, M, c["H"], c["W"],
                                    c["Ho"], c["Wo"])
    torch.cuda.synchronize()
    return rc, y.cpu().numpy()


def _err():
    from tennis_amd import _lib
    return _lib.default_context().lib.tn_last_error()


def _ordered(v):
    """float32 -> int64 that counts representable numbers in order (the distance of two of them is their distance in ulps)"""
    i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def chain_mismatch(got, want):
    """None if the bits agree, else a line: how many outputs differ, the worst distance in ulps, the first differing (row, column)"""
    bad = got != want
    if not bad.any():
        return None
    ulps = np.abs(_ordered(got) - _ordered(want))
    r, col = np.argwhere(bad)[0]
    return "%d of %d outputs differ from the chain, worst %d ulp; first at (row %d, column %d): device %r, chain %r (%d ulp)" % (
        bad.sum(), bad.size, ulps.max(), r, col, float(got[r, col]), float(want[r, col]), ulps[r, col])


def err_over_sum_abs(c, ref, y):
    """worst |y - y64| / sum |a||b| (the stem: after taking the epilogue fma's own rounding, 2^-24 |pre|, off the error, over
    sum |a||b| |es| - the epilogue terms of tests/test_gpu_fp32x3_mode.py::_run_case)"""
    y64, unit = FC.float64_output(c, ref["acc64"], ref["sab"], 1.0)
    err = np.abs(y.astype(np.float64) - y64)
    if c["es"] is not None:
        es64, et64 = c["es"].astype(np.float64), c["et"].astype(np.float64)
        fma = 2.0 ** -24 * np.abs(ref["acc64"] * es64 + et64)
        err, unit = np.maximum(err - fma, 0.0), unit - fma
    return float((err / np.maximum(unit, 1e-300)).max())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_tile_gives_the_chain(case, report):
    kind, B, Ho, Wo, K, N, layout, ldy, yoff, _ = case
    c = _make(case)
    ref = FC.conv_fp32_chain(c)
    assert not ref["subnormal"], "the chain claim is about normal numbers"
    M = B * Ho * Wo
    rec = {"chain": err_over_sum_abs(c, ref, ref["y"])}
    outs, lines = {}, []
    for tile in (1, 2, 0):
        rc, out = _launch(c, tile, ldy, yoff)
        assert rc == 0, _err()
        outs[tile] = out
        # rows past M and columns outside [yoff, yoff + N) are untouched
        assert (out[M:] == POISON).all(), "rows beyond M written (tile %d)" % tile
        assert (out[:M, :yoff] == POISON).all() and (out[:M, yoff + N:] == POISON).all(), "columns outside the window written (tile %d)" % tile
        got = out[:M, yoff:yoff + N]
        assert not np.isnan(got).any(), "NaN in the window (tile %d): channels past K were read" % tile
        rec["tile%d" % tile] = err_over_sum_abs(c, ref, got)
        rec["tile%d_differ_from_chain" % tile] = int((got != ref["y"]).sum())
        lines.append(chain_mismatch(got, ref["y"]))
        print("%s tile %d: |y - y64| / sum|a||b| = %.3e (chain %.3e); %s" % (_id(case), tile, rec["tile%d" % tile], rec["chain"],
                                                                            lines[-1] or "the chain's bits"))
    report.setdefault("fp32_kernel_err_over_sum_abs", {})[_id(case)] = rec
    # the tile choice changes no bit
    np.testing.assert_array_equal(outs[1], outs[2])
    np.testing.assert_array_equal(outs[0], outs[1])
    # the bits are the fused k-ascending chain's
    assert lines == [None, None, None], lines
    # float64: the device within twice the chain's own worst error on this case
    for tile in (1, 2, 0):
        assert rec["tile%d" % tile] <= 2.0 * rec["chain"], (tile, rec)


# ---------------------------------------------------------------- the max pool ----------------------------------------------------------------
def _maxpool(x, ldy, Ho, Wo, y=None, null=None):
    from tennis_amd import _lib
    ctx = _lib.default_context()
    B, H, W, _ = x.shape
    xd = torch.from_numpy(x).cuda()
    if y is None:
        y = torch.full((B * Ho * Wo + PAD_ROWS, max(ldy, 64)), POISON, dtype=torch.float32, device="cuda")
    px = None if null == "x" else C.c_void_p(xd.data_ptr())
    py = None if null == "y" else C.c_void_p(y.data_ptr())
    rc = ctx.lib.tn_dbg_maxpool_fp32(ctx.handle, px, B, H, W, py, ldy, Ho, Wo)
    torch.cuda.synchronize()
    return rc, y.cpu().numpy()


def _pool_input(B, H, W, seed):
    rng = np.random.default_rng(seed)
    return (-0.5 - np.abs(rng.standard_normal((B, H, W, 64)))).astype(np.float32)       # all negative: a 0 for the -inf padding shows


@pytest.mark.parametrize("B,H,W,ldy", [(2, 8, 8, 64), (1, 7, 9, 64), (3, 13, 6, 256)])
def test_maxpool_alone(B, H, W, ldy):
    x = _pool_input(B, H, W, 7 + H)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rc, out = _maxpool(x, ldy, Ho, Wo)
    assert rc == 0, _err()
    M = B * Ho * Wo
    want = SR.maxpool_ref(x).reshape(M, 64)
    assert want.max() < 0
    np.testing.assert_array_equal(out[:M, :64].astype(np.float64), want)
    assert (out[M:] == POISON).all() and (out[:M, 64:] == POISON).all()


def test_maxpool_refusals():
    x = _pool_input(1, 7, 9, 3)
    y = torch.full((4 * 5 + PAD_ROWS, 64), POISON, dtype=torch.float32, device="cuda")
    for kw, ldy, Ho, Wo, msg in ((dict(null="x"), 64, 4, 5, b"null"), (dict(null="y"), 64, 4, 5, b"null"),
                                 ({}, 64, 3, 5, b"tn_dbg_maxpool_fp32"), ({}, 64, 4, 4, b"tn_dbg_maxpool_fp32"), ({}, 64, 5, 5, b"tn_dbg_maxpool_fp32"),
                                 ({}, 48, 4, 5, b"maxpool_fp32: bad output stride"), ({}, 66, 4, 5, b"maxpool_fp32: bad output stride")):
        rc, out = _maxpool(x, ldy, Ho, Wo, y=y, **kw)
        assert rc != 0 and msg in _err(), (ldy, Ho, Wo, _err())
        assert (out == POISON).all()
    rc, out = _maxpool(x, 64, 4, 5, y=y)
    assert rc == 0, _err()
    np.testing.assert_array_equal(out[:20].astype(np.float64), SR.maxpool_ref(x).reshape(20, 64))
    assert (out[20:] == POISON).all()


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------
def test_launcher_refusals_then_a_good_call():
    rng = np.random.default_rng(77)
    good = FC.make_case(C1X1, 1, 5, 5, 64, 128, rng)
    ref = FC.conv_fp32_chain(good)
    M, ldy = 25, 160
    y = torch.full((M + PAD_ROWS, ldy), POISON, dtype=torch.float32, device="cuda")

    def refused(c, tile, ldy_, yoff, msg):
        rc, out = _launch(c, tile, ldy_, yoff, y=y)
        assert rc != 0 and msg in _err(), (rc, _err())
        assert (out == POISON).all(), "a refused call wrote"
        rc, out = _launch(good, 0, ldy, 32, y=torch.full_like(y, POISON))
        assert rc == 0, _err()
        assert chain_mismatch(out[:M, 32:160], ref["y"]) is None, chain_mismatch(out[:M, 32:160], ref["y"])
        assert (out[M:] == POISON).all() and (out[:M, :32] == POISON).all()

    refused(good, 3, ldy, 32, b"conv_fp32: tile selector")
    refused(good, -1, ldy, 32, b"conv_fp32: tile selector")
    k36 = FC.make_case(C1X1, 1, 5, 5, 36, 128, rng)             # the k loop would read s, t and the activation up to channel 64
    refused(k36, 0, ldy, 32, b"conv_fp32: channel strides must be multiples of 4 and K a multiple of the k-stage (32)")
    tr = FC.make_case(TRANS, 1, 5, 5, 64, 128, rng, H=9, W=10)  # 2 Ho > H: the average would read a row past the map
    refused(tr, 0, ldy, 32, b"output")
    refused(good, 0, ldy, 64, b"conv_fp32: output columns out of range")   # yoff + N > ldy
    refused(good, 0, 128, 32, b"conv_fp32: output columns out of range")
