"""oracle/fp32_chain_np.py - the fp32 mode's convolution kernel restated in exact fp32 steps - held to its own references, no GPU:

  * fmaf32 against exact rational arithmetic, on random triples (cancelling ones among them) and on constructed triples whose float64
    sum lands exactly on a float32 tie with a residual of either sign, where float32(float64(a) * b + c) is wrong;
  * the float64 product and sum |a||b| it returns are those of tests/test_gpu_fp32x3_mode.py::_case on the same operands;
  * the discriminators: what tests/test_gpu_fp32_kernels.py can tell apart by comparing bits with the chain - an unfused chain, a
    descending one, one that sums k pairs first, padding before the activation, a left-to-right average - each changes output bits;
  * the debug symbols the GPU test calls are declared in the ctypes table and the header."""
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import fp32_chain_np as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM, C1X1, C3X3, TRANS = 0, 1, 2, 3


def _round_f32(q):
    """a Fraction rounded to the nearest float32, ties to even (below 2^128)"""
    if q == 0:
        return np.float32(0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    unit = Fraction(2) ** (max(e, -126) - 23)                  # spacing of float32 at q (subnormal range: 2^-149)
    n, rem = divmod(q, unit)
    n = int(n)
    if rem * 2 > unit or (rem * 2 == unit and n % 2):
        n += 1
    v = n * unit
    return np.float32(sign * float(v))                         # n < 2^25, unit a power of two: exact in double and in float32


def _fma_exact(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_round_f32_is_float32_rounding():
    rng = np.random.default_rng(1)
    v = rng.standard_normal(500) * 2.0 ** rng.integers(-60, 60, 500)
    for x in v:
        assert _round_f32(Fraction(float(x))) == np.float32(x)
    assert _round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == np.float32(1)                          # tie -> even
    assert _round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == np.float32(1 + 2.0 ** -22)             # tie -> even, upwards
    assert _round_f32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 90)) == np.float32(1 + 2.0 ** -23)


def test_fmaf32_against_rational_arithmetic():
    rng = np.random.default_rng(2)
    n = 3000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    # a third of them cancel: c within a few ulps of -a b, where the fused and the unfused result differ most
    near = (-(a.astype(np.float64) * b)).astype(np.float32)
    near = near.view(np.int32) + rng.integers(-3, 4, n).astype(np.int32)
    c[::3] = near.view(np.float32)[::3]
    # and a third sit at the accumulator's scale in the kernel: |c| ~ 10 |a b|
    c[1::3] = (10.0 * a[1::3].astype(np.float64) * b[1::3] * rng.standard_normal(n)[1::3]).astype(np.float32)
    got = FC.fmaf32(a, b, c)
    assert got.dtype == np.float32 and got.shape == (n,)
    want = np.array([_fma_exact(*t) for t in zip(a, b, c)], np.float32)
    np.testing.assert_array_equal(got, want)
    unfused = a * b + c
    print("fmaf32 differs from the unfused a * b + c on %.1f%% of %d triples" % (100.0 * (unfused != want).mean(), n))
    assert (unfused != want).any()
    # broadcasting, the way the chain calls it
    g2 = FC.fmaf32(a[:40, None], b[None, :30], c[:30][None, :])
    w2 = np.array([[_fma_exact(a[i], b[j], c[j]) for j in range(30)] for i in range(40)], np.float32)
    np.testing.assert_array_equal(g2, w2)


def _tie_triples():
    """a b = 2^-24 (1 +- 2^-46) exactly, from 8384513 * 8392705 = 2^46 + 1 and (2^23 + 1)(2^23 - 1) = 2^46 - 1: added to c = 1 or
    1 + 2^-23 the float64 sum is 1 + 2^-24 or 1 + 3 2^-24 - a float32 tie - and the residual -+2^-70 says which neighbour is right"""
    assert 8384513 * 8392705 == 2 ** 46 + 1
    up = (np.float32(8384513.0), np.float32(8392705.0 * 2.0 ** -70))            # product 2^-24 + 2^-70
    dn = (np.float32(2 ** 23 + 1), np.float32((2 ** 23 - 1) * 2.0 ** -70))      # product 2^-24 - 2^-70
    out = []
    for (a, b), c, want in ((up, 1.0, 1.0 + 2.0 ** -23),                        # ties-to-even says 1: wrong, the sum is above the tie
                            (dn, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23),           # ties-to-even says 1 + 2^-22: wrong, it is below
                            (up, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22),           # (even is right here, and in the next)
                            (dn, 1.0, 1.0)):
        for scale in (1.0, 2.0 ** 17, 2.0 ** -31):
            for sign in (1.0, -1.0):
                out.append((np.float32(a * scale), np.float32(b * sign), np.float32(c * scale * sign), np.float32(want * scale * sign)))
    return out


def test_fmaf32_on_float32_ties_with_a_residual():
    naive_wrong = 0
    for a, b, c, want in _tie_triples():
        s = np.float64(a) * np.float64(b) + np.float64(c)
        lo29 = np.array([s]).view(np.uint64)[0] & np.uint64(0x1FFFFFFF)
        assert lo29 == 0x10000000, "the float64 sum is a float32 tie"
        assert Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)) != Fraction(float(s)), "with a nonzero residual"
        assert _fma_exact(a, b, c) == want
        assert FC.fmaf32(a, b, c) == want, (a, b, c)
        naive_wrong += int(np.float32(s) != want)
    assert naive_wrong == 12, naive_wrong                       # residual above an even-rounded-down tie, below an even-rounded-up one
    a, b, c, want = (np.array(v, np.float32) for v in zip(*_tie_triples()))
    np.testing.assert_array_equal(FC.fmaf32(a, b, c), want)
    assert ((a.astype(np.float64) * b + c).astype(np.float32) != want).sum() == 12


def test_fmaf32_in_the_subnormal_range_and_the_flag():
    rng = np.random.default_rng(3)
    n = 600
    a = (rng.standard_normal(n) * 2.0 ** -70).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** -70).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** -140).astype(np.float32)
    want = np.array([_fma_exact(*t) for t in zip(a, b, c)], np.float32)
    np.testing.assert_array_equal(FC.fmaf32(a, b, c), want)
    _, sub = FC.chain(a[:8].reshape(2, 4), b[:8].reshape(4, 2))
    assert sub
    _, sub = FC.chain(np.ones((2, 4), np.float32), np.ones((4, 2), np.float32))
    assert not sub


# ---- the float64 side is _case's ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,Ho,Wo,K,layout", [(STEM, 2, 3, 3, 147, 0), (STEM, 1, 3, 4, 147, 1), (STEM, 1, 4, 3, 147, 2),
                                                   (C1X1, 2, 3, 5, 64, 0), (C3X3, 2, 3, 4, 1152, 0), (TRANS, 2, 3, 4, 64, 0)])
def test_float64_side_is_the_fp32x3_tests(kind, B, Ho, Wo, K, layout):
    import test_gpu_fp32x3_mode as X3
    c = X3._case(kind, B, Ho, Wo, K, np.random.default_rng(5 + kind), layout)
    r = FC.conv_fp32_chain(c)
    assert not r["subnormal"]
    np.testing.assert_array_equal(r["acc64"], c["acc64"])
    np.testing.assert_array_equal(r["sab"], c["sab"])
    y64, bound = FC.float64_output(c, r["acc64"], r["sab"], 1.0)
    err = np.abs(r["y"].astype(np.float64) - y64) / bound
    print("kind %d K = %d: chain at %.2e of sum |a||b| from float64" % (kind, K, err.max()))
    assert err.max() < 1e-6                                    # an fp32 chain of these K: a few 1e-7
    if layout == 2:                                            # the loader's normalisation is weights.normalize_to_nchw_f32's
        from tennis_amd import weights as W
        np.testing.assert_array_equal(FC.stem_input_nchw(c), W.normalize_to_nchw_f32(c["x"]))


# ---- the discriminators -------------------------------------------------------------------------------------------------------------
SMALL = {STEM: (STEM, 1, 4, 4, 147, 64), C1X1: (C1X1, 1, 4, 4, 64, 128), C3X3: (C3X3, 1, 3, 3, 1152, 32), TRANS: (TRANS, 1, 3, 3, 64, 64)}


@pytest.fixture(scope="module")
def small():
    out = {}
    for kind, spec in SMALL.items():
        c = FC.make_case(*spec, np.random.default_rng(40 + kind), layout=2 if kind == STEM else 0)
        r = FC.conv_fp32_chain(c)
        assert not r["subnormal"] and np.isfinite(r["y"]).all()
        out[kind] = (c, r)
    return out


def _finish(c, acc):
    return acc if c["es"] is None else np.maximum(FC.fmaf32(acc, c["es"], c["et"]), np.float32(0))


@pytest.mark.parametrize("order", ["unfused", "descending", "pairs"])
@pytest.mark.parametrize("kind", [STEM, C1X1, C3X3, TRANS])
def test_chain_order_changes_bits(small, kind, order):
    c, r = small[kind]
    a32, _ = FC.operand_a(c)
    y, _ = FC.chain(a32, c["w"], order)
    frac = float((_finish(c, y) != r["y"]).mean())
    print("kind %d, %s chain: %.1f%% of the outputs differ from the fused ascending chain" % (kind, order, 100.0 * frac))
    assert frac > 0.0
    again, _ = FC.chain(a32, c["w"])                            # (and the chain itself is reproducible)
    np.testing.assert_array_equal(_finish(c, again), r["y"])


def test_padding_before_the_activation_changes_bits(small):
    c, r = small[C3X3]
    a32, _ = FC.operand_a(c, pad_before_activation=True)
    y, _ = FC.chain(a32, c["w"])
    frac = float((y != r["y"]).mean())
    print("3x3, padding before the activation: %.1f%% of the outputs differ" % (100.0 * frac))
    assert frac > 0.0


def test_left_to_right_average_changes_bits(small):
    c, r = small[TRANS]
    a32, _ = FC.operand_a(c, flat_average=True)
    y, _ = FC.chain(a32, c["w"])
    frac = float((y != r["y"]).mean())
    print("transition, (v00 + v01 + v10 + v11) * 0.25 left to right: %.1f%% of the outputs differ" % (100.0 * frac))
    assert frac > 0.0


def test_nan_beyond_k_is_not_read(small):
    for kind in (C1X1, TRANS):
        c, r = small[kind]
        assert np.isnan(c["x"][..., c["K"]:]).all() and c["x"].shape[-1] == c["ldx"] == c["K"] + 32
        assert np.isfinite(r["y"]).all() and np.isfinite(r["acc64"]).all()


def test_symbols_declared():
    from tennis_amd import _lib
    header = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    for name in ("tn_dbg_maxpool_fp32", "tn_dbg_conv_fp32x3"):
        assert name in _lib.declared_symbols()
        assert name in header
    assert "launch_conv_fp32(const Fp32ConvArgs &a, hipStream_t s, int tile = 0)" in open(os.path.join(ROOT, "tennis_amd", "csrc", "common.h")).read()
