"""-m "not gpu": the float64 stem reference and the dither emulation of tests/tools/stem_ref.py, checked on their own - they are what
tests/test_gpu_stem_head.py holds the stem kernels to.

  * stem_exact, fed the fp16 model's own weights, is the oracle's `pool0` tap (oracle/densenet_np.py, fp32) on the golden 224 case;
  * dither_emulate is unbiased where round-to-nearest is not, and the assertion can tell the two apart;
  * the +- slack rule of the bitwise dither check leaves under 5 % of a case's outputs undecided, for every fused case of the GPU
    test - computed from the reference alone, so the rule cannot hide a failure behind its exclusions."""
import numpy as np
import pytest

from oracle import densenet_np as dn
from tennis_amd import weights as W
from tools import stem_ref as SR

FUSED = [c for c in SR.STEM_CASES if c[5]]
SHARE_CAP = 0.05


def test_stem_exact_is_the_oracles_pool0_tap_on_the_golden_case():
    """The fixture's inputs (tests/golden/make_oracle_fixtures.py: weights seed 0, frames seed 1234, 2 x 224 x 224): the oracle works in
    fp32 on ToTensor + Normalize of the frames and the un-folded weights w; stem_exact on the uint8 frames and fp16(w * wfactor), which
    for the fp16 model is w * wfactor itself.  What separates them is the oracle's fp32 arithmetic: the 147 products of a sum (the
    same 160 * 2^-24 * A the kernels are allowed) and the three roundings of the normalisation and the BatchNorm on the result."""
    p = W.make_densenet121_weights(0)
    u8 = W.synthetic_frames_u8(2, 224, 1234)
    taps = {}
    dn.densenet121_features(W.normalize_to_nchw_f32(u8), p, taps=taps)
    pre = "densenet0_"
    ref, A, _ = SR.stem_exact(p[pre + "conv0_weight"], p[pre + "batchnorm0_gamma"], p[pre + "batchnorm0_beta"], p[pre + "batchnorm0_running_mean"],
                              p[pre + "batchnorm0_running_var"], None, False, SR.LAYOUT_NHWC_U8, u8)
    assert ref.shape == taps["pool0"].shape == (2, 56, 56, 64)
    err = np.abs(ref - taps["pool0"].astype(np.float64))
    bound = SR.slack(A) + 8 * 2.0 ** -24 * (np.abs(ref) + 1.0)
    print("stem_exact vs oracle pool0: max err %.3g, worst err / bound %.3f, |ref| max %.3g" % (err.max(), (err / bound).max(), np.abs(ref).max()))
    assert np.all(err <= bound)
    assert err.max() < 2e-5 * max(1.0, np.abs(ref).max())
    # the hi + lo weights of the exact mode are the same numbers for this model (lo = 0)
    assert np.array_equal(SR.stem_weights(p[pre + "conv0_weight"], True), SR.stem_weights(p[pre + "conv0_weight"], False))


def test_rtz_conversion_against_numpy():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(0, 1, 20000), rng.normal(0, 1e-4, 20000), rng.normal(0, 1e-7, 20000), [0.0, -0.0, 65504.0, 1e6, 2.0 ** -24, 2.0 ** -25]]).astype(np.float32)
    h = SR.f32_to_f16_rtz(v.view(np.uint32)).view(np.float16).astype(np.float64)
    near = v.astype(np.float16).astype(np.float64)
    v64 = v.astype(np.float64)
    assert np.all(np.abs(h) <= np.abs(v64)) and np.all(np.signbit(h) == np.signbit(v64))
    ok = np.abs(v64) <= 65504.0
    assert np.all(np.abs(h - v64)[ok] < SR.ulp16(v64)[ok])                      # one of the two neighbours: the one towards zero
    exact = near == v64
    assert np.array_equal(h[exact], v64[exact]) and exact.sum() > 3
    assert h[-3] == 65504.0 and h[-2] == 2.0 ** -24 and h[-1] == 0.0


@pytest.mark.parametrize("value", [0.3001, 1.7003, 5.123, 0.0421, -2.6001, 7.3e-5])
def test_dither_is_unbiased_on_a_constant_map_and_round_to_nearest_is_not(value):
    """A constant over the 56 x 56 x 64 pooled map of a 224 x 224 frame: the mean signed error of a channel over its N = 3136
    positions within 5 sigma of zero, sigma = 0.5 ulp / sqrt(N) (a two-point distribution on the neighbours has a variance of at most
    ulp^2 / 4).  Round-to-nearest makes the same error at every position and misses the same bound."""
    v = np.full((1, 56, 56, 64), value, np.float32)
    exact = v.astype(np.float64)
    n = 56 * 56
    bound = 5 * 0.5 * SR.ulp16(value) / np.sqrt(n)
    d = SR.dither_emulate(v, *SR.grid(v.shape)).astype(np.float64)
    assert np.all(np.abs(d - exact) < SR.ulp16(value))
    bias = (d - exact).mean(axis=(0, 1, 2))
    print("value %g: worst channel bias %.3g ulp (bound %.3g ulp)" % (value, np.abs(bias).max() / SR.ulp16(value), bound / SR.ulp16(value)))
    assert np.all(np.abs(bias) <= bound)
    rn = (v.astype(np.float16).astype(np.float64) - exact).mean(axis=(0, 1, 2))
    assert np.all(np.abs(rn) > bound)
    # the key is (row, column, channel) and nothing else: a second frame gets the same numbers
    v2 = np.full((2, 56, 56, 64), value, np.float32)
    d2 = SR.dither_emulate(v2, *SR.grid(v2.shape))
    assert np.array_equal(d2[0], d2[1])


def test_dither_truncates_below_fp16s_normal_range():
    """What the emulation shows about dither_pack, and the device is held to bit for bit: the 13-bit field sits below the mantissa of
    a NORMAL half.  Below 2^-14 the conversion drops 14 to 24 bits and the field no longer reaches the kept ones - at 2^-15 and
    below the stored value is the truncation to a multiple of 2^-24, the same at every position: a bias of at most 2^-24 = 6e-8
    in absolute terms (docs/numerics.md), not the unbiased rounding of the normal range."""
    for value in (3.1e-5, 1.234e-6, -2.2e-5):
        v = np.full((1, 56, 56, 64), value, np.float32)
        d = SR.dither_emulate(v, *SR.grid(v.shape)).astype(np.float64)
        assert np.all(d == np.trunc(np.float64(np.float32(value)) * 2.0 ** 24) / 2.0 ** 24)


def test_dither_fields_are_spread_over_13_bits():
    t = SR.dither_field(*SR.grid((1, 56, 56, 64))).astype(np.float64)
    assert t.min() >= 0 and t.max() <= 8191
    m = t.mean(axis=(0, 1, 2))
    assert np.all(np.abs(m - 4095.5) < 5 * 8192 / np.sqrt(12 * 3136.0))


@pytest.mark.parametrize("case", FUSED, ids=[c[0] for c in FUSED])
def test_the_slack_rule_leaves_few_outputs_undecided(case):
    """The bitwise dither check of tests/test_gpu_stem_head.py compares only where moving the float64 value by +- its slack
    (160 * 2^-24 * A) does not change the emulated half.  The share it leaves out has to stay under 5 % per case; this is a property of
    the case's inputs (stem_ref.stem_params says how they were chosen) and is established here from the reference alone."""
    p, x, ref, A, pre = SR.case_reference(case)
    _, ok = SR.decided(pre, A, p["m_c"])
    share = 1.0 - ok.mean()
    per_frame = 1.0 - ok.mean(axis=(1, 2, 3))
    print("%s: undecided share %.4f (per frame %s)" % (case[0], share, np.round(per_frame, 4)))
    assert share < SHARE_CAP
