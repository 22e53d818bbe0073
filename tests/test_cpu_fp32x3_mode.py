"""The fp32x3 encoder mode (TN_ENC_FP32X3) on the host side: the flag in the C header and the ctypes table, the backbone's
``conversion="fp32x3"`` keeping the fp32 parameters as they are, evaluate.py's ``--fp16_conversion fp32x3`` and the host's
three-term bf16 weight split (tn_fp32x3_split, host code of the library).  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_in_header_and_binding():
    from tennis_amd import _lib
    assert _lib.ENC_FP32X3 == 8
    assert _lib.ENC_FP32 == 4 and _lib.ENC_EXACT_WEIGHTS == 1                 # the other modes' flags are unchanged
    header = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    assert re.search(r"^#define TN_ENC_FP32X3 8\b", header, re.M)
    assert re.search(r"^#define TN_ENC_FP32 4\b", header, re.M)
    assert re.search(r"^#define TN_ENC_EXACT_WEIGHTS 1\b", header, re.M)
    assert "tn_dbg_conv_fp32x3" in _lib.declared_symbols() and "tn_fp32x3_split" in _lib.declared_symbols()
    assert "tn_dbg_conv_fp32x3" in open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()


def test_backbone_fp32x3_keeps_fp32_parameters():
    from tennis_amd import weights as W
    from tennis_amd.nn import DenseNet121Backbone
    net = DenseNet121Backbone(conversion="fp32x3")
    net.initialize()
    assert net._fp32x3 and not net._fp32 and not net._exact
    ref = W.make_densenet121_weights(0, net.prefix, fp16_model=False)
    conv = [k for k in net._own_params if re.search(r"conv\d+_weight$", k)]
    assert len(conv) == 120
    for k in conv:
        d = net._own_params[k].data
        assert d.dtype == np.float32
        np.testing.assert_array_equal(d, ref[k])                    # adopted bit for bit
    w = net._own_params[net.prefix + "stage2_conv0_weight"].data
    assert (w.astype(np.float16).astype(np.float32) != w).mean() > 0.5        # nothing was rounded on adoption
    # a checkpoint set after construction (load_parameters / set_params go through _adopt) stays fp32 as well
    net = DenseNet121Backbone(conversion="fp32x3", prefix="densenet7_")
    p = W.make_densenet121_weights(3, "densenet7_", fp16_model=False)
    net.set_params(p)
    for k in ("densenet7_conv0_weight", "densenet7_stage4_conv31_weight", "densenet7_conv3_weight"):
        np.testing.assert_array_equal(net._own_params[k].data, p[k])


def test_unknown_conversion_lists_the_new_choice():
    from tennis_amd.nn import DenseNet121Backbone
    with pytest.raises(ValueError) as ei:
        DenseNet121Backbone(conversion="bf16")
    for choice in ("nearest", "calibrated", "exact", "fp32", "fp32x3"):
        assert repr(choice) in str(ei.value)


def test_get_model_passes_fp32x3_through():
    from tennis_amd.model_zoo import get_model
    feats = get_model("DenseNet121", pretrained=False, conversion="fp32x3").features
    assert feats._fp32x3
    w = feats._own_params[feats.prefix + "conv1_weight"].data
    assert (w.astype(np.float16).astype(np.float32) != w).any()


def test_evaluate_accepts_fp32x3_conversion():
    from tennis_amd import evaluate
    p = evaluate.build_parser()
    assert p.parse_args(["--fp16_conversion", "fp32x3"]).fp16_conversion == "fp32x3"
    assert p.parse_args(["--fp16_conversion", "fp32"]).fp16_conversion == "fp32"
    assert p.parse_args([]).fp16_conversion == "nearest"
    with pytest.raises(SystemExit):
        p.parse_args(["--fp16_conversion", "bf16"])


def _bf16_rne_bits(x32):
    """round-to-nearest-even bf16 of finite fp32 values, as uint16 bit patterns (numpy bit arithmetic)"""
    u = x32.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_to_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def test_host_three_term_split():
    """w1 + w2 + w3 reproduces w to 2^-24 |w| on seeded DenseNet weights, each term is a bf16 number, and the terms are the
    round-to-nearest-even chain w1 = bf16(w), w2 = bf16(w - w1), w3 = bf16(w - w1 - w2)."""
    from tennis_amd import _lib
    from tennis_amd import weights as W
    lib = _lib.load()
    p = W.make_densenet121_weights(0, fp16_model=False)
    w = np.concatenate([p["densenet0_" + k].ravel() for k in ("conv0_weight", "stage1_conv0_weight", "stage3_conv47_weight", "conv3_weight")]
                       + [np.array([0.0, -0.0, 1.0, -1.0, 1e-30, 3.0e38, np.float32(1) + np.float32(2.0 ** -23)], np.float32)]).astype(np.float32)
    w = np.ascontiguousarray(w)
    t = [np.empty(w.size, np.uint16) for _ in range(3)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tn_fp32x3_split(ptr(w), w.size, ptr(t[0]), ptr(t[1]), ptr(t[2])) == 0
    f = [_bf16_to_f32(h) for h in t]                                  # a uint16 pattern widened with 16 zero bits IS a bf16 number
    s = f[0].astype(np.float64) + f[1].astype(np.float64) + f[2].astype(np.float64)
    assert (np.abs(s - w.astype(np.float64)) <= 2.0 ** -24 * np.abs(w.astype(np.float64))).all()
    assert (np.abs(s - w.astype(np.float64)) > 0).mean() < 0.01       # (almost every weight is reproduced exactly: 24 bits in three terms)
    # the chain, restated
    h1 = _bf16_rne_bits(w)
    r1 = w - _bf16_to_f32(h1)
    h2 = _bf16_rne_bits(r1)
    r2 = r1 - _bf16_to_f32(h2)
    h3 = _bf16_rne_bits(r2)
    for got, want in zip(t, (h1, h2, h3)):
        np.testing.assert_array_equal(got, want)
    # two terms alone are not enough: the third carries bits on most weights
    assert (f[2] != 0).mean() > 0.5
