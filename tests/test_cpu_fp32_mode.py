"""The fp32 encoder mode (TN_ENC_FP32) on the host side: the flag in the C header and the ctypes table, the backbone's
``conversion="fp32"`` keeping the fp32 parameters as they are, and evaluate.py's ``--fp16_conversion fp32``.  No GPU needed."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_in_header_and_binding():
    from tennis_amd import _lib
    assert _lib.ENC_FP32 == 4
    header = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    assert re.search(r"^#define TN_ENC_FP32 4\b", header, re.M)
    assert re.search(r"^#define TN_ENC_EXACT_WEIGHTS 1\b", header, re.M)      # the other mode's flag is unchanged


def test_backbone_fp32_keeps_fp32_parameters():
    from tennis_amd import weights as W
    from tennis_amd.nn import DenseNet121Backbone
    net = DenseNet121Backbone(conversion="fp32")
    net.initialize()
    assert net._fp32 and not net._exact
    ref = W.make_densenet121_weights(0, net.prefix, fp16_model=False)
    conv = [k for k in net._own_params if k.endswith("conv_weight") or re.search(r"conv\d+_weight$", k)]
    assert len(conv) == 120
    for k in conv:
        d = net._own_params[k].data
        assert d.dtype == np.float32
        np.testing.assert_array_equal(d, ref[k])                    # adopted as they are
    # ... and they are NOT fp16 numbers: nothing was rounded on adoption
    w = net._own_params[net.prefix + "stage2_conv0_weight"].data
    assert (w.astype(np.float16).astype(np.float32) != w).mean() > 0.5
    # the default conversion does change them (the fp16 model)
    dflt = DenseNet121Backbone(prefix="densenet9_")
    dflt.initialize()
    w16 = dflt._own_params["densenet9_stage2_conv0_weight"].data
    assert (w16 != W.make_densenet121_weights(0, "densenet9_", fp16_model=False)["densenet9_stage2_conv0_weight"]).mean() > 0.5


def test_backbone_fp32_keeps_loaded_parameters():
    """A checkpoint set after construction (load_parameters / set_params go through _adopt) stays fp32 as well."""
    from tennis_amd import weights as W
    from tennis_amd.nn import DenseNet121Backbone
    net = DenseNet121Backbone(conversion="fp32", prefix="densenet7_")
    p = W.make_densenet121_weights(3, "densenet7_", fp16_model=False)
    net.set_params(p)
    for k in ("densenet7_conv0_weight", "densenet7_stage4_conv31_weight", "densenet7_conv3_weight"):
        np.testing.assert_array_equal(net._own_params[k].data, p[k])


def test_unknown_conversion_still_raises():
    from tennis_amd.nn import DenseNet121Backbone
    with pytest.raises(ValueError) as ei:
        DenseNet121Backbone(conversion="bf16")
    for choice in ("nearest", "calibrated", "exact", "fp32"):
        assert repr(choice) in str(ei.value)


def test_get_model_passes_fp32_through():
    from tennis_amd.model_zoo import get_model
    feats = get_model("DenseNet121", pretrained=False, conversion="fp32").features
    assert feats._fp32
    w = feats._own_params[feats.prefix + "conv1_weight"].data
    assert (w.astype(np.float16).astype(np.float32) != w).any()


def test_evaluate_accepts_fp32_conversion():
    from tennis_amd import evaluate
    p = evaluate.build_parser()
    assert p.parse_args(["--fp16_conversion", "fp32"]).fp16_conversion == "fp32"
    assert p.parse_args([]).fp16_conversion == "nearest"
    with pytest.raises(SystemExit):
        p.parse_args(["--fp16_conversion", "bf16"])
