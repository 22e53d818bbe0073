"""-m gpu: the fp32 encoder mode (TN_ENC_FP32, csrc/dense_fp32.hip) against the fp32 reference evaluation.

fp32 activations, fp32 weights, every product on the f32-input MFMA: the mode holds the 1e-3 bar where no fp16-activation mode
does (fine checkerboards, flat frames at 512 x 512, trained-looking parameters).  Oracle: oracle/torch_ref.py
on the UN-rounded fp32 weights and the un-rounded normalised input (reference models/vision/definitions.py:27-33); the frame mix of
tests/tools/parity_timed.py (15 frames of each of 16 families + 16 fine checkerboards in one 256-frame call).  What is measured
goes into the session's parity report (the `report` fixture, key "fp32_mode_runs")."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tools import parity_timed as PT

pytestmark = pytest.mark.gpu
BAR = 1e-3


def _record(report, key, r):
    report.setdefault("fp32_mode_runs", {})[key] = r


def _dense_w(dim):
    from tennis_amd import weights as W
    return W.make_dense_weights(1, 11, dim, "framemodel0_dense0_")["framemodel0_dense0_weight"]


def _encoder(p, size, max_batch):
    from tennis_amd.engine import DenseNet121Features
    return DenseNet121Features(p, size, max_batch=max_batch, fp32=True)


@pytest.fixture(scope="module")
def seeded224():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    p = PT.make_weights("seeded")
    frames, labels = PT.batch(256)
    ref = PT.oracle_features(p, frames)
    enc = _encoder(p, 224, 256)
    x = torch.from_numpy(frames).cuda()
    feat = enc(x).cpu().numpy()
    return dict(p=p, frames=frames, labels=labels, ref=ref, enc=enc, x=x, feat=feat)


def _check_all_families(r, tag):
    fams = r["families"]
    assert len(fams) == 17 and "finechecker" in fams, sorted(fams)
    bad = {f: (v["feature_max"], v["logit_max"], v["over_bar"]) for f, v in fams.items()
           if not (v["feature_max"] < BAR and v["logit_max"] < BAR and v["over_bar"] == 0)}
    assert not bad, (tag, bad)


def test_seeded_224_batch256_every_family(seeded224, report):
    S = seeded224
    r = PT.summarize(S["feat"], S["ref"], S["labels"], _dense_w(1024))
    _record(report, "seeded / 224 / B=256", r)
    report["fp32_mode_seeded_224_feature_max"] = r["feature_max"]
    report["fp32_mode_seeded_224_logit_max"] = r["logit_max"]
    print("seeded 224:", {k: r[k] for k in ("feature_max", "logit_max", "over_bar", "worst_family")})
    assert r["frames"] == 256 and r["over_bar"] == 0
    _check_all_families(r, "seeded 224")
    # pinned: measured 9.5e-6 features / 5.4e-6 logits on an MI355X (an fp32 evaluation against another one: summation order only)
    assert r["feature_max"] < 2.8e-5 and r["logit_max"] < 1.6e-5, (r["feature_max"], r["logit_max"])


def test_profile_runs_only_fp32_kernels(seeded224):
    S = seeded224
    stats, out = S["enc"].profile(S["x"][:64])
    names = [s["name"] for s in stats]
    assert names[0] == "fp32_stem_conv7x7_bn_relu" and names[-1] == "head_bnrelu_avgpool7", names
    assert all(n.startswith("fp32_") for n in names[:-1]), names
    for fp16_family in ("dense_layer_strip", "dense_block_", "dense_layer_fused", "conv1x1_bnrelu", "conv3x3_bnrelu",
                        "transition_conv1x1_avgpool", "stem_conv_bn_relu_maxpool"):
        assert not [n for n in names if n.startswith(fp16_family)], names
    assert len(names) <= 16
    launches = {s["name"]: s["launches"] for s in stats}
    assert launches["fp32_dense1x1_56x56"] == 6 and launches["fp32_dense3x3_7x7"] == 16 and launches["fp32_transition_14x14"] == 1
    # the profiled forward computes what the plain one does
    np.testing.assert_array_equal(out.cpu().numpy(), S["feat"][:64])


def test_trained_like_224_batch256(seeded224, report):
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    p = PT.make_weights("trained")
    frames, labels = seeded224["frames"], seeded224["labels"]
    ref = PT.oracle_features(p, frames)
    enc = _encoder(p, 224, 256)
    feat = enc(seeded224["x"]).cpu().numpy()
    r = PT.summarize(feat, ref, labels, _dense_w(1024))
    _record(report, "trained / 224 / B=256", r)
    report["fp32_mode_trained_224_feature_max_scaled"] = r["feature_max_scaled"]
    print("trained 224:", {k: r[k] for k in ("feature_max", "feature_max_scaled", "logit_max_scaled", "worst_family")})
    assert len(r["families"]) == 17
    assert r["feature_max_scaled"] < BAR and r["logit_max_scaled"] < BAR, {f: v["feature_max_scaled"] for f, v in r["families"].items()}


def test_seeded_512_batch32(report):
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    p = PT.make_weights("seeded")
    frames, labels = PT.batch(32, size=512)
    ref = PT.oracle_features(p, frames)
    enc = _encoder(p, 512, 32)
    assert enc.feature_dim == 4096
    feat = enc(torch.from_numpy(frames).cuda()).cpu().numpy()
    r = PT.summarize(feat, ref, labels, _dense_w(4096))
    _record(report, "seeded / 512 / B=32", r)
    report["fp32_mode_seeded_512_feature_max"] = r["feature_max"]
    print("seeded 512:", {k: r[k] for k in ("feature_max", "logit_max", "over_bar", "worst_family")})
    for f in ("constant", "text", "halfblack"):
        assert f in r["families"], sorted(r["families"])
    _check_all_families(r, "seeded 512")


@pytest.mark.parametrize("size", [236, 448])
def test_other_sizes_batch4(size, report):
    p = PT.make_weights("seeded")
    frames, labels = PT.batch(4, seed=11, size=size)
    ref = PT.oracle_features(p, frames)
    enc = _encoder(p, size, 4)
    feat = enc(torch.from_numpy(frames).cuda()).cpu().numpy()
    assert feat.shape == ref.shape
    r = PT.summarize(feat, ref, labels, _dense_w(ref.shape[1]))
    _record(report, f"seeded / {size} / B=4", r)
    assert r["feature_max"] < BAR and r["logit_max"] < BAR, (r["feature_max"], r["logit_max"])


def test_batch_independence_and_pipelining(seeded224):
    """A frame's features are the same bits alone, inside the 256-frame call (two half batches on the side streams) and in a
    pipelined sequence of three whole-batch calls (alternating streams and workspace sets)."""
    S = seeded224
    enc, x, feat = S["enc"], S["x"], S["feat"]
    for i in (0, 77, 255):
        one = enc(x[i:i + 1]).cpu().numpy()
        np.testing.assert_array_equal(one[0], feat[i])
    perm = [x[torch.randperm(256, generator=torch.Generator().manual_seed(s))] for s in range(3)]
    outs = [torch.empty((256, enc.feature_dim), dtype=torch.float32, device=x.device) for _ in range(3)]
    enc.set_pipelined(True)
    try:
        for xi, oi in zip(perm, outs):
            enc(xi, out=oi)
        enc.join(1)
        enc.join(0)
    finally:
        enc.set_pipelined(False)
    torch.cuda.synchronize()
    for s, oi in enumerate(outs):
        idx = torch.randperm(256, generator=torch.Generator().manual_seed(s)).numpy()
        np.testing.assert_array_equal(oi.cpu().numpy(), feat[idx])


def test_input_layouts(seeded224):
    from tennis_amd import weights as W
    S = seeded224
    enc, frames = S["enc"], S["frames"][::8]           # 32 frames, every family
    u8 = enc(torch.from_numpy(np.ascontiguousarray(frames)).cuda()).cpu().numpy()
    x32 = W.normalize_to_nchw_f32(frames)
    f32 = enc(torch.from_numpy(x32).cuda()).cpu().numpy()
    assert np.abs(u8 - f32).max() <= 1e-6, np.abs(u8 - f32).max()
    x16 = torch.from_numpy(np.ascontiguousarray(x32.transpose(0, 2, 3, 1))).half()
    f16 = enc(x16.cuda()).cpu().numpy()
    from oracle.torch_ref import TorchDenseNet121
    ref16 = TorchDenseNet121(S["p"])(x16.float().permute(0, 3, 1, 2).contiguous()).numpy()
    assert np.abs(f16 - ref16).max() < BAR, np.abs(f16 - ref16).max()


def test_abi_flags_and_refusals(seeded224):
    from tennis_amd import _lib
    ctx = _lib.default_context()
    lib = ctx.lib
    arr, keep = _lib.make_params(seeded224["p"])
    h = C.c_void_p()
    for flags in (_lib.ENC_FP32, _lib.ENC_FP32 | _lib.ENC_EXACT_WEIGHTS):
        assert lib.tn_densenet121_create_ex(ctx.handle, arr, len(arr), b"densenet0_", 224, 224, 2, flags, C.byref(h)) == 0
        assert lib.tn_densenet121_feature_dim(h) == 1024
        assert lib.tn_densenet121_destroy(h) == 0
    for flags in (2, 6):
        assert lib.tn_densenet121_create_ex(ctx.handle, arr, len(arr), b"densenet0_", 224, 224, 2, flags, C.byref(h)) != 0
        assert b"unknown flag" in lib.tn_last_error()
    enc, x = seeded224["enc"], seeded224["x"]
    enc(x[:2])
    with pytest.raises(RuntimeError, match="fp32"):
        enc.input_means(x[:1])
    with pytest.raises(RuntimeError, match="fp32"):          # chosen behaviour: the taps are fp16 maps, this mode has none
        enc.read_tap("pool0", 1)
    del keep


def test_framemodel_on_get_model_fp32():
    from oracle.torch_ref import TorchDenseNet121
    from tennis_amd import weights as W
    from tennis_amd.model_zoo import get_model
    from tennis_amd.models.vision.definitions import FrameModel
    feats = get_model("DenseNet121", pretrained=False, conversion="fp32").features
    m = FrameModel(feats, 11)
    frames, _ = PT.batch(6, seed=3)
    logits = m(torch.from_numpy(frames).cuda()).cpu().numpy()
    bb = {k: v.data for k, v in feats._own_params.items()}
    ref = TorchDenseNet121(bb, prefix=feats.prefix)(torch.from_numpy(W.normalize_to_nchw_f32(frames))).numpy()
    cls = m.classes._own_params
    ref_logits = ref.astype(np.float64) @ cls[m.classes.prefix + "weight"].data.T.astype(np.float64) + cls[m.classes.prefix + "bias"].data
    assert np.abs(logits - ref_logits).max() < BAR, np.abs(logits - ref_logits).max()
