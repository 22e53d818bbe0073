"""No GPU: the class activation maps' float64 reference (tests/tools/class_maps_ref.py) against the oracle's own network, the ABI
surface, the driver's flag with its refusals, the file format, and FrameModel's refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tools import class_maps_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def test_cam_sums_to_the_oracles_logits_on_its_own_network():
    """One 224 x 224 frame through oracle/densenet_np with the stage4 tap, the oracle's batchnorm / relu on it, and then
    bias + sum(cam) against vision_np.frame_model's logits.  The oracle works in fp32: its average of 49 terms and its 1024-term
    matrix product are within (1024 + 49 + 8) 2^-24 of T = |bias| + sum |W| A / 49, whatever order numpy sums in."""
    from oracle import densenet_np as dn, vision_np as vn
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(0)
    p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(1, 224))
    taps = {}
    feat = dn.densenet121_features(x, p, taps=taps)
    m = taps["stage4"]
    assert m.shape == (1, 7, 7, 1024)
    a = dn.relu(dn.batchnorm(m, p, "densenet0_batchnorm4"))
    wd, bias = p["framemodel0_dense0_weight"], p["framemodel0_dense0_bias"]
    ones, zeros = np.ones(1024), np.zeros(1024)
    cam = CR.cam_f64(a, ones, zeros, wd, 1, 1)                      # (A >= 0: the reference's ReLU leaves it alone)
    assert cam.shape == (1, 11, 7, 7)
    logits = vn.frame_model(x, p)
    assert logits.shape == (1, 11) and np.array_equal(logits, dn.dense(feat, p, "framemodel0_dense0_"))
    T = np.abs(bias) + CR.cam_f64(a, ones, zeros, np.abs(wd), 1, 1).sum((2, 3))
    err = np.abs(bias + cam.sum((2, 3)) - logits)
    assert np.all(err <= (1024 + 49 + 8) * U * T), (err.max(), T.min())
    assert np.abs(logits).max() > 1e-3                              # (something to compare)
    # the same from the raw tap with the BatchNorm folded to scale / shift, as the kernel gets it
    s = p["densenet0_batchnorm4_gamma"].astype(np.float64) / np.sqrt(p["densenet0_batchnorm4_running_var"].astype(np.float64) + dn.BN_EPS)
    t = p["densenet0_batchnorm4_beta"] - p["densenet0_batchnorm4_running_mean"] * s
    cam2 = CR.cam_f64(m, s, t, wd, 1, 1)
    assert np.abs(cam2 - cam).max() <= 64 * U * CR.cam_scale_f64(m, s, t, wd, 1, 1).max()
    # a wrong index is not within the bound: the weights of another class
    assert not np.all(np.abs(bias + np.roll(cam, 1, axis=1).sum((2, 3)) - logits) <= (1024 + 49 + 8) * U * T)


@pytest.mark.parametrize("H,PH", [(7, 1), (9, 1), (14, 2), (16, 2)])
def test_cam_reference_on_synthetic_maps(H, PH):
    """bias + sum(cam) is the head's logit in float64, on maps with a border no cell owns (9 x 9, 16 x 16: large values planted
    there), and every cell reads the weights of its own pool window in NCHW-flatten order."""
    c = CR.synthetic_case(100 + H, 2, H, H, 24, PH, PH, 5)
    cam = CR.cam_f64(c["m"], c["scale"], c["shift"], c["wd"], PH, PH)
    assert cam.shape == (2, 5, 7 * PH, 7 * PH)
    ref = CR.logits_f64(c["m"], c["scale"], c["shift"], c["wd"], c["bias"], PH, PH)
    T = np.abs(c["bias"]) + CR.cam_scale_f64(c["m"], c["scale"], c["shift"], c["wd"], PH, PH).sum((2, 3))
    assert np.all(np.abs(c["bias"] + cam.sum((2, 3)) - ref) <= 1e-12 * T)
    assert np.abs(cam).max() < 100.0                                # nothing of the planted border
    # one cell by hand
    y, x, k = 7 * PH - 1, 3, 2
    cell = (y // 7) * PH + (x // 7)
    a = np.maximum(c["m"][1, y, x].astype(np.float64) * c["scale"] + c["shift"], 0.0)
    want = (c["wd"][k].astype(np.float64).reshape(24, PH * PH)[:, cell] * a).sum() / 49.0
    assert abs(cam[1, k, y, x] - want) <= 1e-12 * max(1.0, abs(want))
    if PH > 1:      # the flatten order matters: NHWC-flatten weights give other maps
        wrong = c["wd"].reshape(5, 24, PH * PH).transpose(0, 2, 1).reshape(5, -1)
        assert np.abs(CR.cam_f64(c["m"], c["scale"], c["shift"], wrong, PH, PH) - cam).max() > 1e-3


def test_abi_surface():
    from tennis_amd import _lib
    pub = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    declared = _lib.declared_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("tn_densenet121_forward_class_maps", "tn_densenet121_class_map_dims"):
        assert re.search(r"^int %s\(" % name, pub, re.M), name
        assert name in declared and getattr(lib, name) is not None, name
    assert re.search(r"^int tn_dbg_class_maps\(", dbg, re.M)
    assert "tn_dbg_class_maps" not in pub
    assert "tn_dbg_class_maps" in declared and lib.tn_dbg_class_maps is not None


def test_save_cams_flag_and_refusals():
    from tennis_amd import evaluate as ev
    assert ev.build_parser().parse_args([]).save_cams is False
    assert ev.build_parser().parse_args(["--save_cams"]).save_cams is True
    for bad, why in ((["--window", "4", "--temp_pool", "gru"], "--window 4"), (["--feats_model", "0006"], "--feats_model"),
                     (["--temp_pool", "max"], "--temp_pool max"), (["--num_gpus", "2"], "--num_gpus 1")):
        with pytest.raises(SystemExit, match=why):
            ev.main(["--save_cams", "--root", "/nonexistent"] + bad)
    ev.check_save_cams(ev.build_parser().parse_args(["--window", "4"]))          # without the flag nothing is refused
    with pytest.raises(SystemExit, match="one rank"):
        ev.check_save_cams(ev.build_parser().parse_args(["--save_cams"]), world=2)


def test_load_cams_round_trips_the_savers_file(tmp_path):
    from tennis_amd import evaluate as ev
    rng = np.random.default_rng(5)
    n = 6
    cols = dict(cam=rng.normal(0, 1, (n, 7, 7)).astype(np.float32), pred=rng.integers(0, 11, n), label=rng.integers(0, 11, n),
                logit=rng.normal(0, 1, n).astype(np.float32), video=["V%03d" % (i // 3) for i in range(n)], frame=list(range(n)))
    path = str(tmp_path / "exp" / "0006" / "test_cams.npz")
    ev.save_cams(path, **cols)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["cam", "frame", "label", "logit", "pred", "video"]
        assert z["video"].dtype.kind == "U" and z["cam"].dtype == np.float32
    got = ev.load_cams(path)
    for k in ("cam", "pred", "label", "logit", "frame"):
        assert np.array_equal(got[k], np.asarray(cols[k])), k
    assert list(got["video"]) == cols["video"]
    with pytest.raises(ValueError, match="entries"):
        ev.save_cams(path, **{**cols, "pred": cols["pred"][:3]})
    np.savez(str(tmp_path / "other.npz"), cam=cols["cam"])
    with pytest.raises(ValueError, match="save_cams"):
        ev.load_cams(str(tmp_path / "other.npz"))


def test_frame_model_without_classes_refuses_return_cam():
    """raised before the GPU is touched: this test has none"""
    from tennis_amd.models.vision.definitions import FrameModel
    from tennis_amd.nn import DenseNet121Backbone
    m = FrameModel(DenseNet121Backbone(), num_classes=-1)
    with pytest.raises(ValueError, match="classes"):
        m.forward(np.zeros((1, 3, 224, 224), np.float32), return_cam=True)
    import inspect
    from tennis_amd.models.vision import definitions as D
    for cls in (D.CNNRNN, D.TemporalPooling):
        assert "return_cam" not in inspect.signature(cls.forward).parameters
