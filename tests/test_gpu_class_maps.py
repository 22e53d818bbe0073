"""-m gpu: the class activation maps of the frame classifier (csrc/class_maps.hip, tn_densenet121_forward_class_maps).

1. class_maps_kernel alone through tn_dbg_class_maps, both map formats, against float64 (tests/tools/class_maps_ref.py).  Bound, derived:
     |out - ref| <= (n_seq + d + 4) 2^-24 S,   S = (1/49) sum_k |Wd| (|scale v| + |shift|) of that cell
   n_seq = 8 ceil(C / 512): a lane owns the 8-channel chunks l, l + 64, ... and accumulates them one fma after the other;
   d = 6: the xor butterfly over the 64 lanes; + 4: the BatchNorm fma, the constant 1/49, the multiplication by it, one spare.
2. Through the encoder in every mode and every way forward splits a batch: the sum identity against the same call's logits,
   bit-identity of features / logits / maps across the splits, and the fp32 oracle within the project's 1e-3.
3. FrameModel.forward(return_cam=True), evaluate --save_cams, and the entry point's refusals."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tools import class_maps_ref as CR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DEPTH = 6                      # class_maps.hip: kClassMapsDepth, the butterfly 32, 16, 8, 4, 2, 1
BAR = 1e-3                     # the project's bar for this model's features and logits


def n_seq(C_):
    return 8 * -(-C_ // 512)   # class_maps.hip: class_maps_seq


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------
MAPS = [(1, 7, 7, 8, 1), (3, 7, 7, 64, 1), (2, 9, 9, 72, 1), (2, 16, 16, 1024, 2), (5, 14, 14, 136, 2)]      # B, H, W, C, PH = PW


@functools.lru_cache(maxsize=None)
def _case(shape, x32):
    """the case with 64 classes and its float64 maps, computed once; fewer classes read the first rows of the weights"""
    B, H, W, C_, P = shape
    c = CR.synthetic_case(B * 1000 + H * 10 + C_, B, H, W, C_, P, P, 64)
    c["x"] = c["m"] if x32 else c["m"].astype(np.float16)
    c["ref"] = CR.cam_f64(c["x"], c["scale"], c["shift"], c["wd"], P, P)
    c["S"] = CR.cam_scale_f64(c["x"], c["scale"], c["shift"], c["wd"], P, P)
    for v in c.values():
        v.setflags(write=False)                                 # shared among the cases: left unchanged
    return c


def _run_kernel(ctx, x, x32, scale, shift, wd, P, classes):
    from tennis_amd import _lib
    B, H, W, C_ = x.shape
    xd = torch.tensor(x, device="cuda")
    poison = torch.full((B, H, W, C_), float("nan"), dtype=torch.float16, device="cuda")
    sd, td, wdd = (torch.tensor(a, device="cuda") for a in (scale, shift, wd))
    out = torch.full((B, classes, 7 * P, 7 * P), float("nan"), dtype=torch.float32, device="cuda")
    ns, d = C.c_int(), C.c_int()
    _lib.check(ctx.lib.tn_dbg_class_maps(ctx.handle, _lib.ptr(poison if x32 else xd), _lib.ptr(xd if x32 else None), B, H, W, C_, _lib.ptr(sd),
                                         _lib.ptr(td), _lib.ptr(wdd), P, P, classes, _lib.ptr(out), C.byref(ns), C.byref(d)), "tn_dbg_class_maps")
    return out.cpu().numpy(), ns.value, d.value


@pytest.mark.parametrize("x32", [False, True], ids=["f16", "x32"])
@pytest.mark.parametrize("classes", [1, 11, 17, 64])
@pytest.mark.parametrize("shape", MAPS, ids=["x".join(map(str, s)) for s in MAPS])
def test_kernel_against_float64(ctx, report, shape, classes, x32):
    B, H, W, C_, P = shape
    c = _case(shape, x32)
    wd = np.ascontiguousarray(c["wd"][:classes])
    got, ns, d = _run_kernel(ctx, c["x"], x32, c["scale"], c["shift"], wd, P, classes)
    assert (ns, d) == (n_seq(C_), DEPTH)
    assert got.shape == (B, classes, 7 * P, 7 * P)               # cells outside every pool window do not exist
    assert np.all(np.isfinite(got))                             # every cell written, the poisoned fp16 map not read
    ref, S = c["ref"][:, :classes], c["S"][:, :classes]
    bound = (n_seq(C_) + DEPTH + 4) * U * S
    err = np.abs(got.astype(np.float64) - ref)
    key = "class_maps_%s_%s_c%d_err_over_bound" % ("x32" if x32 else "f16", "x".join(map(str, shape)), classes)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: %.3f (max err %.3g)" % (key, ratio, err.max()))
    report[key] = ratio
    assert np.all(err <= bound)
    assert np.abs(ref).max() > 100 * bound.max()                # (the bound discriminates)
    # bit-reproducible from run to run, and a frame's maps do not depend on the batch it came in
    again, _, _ = _run_kernel(ctx, c["x"], x32, c["scale"], c["shift"], wd, P, classes)
    assert np.array_equal(got, again)
    last, _, _ = _run_kernel(ctx, c["x"][B - 1:], x32, c["scale"], c["shift"], wd, P, classes)
    assert np.array_equal(got[B - 1:], last)


def test_kernel_refusals(ctx):
    from tennis_amd import _lib
    lib, h = ctx.lib, ctx.handle
    m = torch.zeros((1, 7, 7, 16), dtype=torch.float16, device="cuda")
    s = torch.zeros(16, dtype=torch.float32, device="cuda")
    w = torch.zeros((65, 16), dtype=torch.float32, device="cuda")
    out = torch.full((1, 65, 7, 7), 7.0, dtype=torch.float32, device="cuda")

    def refused(rc, word):
        msg = lib.tn_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    P = _lib.ptr
    refused(lib.tn_dbg_class_maps(h, P(m), None, 1, 7, 7, 16, P(s), P(s), P(w), 1, 1, 65, P(out), None, None), "[1, 64]")
    refused(lib.tn_dbg_class_maps(h, P(m), None, 1, 7, 7, 16, P(s), P(s), P(w), 1, 1, 0, P(out), None, None), "[1, 64]")
    refused(lib.tn_dbg_class_maps(h, P(m), None, 1, 7, 7, 12, P(s), P(s), P(w), 1, 1, 11, P(out), None, None), "multiple of 8")
    refused(lib.tn_dbg_class_maps(h, P(m), None, 1, 7, 7, 16, P(s), P(s), P(w), 2, 1, 11, P(out), None, None), "shape")
    refused(lib.tn_dbg_class_maps(h, None, None, 1, 7, 7, 16, P(s), P(s), P(w), 1, 1, 11, P(out), None, None), "null")
    refused(lib.tn_dbg_class_maps(h, P(m), None, 1, 7, 7, 16, P(s), P(s), None, 1, 1, 11, P(out), None, None), "null")
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)


# ---- 2. through the encoder --------------------------------------------------------------------------------------------------
MODES = {"default": dict(), "exact_weights": dict(exact_weights=True), "fp32": dict(fp32=True), "fp32x3": dict(fp32x3=True)}


@functools.lru_cache(maxsize=None)
def _weights(fp16_model):
    from tennis_amd import weights as W
    return W.make_densenet121_weights(0, fp16_model=fp16_model)


def _params(mode):
    """seeded weights: the default mode serves the fp16 model (its conversion is not the kernels' error), the others the fp32 parameters"""
    return _weights(mode == "default")


@functools.lru_cache(maxsize=None)
def _dense(dim):
    from tennis_amd import weights as W
    p = W.make_dense_weights(1, 11, dim, "framemodel0_dense0_")
    return p["framemodel0_dense0_weight"], p["framemodel0_dense0_bias"]


@functools.lru_cache(maxsize=None)
def _frames(n, size):
    from tennis_amd import weights as W
    return W.synthetic_frames_u8(n, size, seed=77 + size)


@functools.lru_cache(maxsize=None)
def _oracle(fp16_model, size, n):
    """the fp32 oracle's maps for the first n frames, once per weight set and size"""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    P = 1 if size == 224 else 2
    cam, feat = CR.oracle_cam(_params("default" if fp16_model else "fp32"), _frames(128 if size == 224 else 2, size)[:n], _dense(1024 * P * P)[0], P, P)
    return cam, feat


class _Net:
    """an encoder of one mode with the Dense(11) behind it and the Dense(|W|, 0) of the identity's bound"""

    def __init__(self, mode, size, max_batch):
        from tennis_amd.engine import Dense, DenseNet121Features
        self.enc = DenseNet121Features(_params(mode), size, max_batch=max_batch, **MODES[mode])
        self.wd, self.bias = _dense(self.enc.feature_dim)
        self.cls = Dense(self.wd, self.bias)
        self.cls_abs = Dense(np.abs(self.wd), np.zeros_like(self.bias))
        self.P = self.enc.class_map_dims[0] // 7

    def maps(self, x, cls=None):
        """-> features, logits, maps as numpy, from ONE call (the logits through the Dense from that call's features)"""
        f, m = self.enc(x, class_maps=self.cls if cls is None else cls)
        return f.cpu().numpy(), self.cls(f).cpu().numpy(), m.cpu().numpy()

    def check_identity(self, x, logits, cam, report, key):
        _, _, cam_abs = self.maps(x, self.cls_abs)
        assert np.all(cam_abs >= 0)
        T = np.abs(self.bias)[None] + cam_abs.astype(np.float64).sum((2, 3))
        F = self.enc.feature_dim
        bound = (F + 98 * self.P * self.P + 64) * U * T
        err = np.abs(self.bias[None].astype(np.float64) + cam.astype(np.float64).sum((2, 3)) - logits)
        ratio = float((err / bound).max())
        print("%s: identity err / bound %.4f (max err %.3g)" % (key, ratio, err.max()))
        report[key + "_identity_err_over_bound"] = ratio
        assert np.all(err <= bound), (key, ratio)


@functools.lru_cache(maxsize=None)
def _net(mode, size):
    return _Net(mode, size, 128 if size == 224 else 2)


def _check_oracle(net, mode, size, cam, n, report):
    ref, _ = _oracle(mode == "default", size, n)
    assert ref.shape == cam[:n].shape
    worst = float(np.abs(cam[:n].astype(np.float64) - ref).max())
    print("class_maps %s %d: max |cell - fp32 oracle| = %.3g" % (mode, size, worst))
    report["class_maps_%s_%d_cell_vs_oracle_max" % (mode, size)] = worst
    assert worst < BAR, (mode, size, worst)


@pytest.mark.parametrize("mode", list(MODES))
def test_encoder_maps_224_every_split(mode, report):
    net = _net(mode, 224)
    enc = net.enc
    assert enc.class_map_dims == (7, 7) and enc.feature_dim == 1024
    # 64 frames twice: the two half-batch ranges of the 128-frame call get the same frames
    x128 = torch.from_numpy(np.concatenate([_frames(128, 224)[:64]] * 2)).cuda()
    # B = 1, 3: one range on the caller's stream
    for B in (1, 3):
        x = x128[:B]
        f, lg, cam = net.maps(x)
        assert cam.shape == (B, 11, 7, 7)
        assert np.array_equal(f, enc(x).cpu().numpy())                       # features bit-identical to forward(x)
        assert np.array_equal(lg, net.cls(enc(x)).cpu().numpy())
        net.check_identity(x, lg, cam, report, "class_maps_%s_224_b%d" % (mode, B))
        if B == 3:
            for i in range(3):                                                 # the same frames one by one
                fi, _, cami = net.maps(x[i:i + 1])
                assert np.array_equal(cami[0], cam[i]) and np.array_equal(fi[0], f[i])
            _check_oracle(net, mode, 224, cam, 3, report)
    # B = 128: two half-batch ranges on the side streams ...
    f, lg, cam = net.maps(x128)
    f_plain = enc(x128).cpu().numpy()
    assert np.array_equal(f, f_plain)
    net.check_identity(x128, lg, cam, report, "class_maps_%s_224_b128" % mode)
    # ... and a frame's maps do not know which range it ran in, at which offset it was written, on which stream.  (Against the
    # one-by-one calls above only the maps' source differs: forward picks other kernels for the dense blocks from 64 frames per
    # range on, and the features differ in the same last bits.)
    assert np.array_equal(cam[:64], cam[64:]) and np.array_equal(f[:64], f[64:])
    assert np.abs(cam[1] - cam[0]).max() > 1e-4                                # (64 different frames)
    # ... pipelined: whole batches on alternating side streams and workspace sets, two calls in flight, ordered by join
    xb = torch.flip(x128, dims=[0]).contiguous()
    enc.set_pipelined(True)
    try:
        fa, ma = enc(x128, class_maps=net.cls)
        fb, mb = enc(xb, class_maps=net.cls)
        enc.join(1)
        fa_h, ma_h = fa.cpu().numpy(), ma.cpu().numpy()
        enc.join(0)
        fb_h, mb_h = fb.cpu().numpy(), mb.cpu().numpy()
    finally:
        enc.set_pipelined(False)
    assert np.array_equal(fa_h, f) and np.array_equal(ma_h, cam)
    assert np.array_equal(fb_h, f[::-1]) and np.array_equal(mb_h, cam[::-1])
    # and a forward without maps behind all that is the forward it always was
    assert np.array_equal(enc(x128).cpu().numpy(), f_plain)


@pytest.mark.parametrize("mode", ["default", "fp32"])
def test_encoder_maps_512(mode, report):
    net = _net(mode, 512)
    enc = net.enc
    assert enc.class_map_dims == (14, 14) and enc.feature_dim == 4096
    x = torch.from_numpy(_frames(2, 512)).cuda()
    f, lg, cam = net.maps(x)
    assert cam.shape == (2, 11, 14, 14)
    assert np.array_equal(f, enc(x).cpu().numpy())
    net.check_identity(x, lg, cam, report, "class_maps_%s_512_b2" % mode)
    for i in range(2):
        _, _, cami = net.maps(x[i:i + 1])
        assert np.array_equal(cami[0], cam[i])
    _check_oracle(net, mode, 512, cam, 2, report)


# ---- 3. surface ------------------------------------------------------------------------------------------------------------
def test_frame_model_return_cam():
    from tennis_amd.model_zoo import get_model
    from tennis_amd.models.vision.definitions import FrameModel
    model = FrameModel(get_model("DenseNet121", pretrained=True).features, 11)
    model.initialize()
    x = _frames(128, 224)[:5]
    logits, cam = model(x, return_cam=True)
    assert tuple(logits.shape) == (5, 11) and tuple(cam.shape) == (5, 11, 7, 7) and cam.dtype == torch.float32
    assert torch.equal(logits, model(x))                                       # bit-identical to forward(x)
    assert torch.equal(logits, model.forward(x, return_cam=False))
    # the identity, with T = |bias| + sum_k |W| feature[k] (= sum over the cells of the maps of |W|: A >= 0)
    own = model.classes._own_params
    wd, bias = (np.asarray(own[model.classes.prefix + k].data, np.float64) for k in ("weight", "bias"))
    T = np.abs(bias)[None] + model.backbone(x).cpu().numpy().astype(np.float64) @ np.abs(wd).T
    err = np.abs(bias[None] + cam.cpu().numpy().astype(np.float64).sum((2, 3)) - logits.cpu().numpy())
    assert np.all(err <= (1024 + 98 + 64) * U * T), float((err / T).max())
    with pytest.raises(ValueError, match="classes"):
        FrameModel(model.backbone, -1)(x, return_cam=True)


def test_evaluate_save_cams(tmp_path, monkeypatch, capsys):
    from tennis_amd import engine, evaluate as ev
    from tools import tiny_dataset
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    tiny_dataset.write(root, np.random.default_rng(3))
    seen = {}
    plain, with_cams = ev.evaluate_model, ev.evaluate_model_cams

    def rec_plain(net, *a, **k):
        seen["plain"] = plain(net, *a, **k)
        return seen["plain"]

    def rec_cams(net, *a, **k):
        seen["cams"] = with_cams(net, *a, **k)
        seen["net"] = net
        return seen["cams"]
    feats, call = [], engine.DenseNet121Features.__call__

    def rec_features(self, x, out=None, class_maps=None):
        r = call(self, x, out=out, class_maps=class_maps)
        if class_maps is not None:
            feats.append(r[0].cpu().numpy())
        return r
    monkeypatch.setattr(engine.DenseNet121Features, "__call__", rec_features)
    monkeypatch.setattr(ev, "evaluate_model", rec_plain)
    monkeypatch.setattr(ev, "evaluate_model_cams", rec_cams)
    args = ["--root", root, "--model_id", "0006", "--split", "test", "--batch_size", "5", "--exp_root", exp, "--num_workers", "0"]

    def metrics(out):
        lines = out.splitlines()
        i = lines.index("Test set:")
        fin = [ln for ln in lines if ln.startswith("[Finished]")]
        assert len(fin) == 1
        return lines[i:i + 12], fin[0].split("  # Samples")[0]
    assert ev.main(args) == 0
    m_plain = metrics(capsys.readouterr().out)
    assert not os.path.exists(os.path.join(exp, "0006", "test_cams.npz"))
    assert ev.main(args + ["--save_cams"]) == 0
    m_cams = metrics(capsys.readouterr().out)
    assert m_plain == m_cams                                                    # the run's metrics are those of the run without the flag
    res_p, gt_p = seen["plain"]
    res_c, gt_c, _ = seen["cams"]
    assert list(res_p) == list(res_c) and gt_p == gt_c
    logits = np.stack([res_c[k] for k in res_c])
    assert np.array_equal(logits, np.stack([res_p[k] for k in res_p]))           # the same logits, bit for bit
    d = ev.load_cams(os.path.join(exp, "0006", "test_cams.npz"))
    n = len(res_c)
    assert n == 12 and d["cam"].shape == (n, 7, 7) and d["cam"].dtype == np.float32
    assert np.array_equal(d["pred"], logits.argmax(1))
    assert np.array_equal(d["logit"], logits[np.arange(n), d["pred"]])
    assert np.array_equal(d["label"], np.array([gt_c[k] for k in res_c]))
    assert list(d["video"]) == ["V012"] * n and list(d["frame"]) == list(range(n))
    # cam.sum + bias[pred] = logit within the identity's bound, T = |bias| + sum_k |W[pred, k]| feature[k]: what the maps of |W| sum
    # to over the cells (A >= 0), from the features of the same forwards
    net = seen["net"]
    own = net.classes._own_params
    wd, bias = (np.asarray(own[net.classes.prefix + k].data, np.float64) for k in ("weight", "bias"))
    feat = np.concatenate(feats).astype(np.float64)
    assert wd.shape == (11, 1024) and feat.shape == (n, 1024)
    T = np.abs(bias[d["pred"]]) + (np.abs(wd[d["pred"]]) * feat).sum(1)
    err = np.abs(d["cam"].astype(np.float64).sum((1, 2)) + bias[d["pred"]] - d["logit"])
    assert np.all(err <= (1024 + 98 + 64) * U * T), float((err / T).max())


def test_entry_point_refusals(ctx):
    from tennis_amd import _lib
    from tennis_amd.engine import Dense
    net = _net("default", 224)
    enc, lib = net.enc, ctx.lib
    x = torch.from_numpy(_frames(128, 224)[:2]).cuda()
    feat = torch.full((2, 1024), 5.0, dtype=torch.float32, device="cuda")
    maps = torch.full((2, 11, 7, 7), 5.0, dtype=torch.float32, device="cuda")
    P, U8 = _lib.ptr, _lib.LAYOUT_NHWC_U8

    def refused(rc, word):
        msg = lib.tn_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    fn = lib.tn_densenet121_forward_class_maps
    refused(fn(None, P(x), U8, 2, P(feat), net.cls.handle, P(maps)), "encoder")
    refused(fn(enc.handle, None, U8, 2, P(feat), net.cls.handle, P(maps)), "x is null")
    refused(fn(enc.handle, P(x), U8, 2, None, net.cls.handle, P(maps)), "features is null")
    refused(fn(enc.handle, P(x), U8, 2, P(feat), None, P(maps)), "classes is null")
    refused(fn(enc.handle, P(x), U8, 2, P(feat), net.cls.handle, None), "maps is null")
    narrow = Dense(np.zeros((11, 512), np.float32), None)
    refused(fn(enc.handle, P(x), U8, 2, P(feat), narrow.handle, P(maps)), "in_units 512")
    wide = Dense(np.zeros((65, 1024), np.float32), None)
    refused(fn(enc.handle, P(x), U8, 2, P(feat), wide.handle, P(maps)), "65 units")
    other = Dense(net.wd, net.bias, ctx=_lib.Context(0))
    refused(fn(enc.handle, P(x), U8, 2, P(feat), other.handle, P(maps)), "another context")
    h, w = C.c_int(), C.c_int()
    refused(lib.tn_densenet121_class_map_dims(enc.handle, None, C.byref(w)), "null")
    torch.cuda.synchronize()
    assert torch.all(feat == 5.0) and torch.all(maps == 5.0)                  # a refused call launches nothing
    with pytest.raises(TypeError, match="engine.Dense"):
        enc(x, class_maps=net.wd)
