"""-m gpu: end-to-end fine-tuning step of the frame classifier (DenseNet-121 + Dense, BatchNorm in training mode, softmax CE,
SGD) through the C ABI vs oracle/densenet_train_torch.py (torch autograd on the CPU, float64)."""
import os

import numpy as np
import pytest
import torch

from oracle import densenet_train_torch as dt
from oracle import train_np as tn

pytestmark = pytest.mark.gpu

STOCK_BNS = ("densenet0_batchnorm0", "densenet0_stage1_batchnorm1", "densenet0_stage3_batchnorm47", "densenet0_batchnorm4")
TIGHT_GRADS = ("framemodel0_dense0_weight", "framemodel0_dense0_bias", "densenet0_stage4_conv31_weight", "densenet0_stage4_conv30_weight")


def _cap_threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def _setup(B, size=224, seed=5):
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(0)
    p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(B, size, seed))
    y = np.random.default_rng(seed).integers(0, 11, B).astype(np.int32)
    return p, x, y


def _compare(tr, rg):
    """per parameter: max-abs error relative to the largest reference entry (floored at 1e-3 of the largest gradient entry
    of the whole model: gradients that are analytically ~0, e.g. a BatchNorm shift in front of another training-mode
    BatchNorm with every ReLU open, are pure rounding noise) and cosine similarity of the non-negligible ones"""
    floor = 1e-3 * max(np.abs(g).max() for g in rg.values())
    worst, worst_k, min_cos = 0.0, None, 1.0
    for k, g in rg.items():
        got = tr.get(k, gradient=True).astype(np.float64)
        err = np.abs(got - g).max() / max(floor, np.abs(g).max())
        if np.abs(g).max() > floor:
            min_cos = min(min_cos, float((got * g).sum() / max(1e-30, np.linalg.norm(got) * np.linalg.norm(g))))
        if err > worst:
            worst, worst_k = err, k
    return worst, worst_k, min_cos


def test_every_operator_backward_exact_with_open_relus(report):
    """All 364 gradients against autograd with the BatchNorm shifts raised by +4, so that (almost) no ReLU input lies near
    zero: float32 and float64 then take the same ReLU branches and every convolution / BatchNorm / pooling backward must agree
    to rounding.  (With the stock parameters a handful of the ~5 M ReLU inputs fall within float32 rounding of zero and
    take the other branch than in float64 — with 2 frames a single such element moves a 7x7-stage gradient by percents —
    which is a property of the comparison, not of either implementation; see the next test.)"""
    from tennis_amd.engine import FrameModelTrainer
    B = 2
    p, x, y = _setup(B)
    p = {k: (v + 4.0).astype(np.float32) if k.endswith("_beta") else v for k, v in p.items()}
    tr = FrameModelTrainer(p, 224, 11, batch=B)
    loss, logits = tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    rl, rlog, rg, rstats = dt.loss_and_grads(p, x, y)
    assert np.abs(logits.cpu().numpy() - rlog).max() < 1e-3 * max(1.0, np.abs(rlog).max())
    worst, worst_k, min_cos = _compare(tr, rg)
    report["finetune_open_relu_grad_rel_err_worst"] = float(worst)
    assert worst < 2e-3 and min_cos > 0.999999, (worst_k, worst, min_cos)


def _stock_checks(report, tag, size, B, seed=5, tight=TIGHT_GRADS):
    """the stock-parameter step at (size, B) against autograd: logits and loss, the batch statistics of four BatchNorms, the
    classifier and last-layer gradients, every gradient's worst error and cosine, a running statistic"""
    from tennis_amd.engine import FrameModelTrainer
    _cap_threads()
    p, x, y = _setup(B, size, seed)
    tr = FrameModelTrainer(p, size, 11, batch=B)
    loss, logits = tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    rl, rlog, rg, rstats = dt.loss_and_grads(p, x, y)
    el = float(np.abs(logits.cpu().numpy() - rlog).max())
    report[f"finetune{tag}_logits_maxabs_err"] = el
    assert el < 1e-4 and np.abs(loss.cpu().numpy() - rl).max() < 1e-4, (el, loss.cpu().numpy(), rl)
    for bn in STOCK_BNS:
        c = rstats[bn][0].shape[0]
        em = np.abs(tr.get(bn + "_batch_mean", shape=(c,)) - rstats[bn][0]).max() / max(1.0, np.abs(rstats[bn][0]).max())
        ev = np.abs(tr.get(bn + "_batch_var", shape=(c,)) - rstats[bn][1]).max() / max(1.0, np.abs(rstats[bn][1]).max())
        report[f"finetune{tag}_{bn}_stats_err"] = float(max(em, ev))
        assert em < 1e-4 and ev < 1e-4, (bn, em, ev)
    # the classifier and the last layers' convolutions see no ReLU decision upstream of them: tight
    for k in tight:
        g = rg[k]
        assert np.abs(tr.get(k, gradient=True) - g).max() < 1e-4 * np.abs(g).max(), k
    worst, worst_k, min_cos = _compare(tr, rg)
    report[f"finetune{tag}_grad_rel_err_worst"] = float(worst)
    report[f"finetune{tag}_grad_min_cosine"] = float(min_cos)
    assert min_cos > 0.995 and worst < 0.3, (worst_k, worst, min_cos)     # a few float32 / float64 ReLU branch differences
    # running statistics: 0.9 * old + 0.1 * batch
    bn = "densenet0_stage2_batchnorm3"
    exp = 0.9 * p[bn + "_running_mean"] + 0.1 * rstats[bn][0]
    assert np.abs(tr.get(bn + "_running_mean") - exp).max() < 1e-4


def test_training_forward_backward_matches_autograd(report):
    _stock_checks(report, "", 224, 2)


def test_training_step_at_512_matches_autograd(report):
    """the reference's training frame size (train.py data_shape=512): maps of 256 ... 16, a 256-pixel head average, and split-K
    in blocks 2 and 3 as well"""
    # The last layer's convolutions sit behind ReLUs (conv31 behind the head's BatchNorm + ReLU, conv30 also behind layer 15's BN2 +
    # ReLU); with 1024 rows per channel a ReLU input within float32 rounding of 0 is no longer rare, and one such element moves a
    # whole channel's gradient through the BatchNorm backward's sums (the first test's docstring).  The float32 run of this very
    # oracle is 1.2e-2 of the largest entry off float64 on conv30.  So at 512x512 only the classifier is held to 1e-4.
    _stock_checks(report, "_512x4", 512, 4, tight=TIGHT_GRADS[:2])


def test_training_step_at_batch_32_matches_autograd(report):
    """224x224 with 32 frames: 32x as many rows per BatchNorm as the 2-frame test, split-K in blocks 2 and 3"""
    _stock_checks(report, "_224x32", 224, 32)


def test_every_operator_backward_exact_with_open_relus_at_512(report):
    """the open-ReLU comparison of the first test at 512x512 with 4 frames, with its bars.  The shifts are raised by +8, not +4: a
    BatchNorm here normalises 16x as many rows, and 4 standard deviations below the mean are no longer empty"""
    from tennis_amd.engine import FrameModelTrainer
    _cap_threads()
    B = 4
    p, x, y = _setup(B, 512)
    p = {k: (v + 8.0).astype(np.float32) if k.endswith("_beta") else v for k, v in p.items()}
    tr = FrameModelTrainer(p, 512, 11, batch=B)
    loss, logits = tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    rl, rlog, rg, rstats = dt.loss_and_grads(p, x, y)
    assert np.abs(logits.cpu().numpy() - rlog).max() < 1e-3 * max(1.0, np.abs(rlog).max())
    worst, worst_k, min_cos = _compare(tr, rg)
    report["finetune_512x4_open_relu_grad_rel_err_worst"] = float(worst)
    report["finetune_512x4_open_relu_grad_min_cosine"] = float(min_cos)
    assert worst < 2e-3 and min_cos > 0.999999, (worst_k, worst, min_cos)


def test_training_step_at_the_driver_default_512x64(report):
    """train.py's defaults (data_shape=512, batch_size=64): 64 * 256 * 256 stem rows, 65,536 row tiles of the stem GEMM, split-K
    in every block.  A float64 oracle of the whole step does not fit a host, so: the stem BatchNorm's batch statistics against
    float64 recomputed from the input (a missing stem row range shows here), finite gradients, the loss against the float64
    cross-entropy of the returned logits, bit-identical gradients from two identical calls, and one SGD step."""
    import torch.nn.functional as F
    from tennis_amd.engine import FrameModelTrainer
    _cap_threads()
    B, size = 64, 512
    p, x, y = _setup(B, size, seed=13)
    tr = FrameModelTrainer(p, size, 11, batch=B)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    loss, logits = tr.forward_backward(xd, yd)
    g1 = tr.grads.clone()
    assert bool(torch.isfinite(g1).all())
    # the stem's batch statistics in float64, frame by frame
    w0 = torch.from_numpy(p["densenet0_conv0_weight"]).double()
    z = torch.cat([F.conv2d(torch.from_numpy(x[b:b + 8]).double(), w0, stride=2, padding=3) for b in range(0, B, 8)])
    mean = z.mean(dim=(0, 2, 3)).numpy()
    var = z.var(dim=(0, 2, 3), unbiased=False).numpy()
    del z
    bn = "densenet0_batchnorm0"
    em = np.abs(tr.get(bn + "_batch_mean", shape=(64,)) - mean).max() / max(1.0, np.abs(mean).max())
    ev = np.abs(tr.get(bn + "_batch_var", shape=(64,)) - var).max() / max(1.0, np.abs(var).max())
    report["finetune_512x64_batchnorm0_stats_err"] = float(max(em, ev))
    assert em < 1e-4 and ev < 1e-4, (em, ev)
    # the loss: float64 softmax cross-entropy of the logits the step returned
    lg = logits.cpu().numpy().astype(np.float64)
    mx = lg.max(1, keepdims=True)
    ref = (np.log(np.exp(lg - mx).sum(1)) + mx[:, 0]) - lg[np.arange(B), y]
    el = np.abs(loss.cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max())
    report["finetune_512x64_loss_err"] = float(el)
    assert np.isfinite(lg).all() and el < 1e-5, el
    # a second identical call: split-K slices and BatchNorm reduction slices are summed in a fixed order
    tr.forward_backward(xd, yd)
    assert torch.equal(g1.view(torch.int32), tr.grads.view(torch.int32)), "gradients differ between two identical calls"
    # one SGD step on the library's own gradients
    names = ["framemodel0_dense0_weight", "densenet0_stage2_conv5_weight", "densenet0_conv0_weight", "densenet0_stage4_batchnorm7_gamma"]
    g0 = {k: tr.get(k, gradient=True) for k in names}
    tr.step(B, 0.01, 0.9, 1e-4)
    p1, _ = tn.sgd_momentum({k: p[k].astype(np.float64) for k in names}, g0, {}, 0.01, 0.9, 1e-4, 1.0 / B)
    for k in names:
        assert np.abs(tr.get(k) - p1[k]).max() < 1e-6 * max(1.0, np.abs(p1[k]).max()), k


def test_sgd_steps_reduce_the_loss():
    """A few steps of train.py's recipe (momentum 0.9, wd 1e-4, rescale 1/batch) on one fixed batch; the first update is
    oracle/train_np.py::sgd_momentum applied to the library's own gradients."""
    from tennis_amd.engine import FrameModelTrainer
    B = 4
    p, x, y = _setup(B, seed=9)
    tr = FrameModelTrainer(p, 224, 11, batch=B)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    loss, _ = tr.forward_backward(xd, yd)
    first = float(loss.mean())
    names = ["framemodel0_dense0_weight", "densenet0_stage2_conv5_weight", "densenet0_conv0_weight", "densenet0_stage4_batchnorm7_gamma"]
    g0 = {k: tr.get(k, gradient=True) for k in names}
    tr.step(B, 0.01, 0.9, 1e-4)
    p1, _ = tn.sgd_momentum({k: p[k].astype(np.float64) for k in names}, g0, {}, 0.01, 0.9, 1e-4, 1.0 / B)
    for k in names:
        assert np.abs(tr.get(k) - p1[k]).max() < 1e-6 * max(1.0, np.abs(p1[k]).max()), k
    for _ in range(12):
        loss, _ = tr.forward_backward(xd, yd)
        tr.step(B, 0.01, 0.9, 1e-4)
    assert float(loss.mean()) < 0.7 * first and bool(torch.isfinite(tr.grads).all())


def test_train_model_driver_with_the_frame_classifier(tmp_path):
    """tennis_amd.train.train_model (reference train.py:388-499) drives the end-to-end classifier exactly as it drives the
    temporal head: LR schedule, metric updates, per-epoch parameter files that load back into a FrameModel."""
    from tennis_amd.engine import FrameModelTrainer
    from tennis_amd.metrics.vision import PRF1
    from tennis_amd.model_zoo import get_model
    from tennis_amd.models.vision.definitions import FrameModel
    from tennis_amd.train import Trainer, train_model
    B = 4
    p, x, y = _setup(B, seed=11)
    head = FrameModelTrainer(p, 224, 11, batch=B)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    tr = Trainer(head, "sgd", {"learning_rate": 0.01, "momentum": 0.9, "wd": 1e-4})
    metric = PRF1(label_names=[str(i) for i in range(11)])
    mirror = FrameModel(get_model("DenseNet121", pretrained=True, seed=5).features, 11, prefix="framemodel0_")
    mirror.initialize()
    mirror.classes._materialize(1024)
    hist = train_model(head, lambda: [(xd, yd)] * 3, [metric], tr, epochs=3, batch_size=B, lr_steps=(1, 2), lr_factor=0.75,
                       save_dir=str(tmp_path), log=lambda *_: None, model=mirror)
    assert len(hist) == 3 and hist[-1]["loss"] < hist[0]["loss"] and abs(hist[-1]["lr"] - 0.01 * 0.75 ** 2) < 1e-9
    from tennis_amd.params_io import is_mxnet_params
    assert is_mxnet_params(str(tmp_path / "0002.params"))    # train.py:497: the MXNet container with Gluon's structural names
    fm = FrameModel(get_model("DenseNet121", pretrained=True, seed=3).features, 11, prefix="framemodel0_")
    fm.initialize()
    fm.classes._materialize(1024)
    fm.load_parameters(str(tmp_path / "0002.params"))
    st = head.state_dict()
    for k in ("densenet0_stage3_conv7_weight", "densenet0_batchnorm2_running_var", "framemodel0_dense0_bias"):
        got = fm.collect_params()[k].data
        ref = st[k].astype(np.float16).astype(np.float32) if k.endswith("conv7_weight") else st[k]   # the served model rounds conv weights to fp16
        assert np.allclose(got, ref, atol=1e-6), k
    logits = fm(xd).cpu().numpy()                            # inference with the running statistics just trained
    assert logits.shape == (B, 11) and np.isfinite(logits).all()
