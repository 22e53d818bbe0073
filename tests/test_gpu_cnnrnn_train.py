"""-m gpu: the end-to-end CNN-RNN training step (tn_cnnrnn_trainer_*, engine.CNNRNNTrainer) against the float64 autograd oracle
tests/tools/cnnrnn_train_torch.py, its input-gradient kernel alone (tn_dbg_gemm_nn), the optimiser, the driver route
(train / evaluate --window N --temp_pool gru|lstm without --feats_model) and the ABI's refusals.  Method and bars are
tests/test_gpu_finetune.py's.  Every frame differs from every other, so a wrong frame order (b * steps + t) fails."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import train_np as tn
from tools import cnnrnn_train_torch as ct

pytestmark = pytest.mark.gpu

STOCK_BNS = ("densenet0_batchnorm0", "densenet0_stage1_batchnorm1", "densenet0_stage3_batchnorm47", "densenet0_batchnorm4")


def _cap_threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def _setup(B, T, cell="gru", size=224, seed=5, shift=0.0):
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(0)
    if shift:
        p = {k: (v + shift).astype(np.float32) if k.endswith("_beta") else v for k, v in p.items()}
    p.update(W.make_rnn_weights(2, cell, 1024, 128, f"cnnrnn0_{cell}0_"))
    p.update(W.make_dense_weights(1, 11, 256, "cnnrnn0_dense0_"))
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(B * T, size, seed))          # (B*T, 3, S, S), frame b*T + t
    y = np.random.default_rng(seed).integers(0, 11, B).astype(np.int32)
    return p, x, y


def _trainer(p, B, T, cell="gru", frozen=False, size=224):
    from tennis_amd.engine import CNNRNNTrainer
    return CNNRNNTrainer(p, size, 11, batch=B, steps=T, type=cell, freeze_backbone=frozen)


def _run(tr, x, y, B, T):
    xd = torch.from_numpy(x).cuda().reshape(B, T, *x.shape[1:])                      # (B, T, 3, S, S)
    loss, logits = tr.forward_backward(xd, torch.from_numpy(y).cuda())
    return loss.cpu().numpy(), logits.cpu().numpy()


def _compare(tr, rg):
    """max-abs error per parameter relative to its largest reference entry (floored at 1e-3 of the largest gradient of the whole
    model) and the smallest cosine of the non-negligible ones"""
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


# ---- dX = dGI W_ih alone ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [37, 512])
@pytest.mark.parametrize("K", [768, 1024])
@pytest.mark.parametrize("N", [1000, 1024, 4096])
def test_input_gradient_product_against_float64(report, M, K, N):
    from tennis_amd import _lib as L
    ctx = L.default_context()
    g = torch.Generator(device="cuda")
    g.manual_seed(M * 7 + K * 3 + N)
    A = torch.randn((M, K), generator=g, device="cuda")
    B = torch.randn((K, N), generator=g, device="cuda")
    out = torch.full((M, N), float("nan"), device="cuda")
    L.check(ctx.lib.tn_dbg_gemm_nn(ctx.handle, L.ptr(A), K, L.ptr(B), N, L.ptr(out), N, M, N, K), "tn_dbg_gemm_nn")
    a, b = A.cpu().numpy().astype(np.float64), B.cpu().numpy().astype(np.float64)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    rel = np.abs(got - a @ b) / (np.abs(a) @ np.abs(b))
    report["gemm_nn_rel_err_worst"] = max(float(rel.max()), report.get("gemm_nn_rel_err_worst", 0.0))
    assert rel.max() < 2e-6, (M, K, N, float(rel.max()))


# ---- the step against autograd ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_step_exact_with_open_relus(report, cell):
    """every backbone and head gradient with the BatchNorm shifts raised by +4 (no ReLU input near 0: float32 and float64 take the
    same branches), batch 2 x steps 3 at 224x224"""
    _cap_threads()
    B, T = 2, 3
    p, x, y = _setup(B, T, cell, shift=4.0)
    tr = _trainer(p, B, T, cell)
    loss, logits = _run(tr, x, y, B, T)
    rl, rlog, rg, _ = ct.loss_and_grads(p, x, y, T, cell)
    assert np.abs(logits - rlog).max() < 1e-3 * max(1.0, np.abs(rlog).max())
    assert len([k for k in rg if k.startswith("densenet0_")]) == 362 and len(rg) == 362 + 10
    worst, worst_k, min_cos = _compare(tr, rg)
    report[f"cnnrnn_{cell}_open_relu_grad_rel_err_worst"] = float(worst)
    report[f"cnnrnn_{cell}_open_relu_grad_min_cosine"] = float(min_cos)
    assert worst < 2e-3 and min_cos > 0.999999, (worst_k, worst, min_cos)


def test_stock_step_matches_autograd(report):
    _cap_threads()
    B, T = 2, 3
    p, x, y = _setup(B, T)
    tr = _trainer(p, B, T)
    loss, logits = _run(tr, x, y, B, T)
    rl, rlog, rg, rstats = ct.loss_and_grads(p, x, y, T)
    el = float(np.abs(logits - rlog).max())
    report["cnnrnn_stock_logits_maxabs_err"] = el
    assert el < 1e-4 and np.abs(loss - rl).max() < 1e-4, (el, loss, rl)
    for bn in STOCK_BNS:                                    # batch statistics over all 6 frames
        c = rstats[bn][0].shape[0]
        em = np.abs(tr.get(bn + "_batch_mean", shape=(c,)) - rstats[bn][0]).max() / max(1.0, np.abs(rstats[bn][0]).max())
        ev = np.abs(tr.get(bn + "_batch_var", shape=(c,)) - rstats[bn][1]).max() / max(1.0, np.abs(rstats[bn][1]).max())
        assert em < 1e-4 and ev < 1e-4, (bn, em, ev)
    for k, g in rg.items():
        if k.startswith("cnnrnn0_"):
            assert np.abs(tr.get(k, gradient=True) - g).max() < 1e-4 * np.abs(g).max(), k
    worst, worst_k, min_cos = _compare(tr, rg)
    report["cnnrnn_stock_grad_min_cosine"] = float(min_cos)
    assert min_cos > 0.995, (worst_k, worst, min_cos)
    for bn in ("densenet0_stage2_batchnorm3", "densenet0_batchnorm4"):
        for i, s in enumerate(("_running_mean", "_running_var")):
            exp = 0.9 * p[bn + s].astype(np.float64) + 0.1 * rstats[bn][i]
            assert np.abs(tr.get(bn + s) - exp).max() < 1e-4 * max(1.0, np.abs(exp).max()), (bn, s)


def test_frozen_step(report):
    """--freeze_backbone: the head's gradients against the oracle with detached features, the backbone bit-identical after step,
    its running statistics updated from the batch"""
    _cap_threads()
    B, T = 2, 3
    p, x, y = _setup(B, T)
    tr = _trainer(p, B, T, frozen=True)
    assert len(tr.grads) == 1
    loss, logits = _run(tr, x, y, B, T)
    rl, rlog, rg, rstats = ct.loss_and_grads(p, x, y, T, frozen=True)
    assert set(rg) == {k for k in p if k.startswith("cnnrnn0_")}
    assert np.abs(logits - rlog).max() < 1e-4 and np.abs(loss - rl).max() < 1e-4
    for k, g in rg.items():
        assert np.abs(tr.get(k, gradient=True) - g).max() < 1e-4 * np.abs(g).max(), k
    before = {k: tr.get(k) for k in tr.names if k.startswith("densenet0_") and "running" not in k}
    head_before = tr.get("cnnrnn0_dense0_weight")
    tr.step(B, 0.05, 0.9, 1e-4)
    for k, v in before.items():
        assert np.array_equal(tr.get(k), v), k
    assert not np.array_equal(tr.get("cnnrnn0_dense0_weight"), head_before)
    bn = "densenet0_stage2_batchnorm3"
    exp = 0.9 * p[bn + "_running_mean"].astype(np.float64) + 0.1 * rstats[bn][0]
    assert np.abs(tr.get(bn + "_running_mean") - exp).max() < 1e-4 * max(1.0, np.abs(exp).max())
    assert not np.array_equal(tr.get(bn + "_running_mean"), p[bn + "_running_mean"])


def test_three_sgd_steps_lower_the_loss_and_match_the_update():
    B, T = 2, 3
    p, x, y = _setup(B, T, seed=9)
    tr = _trainer(p, B, T)
    names = ["densenet0_conv0_weight", "densenet0_stage3_conv7_weight", "densenet0_batchnorm4_gamma", "cnnrnn0_gru0_l0_i2h_weight",
             "cnnrnn0_gru0_r0_h2h_bias", "cnnrnn0_dense0_weight"]
    lr, mom, wd = 0.02, 0.9, 1e-4
    w = {k: tr.get(k).astype(np.float64) for k in names}
    m = {}
    losses = []
    for _ in range(3):
        loss, _ = _run(tr, x, y, B, T)
        losses.append(float(loss.sum()))
        g = {k: tr.get(k, gradient=True).astype(np.float64) for k in names}
        tr.step(B, lr, mom, wd)
        w, m = tn.sgd_momentum(w, g, m, lr, mom, wd, 1.0 / B)
        for k in names:
            got = tr.get(k)
            assert np.abs(got - w[k]).max() < 1e-5 * max(1.0, np.abs(w[k]).max()), k
    loss, _ = _run(tr, x, y, B, T)
    losses.append(float(loss.sum()))
    assert losses[-1] < losses[0], losses


def test_uint8_and_nhwc_frames_give_the_nchw_result():
    from tennis_amd import weights as W
    B, T = 2, 3
    p, _, y = _setup(B, T)
    u8 = W.synthetic_frames_u8(B * T, 224, 5)
    x = W.normalize_to_nchw_f32(u8)
    a = _trainer(p, B, T)
    la, ga = _run(a, x, y, B, T)
    b = _trainer(p, B, T)
    lb, gb = b.forward_backward(torch.from_numpy(u8).cuda().reshape(B, T, 224, 224, 3), torch.from_numpy(y).cuda())
    assert np.abs(gb.cpu().numpy() - ga).max() < 1e-4
    c = _trainer(p, B, T)
    xn = torch.from_numpy(x).cuda().reshape(B, T, 3, 224, 224).permute(0, 1, 3, 4, 2).contiguous()
    lc, gc = c.forward_backward(xn, torch.from_numpy(y).cuda())
    assert np.array_equal(gc.cpu().numpy(), ga)


# ---- the driver ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pool,extra", [("gru", []), ("lstm", []), ("gru", ["--freeze_backbone"])])
def test_train_and_evaluate_on_frames(tmp_path, capsys, pool, extra):
    from tennis_amd import evaluate as ev, train as tr
    from tennis_amd import weights as W
    from tennis_amd.params_io import is_mxnet_params, load_mxnet_params
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    args = ["--root", root, "--frames_per_video", "8", "--data_shape", "224", "--model_id", "0007", "--window", "4", "--temp_pool", pool,
            "--epochs", "1", "--batch_size", "2", "--max_batches", "3", "--exp_root", exp] + extra
    assert tr.main(args) == 0
    d = tmp_path / "exp" / "0007"
    assert (d / "scores.txt").exists() and (d / "0000.params").exists()
    f0 = str(d / "0000.params")
    saved = load_mxnet_params(f0)
    assert is_mxnet_params(f0) and "td.model.0.weight" in saved and "rnn.l0_i2h_weight" in saved and "classes.weight" in saved
    assert saved["rnn.l0_i2h_weight"].shape == ((3 if pool == "gru" else 4) * 128, 1024)
    if extra:
        start = W.make_densenet121_weights(0, "densenet0_", fp16_model=True)
        assert np.array_equal(saved["td.model.0.weight"], start["densenet0_conv0_weight"])
        assert not np.array_equal(saved["td.model.1.running_mean"], start["densenet0_batchnorm0_running_mean"])
    capsys.readouterr()
    assert ev.main(["--root", root, "--frames_per_video", "8", "--data_shape", "224", "--model_id", "0007", "--window", "4",
                    "--temp_pool", pool, "--split", "val", "--batch_size", "2", "--exp_root", exp]) == 0
    out = capsys.readouterr().out
    assert "0000.params" in out and "[Finished]" in out
    if pool == "gru" and not extra:                      # a second run resumes after the newest NNNN.params
        assert tr.main(args[:args.index("--epochs")] + ["--epochs", "2"] + args[args.index("--epochs") + 2:]) == 0
        out = capsys.readouterr().out
        assert "Loaded model params" in out and "0000.params" in out and (d / "0001.params").exists()


# ---- ABI refusals ----------------------------------------------------------------------------------------------------------------

def test_abi_refusals():
    from tennis_amd import _lib as L
    ctx = L.default_context()
    lib = ctx.lib
    p, x, y = _setup(2, 3)
    arr, keep = L.make_params(p)
    h = C.c_void_p()

    def create(c=ctx.handle, params=arr, size=224, classes=11, batch=2, steps=3, out=C.byref(h)):
        return lib.tn_cnnrnn_trainer_create(c, L.RNN_GRU, params, len(arr), b"densenet0_", b"cnnrnn0_gru0_", b"cnnrnn0_dense0_",
                                            size, size, classes, batch, steps, 0, out)
    last = lambda: lib.tn_last_error().decode()                  # the whole message a refusal leaves, entry name included
    INV, FB = "invalid argument: ", "invalid argument: tn_cnnrnn_trainer_forward_backward: "
    assert create(c=None) == -1                                  # TN_ERR_INVALID
    assert last() == INV + "tn_cnnrnn_trainer_create: null argument"
    assert create(params=None) != 0
    assert last() == INV + "tn_cnnrnn_trainer_create: null argument"
    assert create(out=None) != 0
    assert last() == INV + "tn_cnnrnn_trainer_create: null argument"
    for size in (100, 0):
        assert create(size=size) != 0
        assert last() == INV + "tn_cnnrnn_trainer_create: frames must be square with a side divisible by 32"
    for classes in (0, -1):
        assert create(classes=classes) != 0
        assert last() == INV + "tn_cnnrnn_trainer_create: classes must be positive"
    assert create(batch=0) != 0
    assert last() == INV + "tn_cnnrnn_trainer_create: bad batch / steps"
    assert create(steps=0) != 0
    assert last() == INV + "tn_cnnrnn_trainer_create: bad batch / steps"
    assert create() == 0 and h.value
    xd = torch.from_numpy(x).cuda().permute(0, 2, 3, 1).contiguous()
    yd = torch.from_numpy(y).cuda()
    loss = torch.empty(2, device="cuda")
    try:
        assert lib.tn_cnnrnn_trainer_forward_backward(h, None, L.ptr(yd), 2, 3, 224, 224, L.ptr(loss), None) != 0
        assert last() == FB + "null argument"
        assert lib.tn_cnnrnn_trainer_forward_backward(h, L.ptr(xd), None, 2, 3, 224, 224, L.ptr(loss), None) != 0
        assert last() == FB + "null argument"
        assert lib.tn_cnnrnn_trainer_forward_backward(None, L.ptr(xd), L.ptr(yd), 2, 3, 224, 224, None, None) != 0
        assert last() == FB + "null argument"
        # frame counts that are not the handle's batch x steps (6 = 2 x 3)
        counts = FB + "batch and steps must equal the handle's (batch x steps frames, BatchNorm statistics over all)"
        assert lib.tn_cnnrnn_trainer_forward_backward(h, L.ptr(xd), L.ptr(yd), 1, 6, 224, 224, None, None) != 0
        assert last() == counts
        assert lib.tn_cnnrnn_trainer_forward_backward(h, L.ptr(xd), L.ptr(yd), 2, 2, 224, 224, None, None) != 0
        assert "batch and steps" in lib.tn_last_error().decode()
        assert last() == counts
        assert lib.tn_cnnrnn_trainer_forward_backward(h, L.ptr(xd), L.ptr(yd), 2, 3, 192, 192, None, None) != 0
        assert "frame size" in lib.tn_last_error().decode()
        assert last() == FB + "the frame size must equal the handle's"
        assert lib.tn_cnnrnn_trainer_buffers(None, None, None, None, None, None, None) != 0
        assert last() == INV + "tn_cnnrnn_trainer_buffers: null handle"
        assert lib.tn_cnnrnn_trainer_sgd_step(None, 0.1, 0.9, 0.0, 0.5) != 0
        assert last() == INV + "tn_cnnrnn_trainer_sgd_step: null handle"
        buf = (C.c_float * 4)()
        n = C.c_int64()
        # (a name with a part's prefix is that part's to refuse, under its own name)
        assert lib.tn_cnnrnn_trainer_read_param(h, b"densenet0_no_such", 0, buf, 4, C.byref(n)) != 0
        assert last() == INV + "tn_finetune_read_param: unknown parameter name"
        assert lib.tn_cnnrnn_trainer_read_param(h, b"cnnrnn0_dense0_bias", 0, buf, 4, C.byref(n)) != 0     # buffer too small
        assert last() == INV + "tn_head_read_param: host buffer too small"
        assert lib.tn_cnnrnn_trainer_read_param(h, b"cnnrnn0_dense0_bias", 0, None, 4, C.byref(n)) != 0
        assert last() == INV + "tn_cnnrnn_trainer_read_param: null argument"
        # a step after the refusals still runs
        assert lib.tn_cnnrnn_trainer_forward_backward(h, L.ptr(xd), L.ptr(yd), 2, 3, 224, 224, L.ptr(loss), None) == 0
        assert bool(torch.isfinite(loss).all())
    finally:
        assert lib.tn_cnnrnn_trainer_destroy(h) == 0
    assert lib.tn_cnnrnn_trainer_destroy(None) == 0
    # a missing parameter
    q = {k: v for k, v in p.items() if k != "cnnrnn0_gru0_r0_h2h_bias"}
    arr2, keep2 = L.make_params(q)
    h2 = C.c_void_p()
    assert lib.tn_cnnrnn_trainer_create(ctx.handle, L.RNN_GRU, arr2, len(arr2), b"densenet0_", b"cnnrnn0_gru0_", b"cnnrnn0_dense0_",
                                        224, 224, 11, 2, 3, 0, C.byref(h2)) != 0
    assert last() == "missing parameter: cnnrnn0_gru0_r0_h2h_bias"
    del keep, keep2
