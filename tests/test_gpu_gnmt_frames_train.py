"""-m gpu: the frame-mode captioner training step (tn_gnmt_frames_trainer_*, engine.GNMTFramesTrainer) against the float64 autograd
oracle tests/tools/gnmt_frames_train_torch.py: the captioner's source gradient alone (tn_dbg_gnmt_trainer_src_grad), the whole step
with open ReLUs and with stock weights, the padded frame slots, the variable frame count, the frozen backbone, Adam over both
parts, the input layouts, the driver route (train_gnmt / evaluate_gnmt without --feats_model) and the ABI's refusals.  Method and
bars are those of tests/test_gpu_cnnrnn_train.py, tests/test_gpu_finetune.py and tests/test_gpu_gnmt_train.py.  Every frame
differs from every other, so a wrong frame order (b * steps + t) fails.  The oracle's steps are computed once and shared."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import gnmt_train_torch as gt
from tools import gnmt_frames_train_torch as ft

pytestmark = pytest.mark.gpu

STOCK_BNS = ("densenet0_batchnorm0", "densenet0_stage1_batchnorm1", "densenet0_stage3_batchnorm47", "densenet0_batchnorm4")
E, V, L = 6, 14, 6
SVL = (3, 2)              # batch 2 x steps 3: one padded slot, six frames


def _cap_threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def _targets(B, seed):
    rng = np.random.default_rng(seed)
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0] = 2
    tvl = rng.integers(3, L + 1, B).astype(np.int32)
    tvl[0] = L
    for b in range(B):
        tgt[b, tvl[b] - 1] = 3
        tgt[b, tvl[b]:] = 1
    return tgt, tvl


@functools.lru_cache(maxsize=None)
def _setup(cell="gru", H=8, shift=0.0, B=2, T=3, svl=SVL, seed=5):
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(0)
    if shift:
        p = {k: (v + shift).astype(np.float32) if k.endswith("_beta") else v for k, v in p.items()}
    p.update(W.make_gnmt_weights(seed, cell, 1024, H, E, V))
    p["gnmt_tgt_embed_weight"] = np.random.default_rng(seed).normal(0, 0.5, (V, E)).astype(np.float32)
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(B * T, 224, seed)).reshape(B, T, 3, 224, 224)
    tgt, tvl = _targets(B, seed)
    return p, x, np.array(svl, np.int32), tgt, tvl


@functools.lru_cache(maxsize=None)
def _oracle(cell="gru", H=8, shift=0.0, B=2, T=3, svl=SVL, seed=5):
    _cap_threads()
    p, x, s, tgt, tvl = _setup(cell, H, shift, B, T, svl, seed)
    return ft.loss_and_grads(p, x, s, tgt, tvl, H, cell=cell)


def _trainer(p, H, cell="gru", frozen=False, max_batch=2, max_src_len=3, max_frames=None):
    from tennis_amd.engine import GNMTFramesTrainer
    return GNMTFramesTrainer(p, H, E, V, size=224, max_batch=max_batch, max_src_len=max_src_len, max_tgt_len=L, max_frames=max_frames,
                             freeze_backbone=frozen, cell_type=cell)


def _run(tr, x, svl, tgt, tvl):
    loss, logits = tr.forward_backward(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(svl).cuda(),
                                       torch.from_numpy(tgt).cuda(), torch.from_numpy(tvl).cuda(), return_logits=True)
    return float(loss), logits.cpu().numpy()


def _compare(tr, rg):
    """max-abs error per parameter relative to its largest reference entry (floored at 1e-3 of the largest gradient of the whole
    model) and the smallest cosine of the non-negligible ones (tests/test_gpu_cnnrnn_train.py)"""
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


def _captioner_grad_err(tr, rg):
    """the captioner test's measure: per parameter, max-abs error relative to its largest reference entry"""
    worst, worst_k = 0.0, None
    for k, g in rg.items():
        if k.startswith("gnmt_"):
            err = np.abs(tr.get(k, gradient=True) - g).max() / max(1e-7, np.abs(g).max())
            if err > worst:
                worst, worst_k = float(err), k
    return worst, worst_k


# ---- 1. d loss / d src of the captioner step alone --------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [dict(seed=21, B=3, T=9, F=18, H=8, nl=2, nbi=1),
                                 dict(seed=22, B=3, T=9, F=18, H=8, nl=3, nbi=1, res=True),
                                 dict(seed=23, B=3, T=9, F=18, H=8, nl=2, nbi=0),
                                 dict(seed=24, B=3, T=9, F=18, H=8, nl=2, nbi=1, cell="lstm"),
                                 dict(seed=25, B=3, T=9, F=18, H=8, nl=3, nbi=1, res=True, cell="lstm"),
                                 dict(seed=26, B=3, T=9, F=18, H=8, nl=2, nbi=0, cell="lstm"),
                                 dict(seed=27, B=4, T=17, F=1024, H=128, nl=2, nbi=1)])          # K = 2 * 3 * 128 = 768, N = 1024
def test_source_gradient_against_autograd(report, cfg):
    """tn_dbg_gnmt_trainer_src_grad on random features, without dropout and with the trainer's own masks replayed by the oracle;
    rows at or past the valid length are exactly 0 (the buffer is handed over full of NaN)"""
    from tennis_amd import _lib as Lb
    from tennis_amd import weights as W
    from tennis_amd.engine import GNMTTrainer
    _cap_threads()
    cell, nl, nbi, res = cfg.get("cell", "gru"), cfg["nl"], cfg["nbi"], cfg.get("res", False)
    B, T, F, H = cfg["B"], cfg["T"], cfg["F"], cfg["H"]
    rng = np.random.default_rng(cfg["seed"])
    p = W.make_gnmt_weights(cfg["seed"], cell, F, H, E, V, num_layers=nl, num_bi_layers=nbi)
    p["gnmt_tgt_embed_weight"] = rng.normal(0, 0.5, (V, E)).astype(np.float32)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    svl = rng.integers(max(1, T // 2), T, B).astype(np.int32)
    svl[0] = T
    tgt, tvl = _targets(B, cfg["seed"])
    tr = GNMTTrainer(p, F, H, E, V, max_batch=B, max_src_len=T, max_tgt_len=L, cell_type=cell, num_layers=nl, num_bi_layers=nbi,
                     use_residual=res)
    sd, vd, td, ld = (torch.from_numpy(a).cuda() for a in (src, svl, tgt, tvl))
    loss = torch.empty(1, device="cuda")
    for p_drop in (0.0, 0.25):
        masks = None
        if p_drop:
            tr.set_dropout(p_drop, seed=3)
        d = torch.full((B, T, F), float("nan"), device="cuda")
        Lb.check(tr.lib.tn_dbg_gnmt_trainer_src_grad(tr.handle, Lb.ptr(sd), Lb.ptr(vd), Lb.ptr(td), L, Lb.ptr(ld), B, T, L, Lb.ptr(loss),
                                                     None, Lb.ptr(d), F), "tn_dbg_gnmt_trainer_src_grad")
        if p_drop:
            masks = {"enc": [tr.dropout_mask(i, (B, T, (2 if i < nbi else 1) * H)).cpu().numpy() for i in range(nl)],
                     "dec": {j: tr.dropout_mask(nl + j, (L - 1, B, H)).cpu().numpy() for j in range(1, nl)}}
        rl, _, rg, rd = ft.captioner_loss_and_grads(p, src, svl, tgt, tvl, H, cell=cell, masks=masks, num_layers=nl, num_bi_layers=nbi,
                                                    use_residual=res)
        got = d.cpu().numpy()
        assert np.isfinite(got).all()
        assert abs(float(loss) - rl) < 1e-4 * max(1.0, abs(rl))
        err = float(np.abs(got - rd).max() / max(1e-7, np.abs(rd).max()))
        report[f"gnmt_src_grad_{cell}_{nl}_{nbi}_{'res' if res else 'plain'}_H{H}_drop{p_drop}_rel_err"] = err
        assert err < 2e-3, (cfg, p_drop, err)
        assert any(int(v) < T for v in svl)
        for b in range(B):
            assert np.all(got[b, int(svl[b]):] == 0.0) and np.all(rd[b, int(svl[b]):] == 0.0), b
            assert np.abs(got[b, :int(svl[b])]).max() > 0
        # the step's other outputs are what tn_gnmt_trainer_forward_backward leaves
        worst, worst_k = _captioner_grad_err(tr, rg)
        assert worst < 2e-3, (worst_k, worst)


# ---- 2. the whole step, open ReLUs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell,H", [("gru", 8), ("lstm", 8), ("gru", 128)])
def test_step_exact_with_open_relus(report, cell, H):
    """every backbone and captioner gradient with the BatchNorm shifts raised by +4 (no ReLU input near 0: float32 and float64 take
    the same branches)"""
    p, x, svl, tgt, tvl = _setup(cell, H, 4.0)
    tr = _trainer(p, H, cell)
    loss, logits = _run(tr, x, svl, tgt, tvl)
    rl, rlog, rg, _, _ = _oracle(cell, H, 4.0)
    el = float(np.abs(logits - rlog).max())
    report[f"gnmt_frames_{cell}_H{H}_open_relu_logits_maxabs_err"] = el
    assert el < 1e-3 * max(1.0, np.abs(rlog).max())
    assert len([k for k in rg if k.startswith("densenet0_")]) == 362 and len(rg) == 362 + len([k for k in p if k.startswith("gnmt_")])
    worst, worst_k, min_cos = _compare(tr, rg)
    report[f"gnmt_frames_{cell}_H{H}_open_relu_grad_rel_err_worst"] = float(worst)
    report[f"gnmt_frames_{cell}_H{H}_open_relu_grad_min_cosine"] = float(min_cos)
    assert worst < 2e-3 and min_cos > 0.999999, (worst_k, worst, min_cos)


# ---- 3. the whole step, stock weights ---------------------------------------------------------------------------------------------

def test_stock_step_matches_autograd(report):
    p, x, svl, tgt, tvl = _setup()
    tr = _trainer(p, 8)
    loss, logits = _run(tr, x, svl, tgt, tvl)
    rl, rlog, rg, rstats, _ = _oracle()
    el = float(np.abs(logits - rlog).max())
    report["gnmt_frames_stock_logits_maxabs_err"] = el
    report["gnmt_frames_stock_loss_abs_err"] = abs(loss - rl)
    assert el < 1e-4 and abs(loss - rl) < 1e-4, (el, loss, rl)
    for bn in STOCK_BNS:                                    # batch statistics over all 6 frames, the zero one included
        c = rstats[bn][0].shape[0]
        em = np.abs(tr.get(bn + "_batch_mean", shape=(c,)) - rstats[bn][0]).max() / max(1.0, np.abs(rstats[bn][0]).max())
        ev = np.abs(tr.get(bn + "_batch_var", shape=(c,)) - rstats[bn][1]).max() / max(1.0, np.abs(rstats[bn][1]).max())
        report[f"gnmt_frames_stock_{bn}_batch_stat_err"] = float(max(em, ev))
        assert em < 1e-4 and ev < 1e-4, (bn, em, ev)
    worst, worst_k = _captioner_grad_err(tr, rg)
    report["gnmt_frames_stock_captioner_grad_rel_err"] = worst
    assert worst < 2e-3, (worst_k, worst)
    _, _, min_cos = _compare(tr, {k: g for k, g in rg.items() if k.startswith("densenet0_")})
    report["gnmt_frames_stock_backbone_grad_min_cosine"] = float(min_cos)
    assert min_cos > 0.995, min_cos
    for bn in ("densenet0_stage2_batchnorm3", "densenet0_batchnorm4"):
        for i, s in enumerate(("_running_mean", "_running_var")):
            exp = 0.9 * p[bn + s].astype(np.float64) + 0.1 * rstats[bn][i]
            assert np.abs(tr.get(bn + s) - exp).max() < 1e-4 * max(1.0, np.abs(exp).max()), (bn, s)


# ---- 4. the padded slots --------------------------------------------------------------------------------------------------------

def test_padded_slots_do_not_depend_on_their_content():
    p, x, svl, tgt, tvl = _setup()
    tr = _trainer(p, 8)
    la, ga = _run(tr, x, svl, tgt, tvl)
    grads_a = [g.clone() for g in tr.grads]
    xn = x.copy()
    xn[1, 2] = np.nan
    lb, gb = _run(tr, xn, svl, tgt, tvl)
    assert np.isfinite(la) and la == lb and np.array_equal(ga, gb)
    for a, b in zip(grads_a, tr.grads):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    # the same through a caller's NHWC tensor, which the step must leave as it was
    xd = torch.from_numpy(xn).cuda().permute(0, 1, 3, 4, 2).contiguous()
    keep = xd.clone()
    lc = tr.forward_backward(xd, torch.from_numpy(svl).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(tvl).cuda())
    assert float(lc) == la and torch.equal(torch.nan_to_num(xd, nan=7.0), torch.nan_to_num(keep, nan=7.0))


# ---- 5. a handle larger than the step ---------------------------------------------------------------------------------------------

def test_larger_handle_is_bit_identical_and_runs_other_shapes(report):
    p, x, svl, tgt, tvl = _setup()
    a = _trainer(p, 8)
    la, ga = _run(a, x, svl, tgt, tvl)
    b = _trainer(p, 8, max_batch=4, max_src_len=3, max_frames=12)
    lb, gb = _run(b, x, svl, tgt, tvl)
    assert la == lb and np.array_equal(ga, gb)
    for u, v in zip(a.grads, b.grads):
        assert torch.equal(u, v)
    for bn in STOCK_BNS:
        c = p[bn + "_gamma"].shape[0]
        assert np.array_equal(a.get(bn + "_batch_var", shape=(c,)), b.get(bn + "_batch_var", shape=(c,)))
        assert np.array_equal(a.get(bn + "_running_var"), b.get(bn + "_running_var"))
    # batch 3 x steps 2 on the larger handle (fresh parameters: nothing was updated)
    p3, x3, svl3, tgt3, tvl3 = _setup(B=3, T=2, svl=(2, 2, 1), seed=6)
    c3 = _trainer(p3, 8, max_batch=4, max_src_len=3, max_frames=12)
    _run(c3, x, svl, tgt[:, :L], tvl)                       # first another shape, then this one
    l3, g3 = _run(c3, x3, svl3, tgt3, tvl3)
    r3 = _oracle(B=3, T=2, svl=(2, 2, 1), seed=6)
    report["gnmt_frames_3x2_loss_abs_err"] = abs(l3 - r3[0])
    assert abs(l3 - r3[0]) < 1e-4 and np.abs(g3 - r3[1]).max() < 1e-4


# ---- 6. frozen backbone -----------------------------------------------------------------------------------------------------------

def test_frozen_step(report):
    """--freeze_backbone: the captioner's gradients are the trainable step's (the oracle with detached features has the same graph
    above the features), the backbone bit-identical after step, its running statistics updated from the batch"""
    p, x, svl, tgt, tvl = _setup()
    tr = _trainer(p, 8, frozen=True)
    assert len(tr.grads) == 1
    loss, logits = _run(tr, x, svl, tgt, tvl)
    rl, rlog, rg, rstats, _ = _oracle()
    assert np.abs(logits - rlog).max() < 1e-4 and abs(loss - rl) < 1e-4
    worst, worst_k = _captioner_grad_err(tr, rg)
    report["gnmt_frames_frozen_captioner_grad_rel_err"] = worst
    assert worst < 2e-3, (worst_k, worst)
    before = {k: tr.get(k) for k in tr.names if k.startswith("densenet0_") and "running" not in k}
    cap_before = tr.get("gnmt_tgt_proj_bias")
    tr.step(1e-3)
    for k, v in before.items():
        assert np.array_equal(tr.get(k), v), k
    assert not np.array_equal(tr.get("gnmt_tgt_proj_bias"), cap_before)
    bn = "densenet0_stage2_batchnorm3"
    exp = 0.9 * p[bn + "_running_mean"].astype(np.float64) + 0.1 * rstats[bn][0]
    assert np.abs(tr.get(bn + "_running_mean") - exp).max() < 1e-4 * max(1.0, np.abs(exp).max())
    assert not np.array_equal(tr.get(bn + "_running_mean"), p[bn + "_running_mean"])


def test_frozen_oracle_has_the_trainable_captioner_gradients():
    """what test_frozen_step relies on, on the captioner alone: detaching the source does not change the parameters' gradients"""
    p, x, svl, tgt, tvl = _setup()
    rng = np.random.default_rng(1)
    q = {k: v for k, v in p.items() if k.startswith("gnmt_")}
    src = np.abs(rng.normal(0, 0.5, (2, 3, 1024)))
    _, _, ga, _ = ft.captioner_loss_and_grads(q, src, svl, tgt, tvl, 8)
    _, _, gb = gt.loss_and_grads(q, src, svl, tgt, tvl, 8)
    for k in ga:
        assert np.abs(ga[k] - gb[k]).max() < 1e-12, k


# ---- 7. Adam over both parts ------------------------------------------------------------------------------------------------------

def test_three_adam_steps_lower_the_loss_and_match_the_update(report):
    p, x, svl, tgt, tvl = _setup(seed=9)
    tr = _trainer(p, 8)
    names = ["densenet0_conv0_weight", "densenet0_stage3_conv7_weight", "densenet0_stage4_conv31_weight", "densenet0_batchnorm4_gamma",
             "gnmt_enc_rnn0_l_i2h_weight", "gnmt_tgt_proj_bias"]
    lr = 1e-3
    w = {k: tr.get(k).astype(np.float64) for k in names}
    m, v = {}, {}
    rm = tr.get("densenet0_batchnorm4_running_mean")
    losses = []
    for step in range(1, 4):
        loss, _ = _run(tr, x, svl, tgt, tvl)
        losses.append(loss)
        g = {k: tr.get(k, gradient=True).astype(np.float64) for k in names}
        rm_before = tr.get("densenet0_batchnorm4_running_mean")
        tr.step(lr)
        assert np.array_equal(tr.get("densenet0_batchnorm4_running_mean"), rm_before)       # no parameter: Adam leaves it alone
        w, m, v = gt.adam_step(w, g, m, v, step, lr)
        for k in names:
            err = float(np.abs(tr.get(k) - w[k]).max() / max(1.0, np.abs(w[k]).max()))
            report[f"gnmt_frames_adam_{k}_err"] = max(err, report.get(f"gnmt_frames_adam_{k}_err", 0.0))
            assert err < 2e-4, (step, k, err)
    assert not np.array_equal(tr.get("densenet0_batchnorm4_running_mean"), rm)
    loss, _ = _run(tr, x, svl, tgt, tvl)
    losses.append(loss)
    report["gnmt_frames_adam_losses"] = [float(l) for l in losses]
    assert losses[-1] < losses[0], losses


# ---- 8. input layouts -------------------------------------------------------------------------------------------------------------

def test_uint8_and_nhwc_frames_give_the_nchw_result():
    from tennis_amd import weights as W
    p, x, svl, tgt, tvl = _setup()
    u8 = W.synthetic_frames_u8(6, 224, 5)
    assert np.array_equal(W.normalize_to_nchw_f32(u8).reshape(x.shape), x)
    args = [torch.from_numpy(a).cuda() for a in (svl, tgt, tvl)]
    a = _trainer(p, 8)
    la, ga = _run(a, x, svl, tgt, tvl)
    b = _trainer(p, 8)
    lb, gb = b.forward_backward(torch.from_numpy(u8).cuda().reshape(2, 3, 224, 224, 3), *args, return_logits=True)
    assert np.abs(gb.cpu().numpy() - ga).max() < 1e-4
    c = _trainer(p, 8)
    xn = torch.from_numpy(x).cuda().permute(0, 1, 3, 4, 2).contiguous()
    lc, gc = c.forward_backward(xn, *args, return_logits=True)
    assert np.array_equal(gc.cpu().numpy(), ga) and float(lc) == la


# ---- 9. the driver --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [[], ["--freeze_backbone"]])
def test_train_and_evaluate_on_frames(tmp_path, capsys, extra):
    import re
    from tennis_amd import evaluate_gnmt as eg, train_gnmt as tg
    from tennis_amd import weights as W
    from tennis_amd.params_io import is_mxnet_params, load_mxnet_params
    from tools import tiny_dataset
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    tiny_dataset.write(root, np.random.default_rng(0), frames_per_point=5)          # every 2: clips of 3 frames
    args = ["--data_root", root, "--data_shape", "224", "--model_id", "0200", "--epochs", "1", "--batch_size", "2", "--num_hidden", "8",
            "--emb_size", "6", "--emb_file", "", "--every", "2", "--root", exp] + extra
    assert tg.main(args) == 0
    out = capsys.readouterr().out
    for name in ("valid", "test"):
        m = re.search(name + r" Loss=([0-9.naninf]+), .* bleu=([0-9.naninf]+)", out)
        assert m and np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(2))), out
    f0 = os.path.join(exp, "0200", "0000.params")
    saved = load_mxnet_params(f0)
    assert is_mxnet_params(f0) and "src_embed.model.0.weight" in saved and "src_embed.model.1.running_mean" in saved
    assert "encoder.rnn_cells.0.l_cell.i2h_weight" in saved and "tgt_proj.weight" in saved and any(k.startswith("decoder.") for k in saved)
    assert saved["encoder.rnn_cells.0.l_cell.i2h_weight"].shape == (3 * 8, 1024)
    start = W.make_densenet121_weights(0, "densenet0_", fp16_model=True)
    if extra:
        assert np.array_equal(saved["src_embed.model.0.weight"], start["densenet0_conv0_weight"])
        assert not np.array_equal(saved["src_embed.model.1.running_mean"], start["densenet0_batchnorm0_running_mean"])
    else:
        assert not np.array_equal(saved["src_embed.model.0.weight"], start["densenet0_conv0_weight"])
    out = eg.main(args)
    text = capsys.readouterr().out
    assert "0000.params" in text or "valid_best.params" in text
    assert all(np.isfinite(v[0]) and np.isfinite(v[1]) for v in out.values()) and set(out) == {"valid", "test"}
    if not extra:                                        # a second run resumes after the newest NNNN.params
        assert tg.main(args[:args.index("--epochs")] + ["--epochs", "2"] + args[args.index("--epochs") + 2:]) == 0
        text = capsys.readouterr().out
        assert "Loaded model params" in text and "0000.params" in text and os.path.exists(os.path.join(exp, "0200", "0001.params"))


# ---- 10. ABI refusals -------------------------------------------------------------------------------------------------------------

def test_abi_refusals():
    from tennis_amd import _lib as Lb
    from tennis_amd import weights as W
    ctx = Lb.default_context()
    lib = ctx.lib
    p, x, svl, tgt, tvl = _setup()
    arr, keep = Lb.make_params(p)
    h = C.c_void_p()

    def create(c=ctx.handle, params=arr, n=len(arr), bb=b"densenet0_", pre=b"gnmt_", side=224, max_batch=2, max_src_len=3, max_frames=6,
               out=C.byref(h)):
        return lib.tn_gnmt_frames_trainer_create(c, params, n, bb, pre, Lb.RNN_GRU, 8, E, V, 2, 1, 0, side, max_batch, max_src_len, L,
                                                 max_frames, 0, out)
    last = lambda: lib.tn_last_error().decode()                  # the whole message a refusal leaves, entry name included
    INV, CR, FB = ("invalid argument: " + s for s in ("", "tn_gnmt_frames_trainer_create: ", "tn_gnmt_frames_trainer_forward_backward: "))
    assert create(c=None) == -1                                  # TN_ERR_INVALID
    assert last() == CR + "null argument"
    for null in ("params", "bb", "pre", "out"):
        assert create(**{null: None}) != 0
        assert last() == CR + "null argument"
    for side in (100, 0):
        assert create(side=side) != 0
        assert "divisible by 32" in lib.tn_last_error().decode()
        assert last() == CR + "frames must be square with a side divisible by 32"
    for zero in ("max_batch", "max_src_len", "max_frames"):
        assert create(**{zero: 0}) != 0
        assert last() == CR + "bad max_batch / max_src_len / max_frames"
    assert create() == 0 and h.value
    xd = torch.from_numpy(x).cuda().permute(0, 1, 3, 4, 2).contiguous()
    sd, td, ld = (torch.from_numpy(a).cuda() for a in (svl, tgt, tvl))
    loss = torch.empty(1, device="cuda")

    def fb(t=h, frames=Lb.ptr(xd), s=Lb.ptr(sd), tg=Lb.ptr(td), tv=Lb.ptr(ld), batch=2, steps=3, lo=Lb.ptr(loss)):
        return lib.tn_gnmt_frames_trainer_forward_backward(t, frames, s, tg, L, tv, batch, steps, L, lo, None)
    try:
        for null in ("t", "frames", "s", "tg", "tv", "lo"):
            assert fb(**{null: None}) != 0
            assert last() == FB + "null argument"
        assert fb(batch=3, steps=2) != 0 and "max_batch" in lib.tn_last_error().decode()
        assert last() == FB + "batch exceeds max_batch"
        assert fb(batch=1, steps=4) != 0 and "max_src_len" in lib.tn_last_error().decode()
        assert last() == FB + "steps exceed max_src_len"
        assert fb(batch=0) != 0
        assert last() == FB + "batch exceeds max_batch"
        assert fb(steps=0) != 0
        assert last() == FB + "steps exceed max_src_len"
        assert lib.tn_gnmt_frames_trainer_buffers(None, None, None, None, None, None, None) != 0
        assert last() == INV + "tn_gnmt_frames_trainer_buffers: null handle"
        assert lib.tn_gnmt_frames_trainer_adam_step(None, 1e-3, 0.9, 0.999, 1e-8) != 0
        assert last() == INV + "tn_gnmt_frames_trainer_adam_step: null handle"
        # (what a part refuses, it refuses under its own name)
        assert lib.tn_gnmt_frames_trainer_set_dropout(None, 0.1, 0) != 0
        assert last() == INV + "tn_gnmt_frames_trainer_set_dropout: null handle"
        assert lib.tn_gnmt_frames_trainer_set_dropout(h, 1.0, 0) != 0
        assert last() == INV + "tn_gnmt_trainer_set_dropout: rate must be in [0, 1)"
        buf = (C.c_float * 4)()
        n = C.c_int64()
        assert lib.tn_gnmt_frames_trainer_read_param(h, b"densenet0_no_such", 0, buf, 4, C.byref(n)) != 0
        assert last() == INV + "tn_finetune_read_param: unknown parameter name"
        assert lib.tn_gnmt_frames_trainer_read_param(h, b"other_name", 0, buf, 4, C.byref(n)) != 0
        assert last() == INV + "tn_gnmt_frames_trainer_read_param: unknown parameter name"
        assert lib.tn_gnmt_frames_trainer_read_param(h, b"gnmt_tgt_proj_bias", 0, buf, 4, C.byref(n)) != 0     # buffer too small
        assert last() == INV + "tn_gnmt_trainer_read_param: host buffer too small"
        assert lib.tn_gnmt_frames_trainer_read_param(h, b"gnmt_tgt_proj_bias", 0, None, 4, C.byref(n)) != 0
        assert last() == INV + "tn_gnmt_frames_trainer_read_param: null argument"
        # a step after the refusals still runs
        assert fb() == 0 and bool(torch.isfinite(loss).all())
    finally:
        assert lib.tn_gnmt_frames_trainer_destroy(h) == 0
    assert lib.tn_gnmt_frames_trainer_destroy(None) == 0
    # batch * steps beyond max_frames on a handle whose other maxima would allow it
    h3 = C.c_void_p()
    assert create(max_batch=2, max_src_len=3, max_frames=4, out=C.byref(h3)) == 0
    try:
        assert lib.tn_gnmt_frames_trainer_forward_backward(h3, Lb.ptr(xd), Lb.ptr(sd), Lb.ptr(td), L, Lb.ptr(ld), 2, 3, L, Lb.ptr(loss),
                                                           None) != 0
        assert "max_frames" in lib.tn_last_error().decode()
        assert last() == FB + "batch * steps exceeds max_frames"
        assert lib.tn_gnmt_frames_trainer_forward_backward(h3, Lb.ptr(xd), Lb.ptr(sd), Lb.ptr(td), L, Lb.ptr(ld), 2, 2, L, Lb.ptr(loss),
                                                           None) == 0
    finally:
        assert lib.tn_gnmt_frames_trainer_destroy(h3) == 0
    # a first encoder layer that is not as wide as the backbone's features
    q = {k: v for k, v in p.items() if not k.startswith("gnmt_")}
    q.update(W.make_gnmt_weights(5, "gru", 512, 8, E, V))
    arr2, keep2 = Lb.make_params(q)
    h2 = C.c_void_p()
    assert create(params=arr2, n=len(arr2), out=C.byref(h2)) != 0
    assert "feature width" in lib.tn_last_error().decode()
    assert last() == "tn_gnmt_frames_trainer_create: gnmt_enc_rnn0_l_i2h_weight is not (gates * hidden, 1024), the backbone's feature width"
    # a missing parameter, of either part
    for gone in ("gnmt_dec_rnn1_h2h_bias", "densenet0_stage2_conv3_weight"):
        q = {k: v for k, v in p.items() if k != gone}
        arr3, keep3 = Lb.make_params(q)
        assert create(params=arr3, n=len(arr3), out=C.byref(h2)) != 0
        assert gone in lib.tn_last_error().decode()
        assert last() == "missing parameter: " + gone
    del keep, keep2, keep3
