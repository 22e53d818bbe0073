"""-m gpu: the temporal head trained from a device-resident feature table (``TemporalHeadTrainer.set_features`` /
``forward_backward_rows`` / ``predict_rows``; ``tn_head_*_rows``): the step whose windows are gathered inside the two kernels that
read the (B*T, F) window matrix against the same step on the materialised ``table[idx]`` - bit for bit, because the gathered forms
keep the k-loop and the MFMA order - and against the float64 oracle (oracle/train_np.py) at the bars tests/test_gpu_train.py
uses for that step; then ``train --dense_windows`` against the loader route.

No test hands an out-of-range index to the device: the kernels' clamp is read from the code, not provoked."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import train_np as tn

pytestmark = pytest.mark.gpu

CLASSES = 11
ROWS = 301            # rows of the feature table: a few hundred, no multiple of 64
LR, MOM, WD = 1e-2, 0.9, 1e-4
# (B, T, F, H): the skinny linear kernel with partial tiles in every dimension; F % 4 != 0: the scalar staging path; and per
# cell a shape with ceil(BT / 64) * ceil(2GH / 64) >= 512 tiles, where launch_linear_f32 picks linear_f32_kernel<2>
SHAPES = {"gru": [(3, 5, 24, 8), (6, 9, 30, 32), (92, 30, 64, 128)],
          "lstm": [(3, 5, 24, 8), (6, 9, 30, 32), (32, 64, 64, 128)]}
CASES = [(cell, *shape) for cell in ("gru", "lstm") for shape in SHAPES[cell]]


def _trainer(p, B, T, F, H, cell):
    from tennis_amd.engine import TemporalHeadTrainer
    return TemporalHeadTrainer(p, F, H, CLASSES, max_batch=B, max_steps=T, type=cell)


def _inputs(cell, B, T, F, H, seed=11):
    from tennis_amd import weights as W
    p = W.make_rnn_weights(seed, cell, F, H, f"cnnrnn0_{cell}0_")
    p.update(W.make_dense_weights(seed + 1, CLASSES, 2 * H, "cnnrnn0_dense0_"))
    rng = np.random.default_rng(seed)
    table = (np.abs(rng.normal(0, 1, (ROWS, F))) * 0.5).astype(np.float32)
    idx = rng.integers(0, ROWS, (B, T)).astype(np.int32)
    idx[0, 0], idx[0, 1], idx[-1, -1] = 0, ROWS - 1, ROWS - 1       # the table's first and last row
    idx[1] = idx[0]                                                 # a whole window twice
    idx[2, :3] = idx[2, 0]                                          # one row at neighbouring steps
    y = rng.integers(0, CLASSES, B).astype(np.int32)
    return p, table, idx, y


@functools.lru_cache(maxsize=None)
def _run(cell, B, T, F, H):
    """Both steps and the oracle, once per case: the materialised step, the gathered step (with predict_rows in front of it and
    behind it), one SGD update of each."""
    p, table, idx, y = _inputs(cell, B, T, F, H)
    td, yd = torch.from_numpy(table).cuda(), torch.from_numpy(y).cuda()
    idx_d = torch.from_numpy(idx).cuda()
    out = {"p": p, "x": table[idx], "y": y}
    mat = _trainer(p, B, T, F, H, cell)
    loss, logits = mat.forward_backward(td[idx_d.long()], yd)
    out["mat"] = (loss.cpu().numpy(), logits.cpu().numpy(), {k: mat.get(k, gradient=True) for k in mat.names})
    mat.step(B, LR, MOM, WD)
    out["mat_params"] = mat.state_dict()

    rows = _trainer(p, B, T, F, H, cell)
    rows.set_features(td)
    out["predict_before"] = rows.predict_rows(idx_d).cpu().numpy()
    loss, logits = rows.forward_backward_rows(idx_d, yd)
    out["rows"] = (loss.cpu().numpy(), logits.cpu().numpy(), {k: rows.get(k, gradient=True) for k in rows.names})
    g0, w0 = rows.grads.clone(), rows.params.clone()
    out["predict_after"] = rows.predict_rows(idx_d).cpu().numpy()
    out["predict_host_idx"] = rows.predict_rows(idx).cpu().numpy()       # a numpy idx: range-checked, then the same call
    out["predict_left_alone"] = bool(torch.equal(g0, rows.grads)) and bool(torch.equal(w0, rows.params))
    rows.step(B, LR, MOM, WD)
    out["rows_params"] = rows.state_dict()
    out["predict_left_momentum_alone"] = all(np.array_equal(out["rows_params"][k], out["mat_params"][k]) for k in mat.names)
    return out


@pytest.mark.parametrize("cell,B,T,F,H", CASES)
def test_gathered_step_equals_the_materialised_step_bit_for_bit(cell, B, T, F, H):
    r = _run(cell, B, T, F, H)
    (l0, lg0, g0), (l1, lg1, g1) = r["mat"], r["rows"]
    assert np.array_equal(l0, l1) and np.array_equal(lg0, lg1)
    assert set(g0) == set(g1) == set(r["p"])
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
        assert np.abs(g0[k]).max() > 0, k
    for k in r["p"]:
        assert np.array_equal(r["mat_params"][k], r["rows_params"][k]), k
        assert not np.array_equal(r["rows_params"][k], r["p"][k]), k


@pytest.mark.parametrize("cell,B,T,F,H", CASES)
def test_gathered_step_against_the_float64_oracle(report, cell, B, T, F, H):
    r = _run(cell, B, T, F, H)
    loss, logits, grads = r["rows"]
    rl, rlg, rg = tn.forward_backward(r["x"], r["y"], r["p"], cell=cell)
    e_loss, e_logits = float(np.abs(loss - rl).max()), float(np.abs(logits - rlg).max())
    print(f"{cell} B{B} T{T} F{F} H{H}: loss err {e_loss:.2e} logits err {e_logits:.2e}")
    worst = 0.0
    errs = {}
    for k, g in rg.items():
        errs[k] = float(np.abs(grads[k].reshape(g.shape) - g).max() / max(1e-6, np.abs(g).max()))
        worst = max(worst, errs[k])
    print(f"  worst gradient error relative to the tensor's maximum: {worst:.2e}")
    p1, _ = tn.sgd_momentum({k: v.astype(np.float64) for k, v in r["p"].items()}, rg, {}, LR, MOM, WD, 1.0 / B)
    perr = {k: float(np.abs(r["rows_params"][k] - p1[k]).max() / np.abs(p1[k]).max()) for k in p1}
    print(f"  worst parameter error after a step relative to the parameter's maximum: {max(perr.values()):.2e}")
    report[f"head_rows_{cell}_grad_rel_err_B{B}_T{T}_F{F}"] = worst
    assert e_loss < 1e-4 and e_logits < 1e-4
    for k, e in errs.items():
        assert e < 2e-4, (k, e)
    for k, e in perr.items():
        assert e < 1e-5, (k, e)


@pytest.mark.parametrize("cell,B,T,F,H", CASES)
def test_predict_rows_is_the_forward_half(cell, B, T, F, H):
    r = _run(cell, B, T, F, H)
    assert np.array_equal(r["predict_before"], r["rows"][1])     # same handle, same parameters: the step's own logits
    assert np.array_equal(r["predict_after"], r["rows"][1])
    assert r["predict_left_alone"], "predict_rows changed the gradients or the parameters"
    assert r["predict_left_momentum_alone"], "the update after predict_rows differs from the one without it"
    assert np.array_equal(r["predict_host_idx"], r["rows"][1])


def test_rows_calls_contract():
    from tennis_amd import _lib
    cell, B, T, F, H = "gru", 3, 5, 24, 8
    p, table, idx, y = _inputs(cell, B, T, F, H)
    tr = _trainer(p, B, T, F, H, cell)
    td, yd, idx_d = torch.from_numpy(table).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(idx).cuda()
    loss, logits = torch.empty(B, device="cuda"), torch.empty((B, CLASSES), device="cuda")
    lib, ptr, null = tr.lib, _lib.ptr, C.c_void_p(None)
    # before set_features: the Python layer raises, and so does the C ABI underneath it
    with pytest.raises(RuntimeError, match="set_features"):
        tr.forward_backward_rows(idx_d, yd)
    with pytest.raises(RuntimeError, match="set_features"):
        tr.predict_rows(idx_d)
    assert lib.tn_head_forward_backward_rows(tr.handle, ptr(idx_d), ptr(yd), B, T, ptr(loss), ptr(logits)) == -1
    assert b"tn_head_set_features" in lib.tn_last_error()
    assert lib.tn_head_forward_rows(tr.handle, ptr(idx_d), B, T, ptr(logits)) == -1
    assert lib.tn_head_set_features(tr.handle, null, ROWS, F) == -1
    assert lib.tn_head_set_features(tr.handle, ptr(td), 0, F) == -1
    assert lib.tn_head_set_features(tr.handle, ptr(td), ROWS, F - 1) == -1
    with pytest.raises(ValueError):
        tr.set_features(td[:, :F - 1])
    with pytest.raises(ValueError):
        tr.set_features(torch.from_numpy(table))            # a host tensor: the table is uploaded by the caller, once
    tr.set_features(td)
    # nulls, and batch / steps over the handle's maxima
    assert lib.tn_head_forward_backward_rows(tr.handle, null, ptr(yd), B, T, ptr(loss), ptr(logits)) == -1
    assert lib.tn_head_forward_backward_rows(tr.handle, ptr(idx_d), null, B, T, ptr(loss), ptr(logits)) == -1
    assert lib.tn_head_forward_rows(tr.handle, null, B, T, ptr(logits)) == -1
    assert lib.tn_head_forward_rows(tr.handle, ptr(idx_d), B, T, null) == -1
    for b, t in ((B + 1, T), (B, T + 1), (0, T), (B, 0)):
        assert lib.tn_head_forward_backward_rows(tr.handle, ptr(idx_d), ptr(yd), b, t, ptr(loss), ptr(logits)) == -1
        assert lib.tn_head_forward_rows(tr.handle, ptr(idx_d), b, t, ptr(logits)) == -1
    # a host idx out of range raises before any launch: the gradient buffer is still the zeros of a fresh handle
    for bad in (-1, ROWS):
        wrong = idx.copy()
        wrong[1, 2] = bad
        for host in (wrong, torch.from_numpy(wrong), wrong.astype(np.int64)):
            with pytest.raises(ValueError, match="idx must lie in"):
                tr.forward_backward_rows(host, yd)
            with pytest.raises(ValueError, match="idx must lie in"):
                tr.predict_rows(host)
    with pytest.raises(ValueError):
        tr.predict_rows(idx.astype(np.float32))
    assert float(tr.grads.abs().max()) == 0.0
    # a smaller batch and fewer steps than the maxima are fine, from a host idx too
    _, lg = tr.forward_backward_rows(idx[:2, :3], yd[:2])
    assert lg.shape == (2, CLASSES) and torch.isfinite(lg).all() and float(tr.grads.abs().max()) > 0


def test_train_dense_windows_equals_the_loader_route(tmp_path, capsys):
    """evaluate --save_feats, then train --feats_model --window 4 --temp_pool gru --epochs 2 with and without --dense_windows: the
    same parameters bit for bit, the same scores.txt."""
    from tennis_amd import evaluate as ev, train as tr
    from tennis_amd.params_io import load_mxnet_params
    root = str(tmp_path / "data")
    common = ["--root", root, "--frames_per_video", "12", "--data_shape", "224", "--model_id", "0001"]
    for split in ("train", "val"):
        assert ev.main(common + ["--split", split, "--save_feats", "--batch_size", "8"]) == 0
    finals, scores = [], []
    for model_id, extra in (("0002", []), ("0003", ["--dense_windows"])):
        exp = str(tmp_path / "exp")
        args = ["--root", root, "--frames_per_video", "12", "--data_shape", "224", "--model_id", model_id, "--feats_model", "0001",
                "--window", "4", "--temp_pool", "gru", "--epochs", "2", "--batch_size", "8", "--lr", "0.01", "--lr_steps", "1, 2",
                "--exp_root", exp] + extra
        assert tr.main(args) == 0
        finals.append(load_mxnet_params(str(tmp_path / "exp" / model_id / "0001.params")))
        scores.append((tmp_path / "exp" / model_id / "scores.txt").read_text().splitlines())
    out = capsys.readouterr().out
    assert out.count("[dense_windows] train split") == 1 and out.count("[dense_windows] val split") == 1
    assert set(finals[0]) == set(finals[1]) and len(finals[0]) >= 10
    for k in finals[0]:
        assert np.array_equal(np.asarray(finals[0][k]), np.asarray(finals[1][k])), k
    assert len(scores[0]) == 2 and scores[0] == scores[1]
