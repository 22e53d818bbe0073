"""-m gpu: the table form of the windowed kernels (csrc/rnn_window.hip: rows named by an index table instead of (centre, lo, hi);
engine.WindowHead.forward_rows, engine.temporal_pool_rows, tn_window_head_forward_rows, tn_temporal_pool_rows) and the feature-mode
fallback of evaluate --dense_windows (evaluate.evaluate_table).

Two references.  (1) The arithmetic form of the same kernels, whose bits tests/test_gpu_window_head.py pins: a table that spells out
a (centre, lo, hi, stride) window must give those bits.  (2) The float64 head of that file on host-gathered windows, for tables no
(centre, lo, hi) can express; bar 1e-4, that file's figure for this kernel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_gpu_window_head import (BAR, CLASSES, STRIDES, WINDOWS, _features, _index_arrays, _model, host_rows, oracle_f64)

pytestmark = pytest.mark.gpu

CELLS = [(m, h) for m in ("gru", "lstm") for h in (128, 32, 8)]      # the three routes: column in registers, DPP, plain
FEAT = 64


def _head(mode, hidden, tag, feats):
    from tennis_amd.engine import WindowHead
    _, p, rp, dp = _model(mode, FEAT, hidden, f"rows_{tag}_{mode}{hidden}")
    rows = feats.shape[0]
    head = WindowHead(mode, FEAT, hidden, CLASSES, p, rp, dp, max_rows=rows, max_samples=max(rows, 64))
    return head.project(torch.from_numpy(feats).cuda()), p, rp, dp


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("mode,hidden", CELLS)
def test_table_of_a_window_gives_the_arithmetic_forms_bits(mode, hidden):
    centre, lo, hi, rows = _index_arrays()
    head, *_ = _head(mode, hidden, "bits", _features(rows, FEAT))
    for window in WINDOWS:
        for stride in STRIDES:
            idx = host_rows(centre, lo, hi, window, stride, rows)
            want_l, want_p = _np(*head.forward(centre, lo, hi, window, stride, return_pooled=True))
            got_l, got_p = _np(*head.forward_rows(idx, return_pooled=True))
            assert got_l.shape == (rows, CLASSES) and got_p.shape == (rows, 2 * hidden)
            assert np.array_equal(got_p, want_p), (window, stride)
            assert np.array_equal(got_l, want_l), (window, stride)
    # a table that is already on the device, in another integer type
    dev = torch.from_numpy(idx).cuda()
    assert np.array_equal(head.forward_rows(dev).cpu().numpy(), want_l)


@pytest.mark.parametrize("mode,hidden", CELLS)
def test_sample_counts_around_both_rows_per_workgroup(mode, hidden):
    centre, lo, hi, rows = _index_arrays()
    head, *_ = _head(mode, hidden, "nb", _features(rows, FEAT))
    window, stride = 7, 1
    idx = host_rows(centre, lo, hi, window, stride, rows)
    for nb in (4, 6 if mode == "gru" else 8):
        head._set_rows_per_group(nb)
        for n in (nb - 1, nb, nb + 1, 2 * nb + 1):
            want_l, want_p = _np(*head.forward(centre[:n], lo[:n], hi[:n], window, stride, return_pooled=True))
            got_l, got_p = _np(*head.forward_rows(idx[:n], return_pooled=True))
            assert got_l.shape == (n, CLASSES)
            assert np.array_equal(got_p, want_p) and np.array_equal(got_l, want_l), (nb, n)


def _free_table(rng, samples, window, rows):
    """rows no (centre, lo, hi) can name: random with repeats, a descending run, a constant row, rows of every video mixed"""
    idx = rng.integers(0, rows, (samples, window))
    idx[1] = np.arange(rows - 1, rows - 1 - window, -1) % rows
    idx[2] = 5
    idx[3, ::2] = idx[3, 0]
    return idx.astype(np.int64)


@pytest.mark.parametrize("mode,hidden", CELLS)
def test_free_tables_against_float64(mode, hidden, report):
    _, _, _, rows = _index_arrays()
    feats = _features(rows, FEAT, seed=2)
    head, p, rp, dp = _head(mode, hidden, "f64", feats)
    rng = np.random.default_rng(11)
    worst = 0.0
    for window in (2, 7, 30):
        idx = _free_table(rng, 37, window, rows)
        ref_p, ref_l = oracle_f64(feats[idx], p, mode, rp, dp)
        got_l, got_p = _np(*head.forward_rows(idx, return_pooled=True))
        e_l, e_p = float(np.abs(got_l - ref_l).max()), float(np.abs(got_p - ref_p).max())
        print(f"{mode} H={hidden} window={window}: logits {e_l:.3e} pooled {e_p:.3e}")
        worst = max(worst, e_l, e_p)
        assert e_l < BAR and e_p < BAR, (window, e_l, e_p)
    report[f"window_rows_{mode}_H{hidden}_free_table_maxabs"] = worst


def test_entries_outside_the_matrix_are_clamped():
    from tennis_amd.engine import temporal_pool_rows
    _, _, _, rows = _index_arrays()
    feats = _features(rows, FEAT, seed=3)
    x = torch.from_numpy(feats).cuda()
    rng = np.random.default_rng(12)
    for window in (7, 30):
        idx = _free_table(rng, 29, window, rows)
        idx[0, :3] = (-1, -2_000_000_000, -7)                 # negative: row 0 (not a zero row)
        idx[4, -3:] = (rows, rows + 5, 2_000_000_000)          # past the end: the last row
        idx[6] = -1
        idx[7] = rows
        clamped = np.clip(idx, 0, rows - 1)
        assert not np.array_equal(idx, clamped)
        for mode, hidden in CELLS:
            head, *_ = _head(mode, hidden, "clamp", feats)
            a = _np(*head.forward_rows(idx, return_pooled=True))
            b = _np(*head.forward_rows(clamped, return_pooled=True))
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (mode, hidden, window)
        for kind in ("max", "mean"):
            assert np.array_equal(temporal_pool_rows(x, idx, kind).cpu().numpy(), temporal_pool_rows(x, clamped, kind).cpu().numpy())
        assert np.array_equal(temporal_pool_rows(x, idx, "max").cpu().numpy()[6], feats[0])      # all -1: row 0 itself


@pytest.mark.parametrize("feat", [64, 1000])
def test_temporal_pool_rows(feat, report):
    from tennis_amd.engine import temporal_pool_rows, temporal_pool_windows
    centre, lo, hi, rows = _index_arrays()
    feats = np.random.default_rng(5).normal(0, 1, (rows, feat)).astype(np.float32)
    x = torch.from_numpy(feats).cuda()
    scale = float(np.abs(feats).max())
    worst = 0.0
    for window in WINDOWS:
        for stride in STRIDES:
            idx = host_rows(centre, lo, hi, window, stride, rows)
            for kind in ("max", "mean"):                                   # the arithmetic form's bits
                assert np.array_equal(temporal_pool_rows(x, idx, kind).cpu().numpy(),
                                      temporal_pool_windows(x, centre, lo, hi, window, stride, kind).cpu().numpy()), (window, stride, kind)
    rng = np.random.default_rng(13)
    for window in (2, 7, 30):
        idx = _free_table(rng, 37, window, rows)
        win = feats[idx]
        assert np.array_equal(temporal_pool_rows(x, idx, "max").cpu().numpy(), win.max(1))
        e = float(np.abs(temporal_pool_rows(x, idx, "mean").cpu().numpy() - win.astype(np.float64).mean(1)).max()) / scale
        print(f"mean F={feat} window={window}: {e:.3e} of max|x|")
        worst = max(worst, e)
        assert e < 1e-6, (window, e)
    report[f"temporal_pool_rows_mean_F{feat}_rel_maxabs"] = worst


def test_table_form_abi_errors():
    from tennis_amd import _lib
    from tennis_amd import weights as W
    from tennis_amd.engine import WindowHead, temporal_pool_rows
    p = W.make_rnn_weights(1, "gru", 32, 16, "w_gru0_")
    p.update(W.make_dense_weights(2, CLASSES, 32, "w_dense0_"))
    head = WindowHead("gru", 32, 16, CLASSES, p, "w_gru0_", "w_dense0_", max_rows=8, max_samples=4)
    lib = _lib.load()
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, device="cuda")
    ok = np.zeros((3, 7), np.int32)

    def refused(rc, text):
        return rc == -1 and text in lib.tn_last_error()
    assert refused(lib.tn_window_head_forward_rows(head.handle, _lib.ptr(d), 3, 7, None, _lib.ptr(out)), b"project")      # no projection yet
    with pytest.raises(RuntimeError, match="project"):
        head.forward_rows(ok)
    head.project(torch.zeros((8, 32), device="cuda"))
    assert refused(lib.tn_window_head_forward_rows(None, _lib.ptr(d), 3, 7, None, _lib.ptr(out)), b"null")
    assert refused(lib.tn_window_head_forward_rows(head.handle, None, 3, 7, None, _lib.ptr(out)), b"null")
    assert refused(lib.tn_window_head_forward_rows(head.handle, _lib.ptr(d), 3, 7, None, None), b"null")
    assert refused(lib.tn_window_head_forward_rows(head.handle, _lib.ptr(d), 5, 7, None, _lib.ptr(out)), b"max_samples")
    assert refused(lib.tn_window_head_forward_rows(head.handle, _lib.ptr(d), 0, 7, None, _lib.ptr(out)), b"max_samples")
    assert refused(lib.tn_window_head_forward_rows(head.handle, _lib.ptr(d), 3, 0, None, _lib.ptr(out)), b"window")
    with pytest.raises(RuntimeError, match="max_samples"):
        head.forward_rows(np.zeros((5, 7), np.int32))
    with pytest.raises(ValueError):
        head.forward_rows(np.zeros(7, np.int32))                                  # not a (samples, window) table
    with pytest.raises(ValueError):
        head.forward_rows(np.zeros((3, 0), np.int32))
    with pytest.raises(RuntimeError, match="max_rows"):
        head.project(torch.zeros((9, 32), device="cuda"))
    head.project(torch.zeros((8, 32), device="cuda"))
    assert head.forward_rows(ok).shape == (3, CLASSES)                           # the handle still works
    assert head.forward(np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32), 7).shape == (3, CLASSES)
    ctx = _lib.default_context()
    x = torch.zeros((8, 32), device="cuda")
    args = lambda **k: [k.get("ctx", ctx.handle), k.get("x", _lib.ptr(x)), k.get("rows", 8), 32, k.get("idx", _lib.ptr(d)), k.get("n", 3),
                        k.get("w", 7), k.get("kind", 0), k.get("y", _lib.ptr(out))]
    for bad in (dict(ctx=None), dict(x=None), dict(idx=None), dict(y=None)):
        assert refused(lib.tn_temporal_pool_rows(*args(**bad)), b"null")
    assert refused(lib.tn_temporal_pool_rows(*args(w=0)), b"window")
    assert refused(lib.tn_temporal_pool_rows(*args(n=0)), b"shape") and refused(lib.tn_temporal_pool_rows(*args(rows=0)), b"shape")
    assert refused(lib.tn_temporal_pool_rows(*args(kind=5)), b"kind")
    assert lib.tn_temporal_pool_rows(*args()) == 0
    assert temporal_pool_rows(x, ok, "mean").shape == (3, 32)
    with pytest.raises(ValueError):
        temporal_pool_rows(x, np.zeros(7, np.int32), "max")


# ---- the feature-mode fallback of evaluate --dense_windows: a split without a (centre, lo, hi) form -------------------------------

EVAL_SEED = 1


def test_evaluate_table_where_window_rows_raises(tmp_path, report):
    from tennis_amd.dataset import DataLoader, TennisSet
    from tennis_amd.evaluate import evaluate_model, evaluate_table, evaluate_windows
    from tennis_amd.metrics.vision import PRF1
    ds = TennisSet(root=str(tmp_path), videos=("V1", "V2", "V3"), frames_per_video=13, window=7, every=2, stride=3, split_first=4,
                   feats_model="0006", balance=False, synthetic=True)
    with pytest.raises(ValueError):
        ds.window_rows()
    with pytest.raises(ValueError):
        evaluate_windows(None, ds, [])
    frames, idx = ds.window_table()
    assert set(frames) - {(s[0], s[1]) for s in ds._samples}                     # the windows reach frames that are no sample
    table = (np.abs(np.random.default_rng(EVAL_SEED).normal(0, 1, (len(frames), FEAT))) * 0.5).astype(np.float32)
    for (v, f), row in zip(frames, table):
        path = ds.get_feature_path(ds.feat_dir, v, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, row)
    m, p, rp, dp = _model("gru", FEAT, 128, "tabeval")
    ref = oracle_f64(table[idx], p, "gru", rp, dp)[1]
    m_loader, m_dense = [PRF1(label_names=ds.classes)], [PRF1(label_names=ds.classes)]
    res_a, gt_a = evaluate_model(m, DataLoader(ds, batch_size=16), ds, m_loader)
    res_b, gt_b = evaluate_table(m, ds, m_dense)
    assert list(res_a) == list(res_b) and gt_a == gt_b
    keys = [ds.get_image_path(ds._frames_dir, s[0], s[1]) for s in ds._samples]
    assert list(res_b) == keys and [gt_b[k] for k in keys] == [ds.classes.index(s[2]) for s in ds._samples]
    a, b = np.stack([res_a[k] for k in keys]), np.stack([res_b[k] for k in keys])
    e_a, e_b = float(np.abs(a - ref).max()), float(np.abs(b - ref).max())
    report["evaluate_table_logits_maxabs"], report["evaluate_model_table_split_logits_maxabs"] = e_b, e_a
    report["evaluate_table_vs_model_maxabs"] = float(np.abs(a - b).max())
    assert e_a < BAR and e_b < BAR, (e_a, e_b)
    assert m_dense[0].mat.sum() == len(ds)
    # the table handed over instead of the files; a table cut at the video boundaries (same bits per sample's pooled vector)
    res_c, _ = evaluate_table(m, ds, [PRF1(label_names=ds.classes)], features=table, frames_idx=(frames, idx))
    assert all(np.array_equal(res_b[k], res_c[k]) for k in keys)
    per_video = len(frames) // 3
    cut = m.forward_table(table, idx, max_rows=per_video, row_videos=[v for v, _ in frames]).cpu().numpy()
    assert float(np.abs(cut - ref).max()) < BAR
    with pytest.raises(ValueError, match="does not fit"):
        m.forward_table(table, idx, max_rows=per_video - 1, row_videos=[v for v, _ in frames])
    with pytest.raises(ValueError, match="row_videos"):
        m.forward_table(table, idx, max_rows=per_video)
