"""-m gpu: dense windowed evaluation of the temporal heads (csrc/rnn_window.hip, engine.WindowHead, CNNRNN / TemporalPooling
.forward_windows, evaluate.evaluate_windows).

Oracle: a float64 evaluation of the equations of oracle/rnn_np.py (GRU gates [r, z, n], LSTM gates [i, f, g, o]) on windows
materialised on the host with numpy, max over the steps, Dense.  Bar: logits and pooled within 1e-4 of it, the figure
tests/test_gpu_models.py::test_cnnrnn_feature_mode asserts for this model.  The measured worst cases go to the parity report."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 1e-4
VIDEOS = (5, 40, 17, 1)            # rows per "video": 5 is shorter than every window but 2; a one-row video has lo == hi
WINDOWS, STRIDES = (2, 7, 8, 30), (1, 3)
CLASSES = 11


def _index_arrays():
    centre, lo, hi, a = [], [], [], 0
    for n in VIDEOS:
        centre += list(range(a, a + n)); lo += [a] * n; hi += [a + n - 1] * n
        a += n
    return np.asarray(centre, np.int64), np.asarray(lo, np.int64), np.asarray(hi, np.int64), a


def host_rows(centre, lo, hi, window, stride, rows):
    """(samples, window) rows of the matrix: clamp(centre + (t - window // 2) * stride, lo, hi), then to [0, rows - 1]"""
    t = np.arange(window, dtype=np.int64)
    r = np.asarray(centre, np.int64)[:, None] + (t - window // 2)[None, :] * stride
    r = np.minimum(np.maximum(r, np.asarray(lo, np.int64)[:, None]), np.asarray(hi, np.int64)[:, None])
    return np.clip(r, 0, rows - 1)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def oracle_f64(x, p, mode, rnn_prefix, dense_prefix):
    """x (S, T, F) -> (pooled (S, 2H), logits (S, classes)), float64 throughout"""
    x = x.astype(np.float64)
    halves = []
    for d, rev in (("l0_", False), ("r0_", True)):
        wi, wh = p[rnn_prefix + d + "i2h_weight"].astype(np.float64), p[rnn_prefix + d + "h2h_weight"].astype(np.float64)
        bi, bh = p[rnn_prefix + d + "i2h_bias"].astype(np.float64), p[rnn_prefix + d + "h2h_bias"].astype(np.float64)
        hid = wh.shape[1]
        h = np.zeros((x.shape[0], hid))
        c = np.zeros_like(h)
        best = None
        for t in (range(x.shape[1] - 1, -1, -1) if rev else range(x.shape[1])):
            gi, gh = x[:, t] @ wi.T + bi, h @ wh.T + bh
            if mode == "gru":
                r = _sig(gi[:, :hid] + gh[:, :hid])
                z = _sig(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])
                n = np.tanh(gi[:, 2 * hid:] + r * gh[:, 2 * hid:])
                h = (1 - z) * n + z * h
            else:
                g = gi + gh
                c = _sig(g[:, hid:2 * hid]) * c + _sig(g[:, :hid]) * np.tanh(g[:, 2 * hid:3 * hid])
                h = _sig(g[:, 3 * hid:]) * np.tanh(c)
            best = h if best is None else np.maximum(best, h)
        halves.append(best)
    pooled = np.concatenate(halves, 1)
    return pooled, pooled @ p[dense_prefix + "weight"].astype(np.float64).T + p[dense_prefix + "bias"].astype(np.float64)


def _model(mode, feat, hidden, tag):
    from tennis_amd import weights as W
    from tennis_amd.models.vision.definitions import CNNRNN
    pre = f"winhead_{tag}_"
    m = CNNRNN(None, num_classes=CLASSES, type=mode, hidden_size=hidden, prefix=pre)
    m.initialize()
    p = W.make_rnn_weights(3, mode, feat, hidden, f"{pre}{mode}0_")
    p.update(W.make_dense_weights(4, CLASSES, 2 * hidden, f"{pre}dense0_"))
    m.set_params(p)
    return m, p, f"{pre}{mode}0_", f"{pre}dense0_"


def _features(rows, feat, seed=0):
    return (np.abs(np.random.default_rng(seed).normal(0, 1, (rows, feat))) * 0.5).astype(np.float32)


# H = 128 is the register-resident DPP form, H = 32 the streamed DPP form, H = 8 the plain form of the kernel
@pytest.mark.parametrize("mode,hidden,feat", [(m, h, f) for m in ("gru", "lstm") for h in (128, 8) for f in (64, 1024)]
                         + [("gru", 32, 64), ("lstm", 32, 64)])
def test_window_head_against_float64(mode, hidden, feat, report):
    from tennis_amd.engine import WindowHead
    centre, lo, hi, rows = _index_arrays()
    feats = _features(rows, feat)
    m, p, rp, dp = _model(mode, feat, hidden, f"{mode}{hidden}_{feat}")
    head = WindowHead(mode, feat, hidden, CLASSES, p, rp, dp, max_rows=rows, max_samples=rows)
    head.project(torch.from_numpy(feats).cuda())            # ONE projection serves every window / stride below
    worst = dict(logits=0.0, pooled=0.0, product=0.0, dense_vs_product=0.0)
    for window in WINDOWS:
        for stride in STRIDES:
            idx = host_rows(centre, lo, hi, window, stride, rows)
            ref_pooled, ref_logits = oracle_f64(feats[idx], p, mode, rp, dp)
            logits, pooled = head.forward(centre, lo, hi, window, stride, return_pooled=True)
            logits, pooled = logits.cpu().numpy(), pooled.cpu().numpy()
            via_model = m.forward_windows(feats, centre, lo, hi, window, stride).cpu().numpy()
            product = m(feats[idx]).cpu().numpy()           # the sample-by-sample path on the materialised windows
            e_l, e_p = float(np.abs(logits - ref_logits).max()), float(np.abs(pooled - ref_pooled).max())
            e_prod = float(np.abs(product - ref_logits).max())
            worst["logits"], worst["pooled"] = max(worst["logits"], e_l), max(worst["pooled"], e_p)
            worst["product"] = max(worst["product"], e_prod)
            worst["dense_vs_product"] = max(worst["dense_vs_product"], float(np.abs(logits - product).max()))
            print(f"{mode} H={hidden} F={feat} window={window} stride={stride}: logits {e_l:.3e} pooled {e_p:.3e} product {e_prod:.3e}")
            assert logits.shape == (rows, CLASSES) and pooled.shape == (rows, 2 * hidden)
            assert e_l < BAR and e_p < BAR, (window, stride, e_l, e_p)
            assert e_prod < BAR, (window, stride, e_prod)
            assert np.array_equal(via_model, logits)        # CNNRNN.forward_windows is this handle's arithmetic
    dev = [torch.from_numpy(a.astype(np.int32)).cuda() for a in (centre, lo, hi)]      # index arrays already on the device
    assert np.array_equal(m.forward_windows(torch.from_numpy(feats).cuda(), *dev, window, stride).cpu().numpy(), via_model)
    # a row budget below the matrix: cut at the video boundaries, the same bits per sample's pooled vector, logits within the bar
    cut = m.forward_windows(feats, centre, lo, hi, window, stride, max_rows=45).cpu().numpy()
    assert float(np.abs(cut - ref_logits).max()) < BAR
    with pytest.raises(ValueError, match="does not fit"):
        m.forward_windows(feats, centre, lo, hi, window, stride, max_rows=39)
    for k, v in worst.items():
        report[f"window_head_{mode}_H{hidden}_F{feat}_{k}_maxabs"] = v      # dense_vs_product: recorded, not asserted


@pytest.mark.parametrize("mode", ["gru", "lstm"])
def test_sample_counts_around_the_rows_per_workgroup(mode, report):
    """one below, at and above a multiple of every rows-per-workgroup the kernel has (4, 6 GRU, 8 LSTM): a sample's result
    does not depend on how many samples the call carries"""
    from tennis_amd.engine import WindowHead
    centre, lo, hi, rows = _index_arrays()
    feat, hidden, window, stride = 64, 128, 7, 1
    feats = _features(rows, feat)
    _, p, rp, dp = _model(mode, feat, hidden, f"nb_{mode}")
    idx = host_rows(centre, lo, hi, window, stride, rows)
    ref_pooled, ref_logits = oracle_f64(feats[idx], p, mode, rp, dp)
    head = WindowHead(mode, feat, hidden, CLASSES, p, rp, dp, max_rows=rows, max_samples=rows).project(torch.from_numpy(feats).cuda())
    full = head.forward(centre, lo, hi, window, stride, return_pooled=True)[1].cpu().numpy()
    worst = 0.0
    for nb in (0, 4, 6 if mode == "gru" else 8):
        head._set_rows_per_group(nb)
        for n in sorted({k * g + d for g in (4, 6, 8) for k in (1, 5) for d in (-1, 0, 1)}):
            logits, pooled = head.forward(centre[:n], lo[:n], hi[:n], window, stride, return_pooled=True)
            logits, pooled = logits.cpu().numpy(), pooled.cpu().numpy()
            assert logits.shape == (n, CLASSES)
            e = max(float(np.abs(logits - ref_logits[:n]).max()), float(np.abs(pooled - ref_pooled[:n]).max()))
            worst = max(worst, e)
            assert e < BAR, (nb, n, e)
            assert np.array_equal(pooled, full[:n]), (nb, n)
    report[f"window_head_{mode}_sample_counts_maxabs"] = worst


def test_project_once_forward_twice_equals_fresh_handles():
    from tennis_amd.engine import WindowHead
    centre, lo, hi, rows = _index_arrays()
    feat, hidden = 64, 128
    feats = torch.from_numpy(_features(rows, feat)).cuda()
    _, p, rp, dp = _model("gru", feat, hidden, "reuse")
    mk = lambda: WindowHead("gru", feat, hidden, CLASSES, p, rp, dp, max_rows=rows, max_samples=rows).project(feats)
    head = mk()
    a = head.forward(centre, lo, hi, 7, 1).cpu().numpy()
    b = head.forward(centre, lo, hi, 30, 3).cpu().numpy()
    assert np.array_equal(a, mk().forward(centre, lo, hi, 7, 1).cpu().numpy())
    assert np.array_equal(b, mk().forward(centre, lo, hi, 30, 3).cpu().numpy())
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("feat", [64, 1024])
def test_temporal_pooling_forward_windows(feat, report):
    from tennis_amd import weights as W
    from tennis_amd.engine import temporal_pool_windows
    from tennis_amd.models.vision.definitions import TemporalPooling
    centre, lo, hi, rows = _index_arrays()
    feats = np.random.default_rng(5).normal(0, 1, (rows, feat)).astype(np.float32)
    x = torch.from_numpy(feats).cuda()
    scale = float(np.abs(feats).max())
    worst = 0.0
    for kind in ("max", "mean"):
        tp = TemporalPooling(None, num_classes=CLASSES, pool=kind, feats=True, prefix=f"wintp_{kind}{feat}_")
        tp.initialize()
        q = W.make_dense_weights(6, CLASSES, feat, f"wintp_{kind}{feat}_dense0_")
        tp.set_params(q)
        wd, bd = q[f"wintp_{kind}{feat}_dense0_weight"].astype(np.float64), q[f"wintp_{kind}{feat}_dense0_bias"].astype(np.float64)
        for window in WINDOWS:
            for stride in STRIDES:
                win = feats[host_rows(centre, lo, hi, window, stride, rows)]
                got = temporal_pool_windows(x, centre, lo, hi, window, stride, kind).cpu().numpy()
                if kind == "max":
                    assert np.array_equal(got, win.max(1)), (window, stride)
                    ref = win.max(1).astype(np.float64)
                else:
                    ref = win.astype(np.float64).mean(1)
                    e = float(np.abs(got - ref).max()) / scale
                    worst = max(worst, e)
                    print(f"mean F={feat} window={window} stride={stride}: {e:.3e} of max|x|")
                    assert e < 1e-6, (window, stride, e)
                logits = tp.forward_windows(feats, centre, lo, hi, window, stride).cpu().numpy()
                if kind == "max":
                    assert np.array_equal(logits, tp(win).cpu().numpy())      # the loader path's very bits
                assert float(np.abs(logits - (ref @ wd.T + bd)).max()) < BAR
    report[f"temporal_pool_windows_mean_F{feat}_rel_maxabs"] = worst
    # index arrays that are already on the device (what evaluate.py --corpus_frames --dense_windows hands over)
    dev = [torch.from_numpy(a.astype(np.int32)).cuda() for a in (centre, lo, hi)]
    assert np.array_equal(tp.forward_windows(x, *dev, 7, 3).cpu().numpy(), tp.forward_windows(feats, centre, lo, hi, 7, 3).cpu().numpy())
    with pytest.raises(NotImplementedError):
        TemporalPooling(None, num_classes=CLASSES, pool="max", feats=False).forward_windows(feats, centre, lo, hi, 7)


def test_index_arrays_outside_the_matrix_are_clamped():
    """The kernels clamp every row index to [0, rows - 1] unconditionally, whatever centre / lo / hi hold.  The arrays below are
    outside the matrix in ways for which the clamp has a host equivalent (so the result is pinned, not just 'no fault'):
    lo far negative / hi far too large around centres inside (clamping [lo, hi] to the matrix is the same interval), and
    centres far outside a window with lo == hi (every step reads that one row either way)."""
    from tennis_amd.engine import WindowHead, temporal_pool_windows
    centre, lo, hi, rows = _index_arrays()
    feat, hidden = 64, 128
    feats = _features(rows, feat)
    x = torch.from_numpy(feats).cuda()
    c, l, h = centre.copy(), lo.copy(), hi.copy()
    l[:] = -1_000_000_000
    h[:] = 2_000_000_000
    l[5:9], h[5:9] = 7, 7
    c[5:7], c[7:9] = -1_000_000_000, 2_000_000_000
    l[20:24], h[20:24] = -5, -5                       # an interval wholly below the matrix: row 0
    l[30:34], h[30:34] = rows + 3, rows + 3           # ... and wholly above: the last row
    cc, lc, hc = (np.clip(a, 0, rows - 1) for a in (c, l, h))
    for window, stride in ((30, 3), (7, 1)):
        want = host_rows(cc, lc, hc, window, stride, rows)
        assert np.array_equal(host_rows(c, l, h, window, stride, rows), want)       # the host equivalent holds for these arrays
        for mode in ("gru", "lstm"):
            _, p, rp, dp = _model(mode, feat, hidden, f"clamp_{mode}")
            head = WindowHead(mode, feat, hidden, CLASSES, p, rp, dp, max_rows=rows, max_samples=rows).project(x)
            assert np.array_equal(head.forward(c, l, h, window, stride).cpu().numpy(), head.forward(cc, lc, hc, window, stride).cpu().numpy())
        for kind in ("max", "mean"):
            assert np.array_equal(temporal_pool_windows(x, c, l, h, window, stride, kind).cpu().numpy(),
                                  temporal_pool_windows(x, cc, lc, hc, window, stride, kind).cpu().numpy())


EVAL_SEED = 1      # chosen on the CPU: the float64 oracle's top-2 logit margin exceeds 1e-3 on every sample (asserted below)


def _eval_setup(tmp_path, seed=EVAL_SEED, write=True):
    import os
    from tennis_amd.dataset import TennisSet
    ds = TennisSet(root=str(tmp_path), videos=("V1", "V2", "V3"), frames_per_video=13, window=7, stride=2, feats_model="0006",
                   balance=False, synthetic=True)
    rng = np.random.default_rng(seed)
    feats = (np.abs(rng.normal(0, 1, (len(ds), 64))) * 0.5).astype(np.float32)
    if write:
        for s, row in zip(ds._samples, feats):
            path = ds.get_feature_path(ds.feat_dir, s[0], s[1])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, row)
    return ds, feats


def _eval_oracle(ds, feats, p, rp, dp):
    centre, lo, hi, rs = ds.window_rows()
    return oracle_f64(feats[host_rows(centre, lo, hi, ds._window, rs, len(ds))], p, "gru", rp, dp)[1]


def test_evaluate_windows_against_evaluate_model(tmp_path, report):
    from tennis_amd.dataset import DataLoader
    from tennis_amd.evaluate import evaluate_model, evaluate_windows
    from tennis_amd.metrics.vision import PRF1
    ds, feats = _eval_setup(tmp_path)
    m, p, rp, dp = _model("gru", 64, 128, "eval")
    ref = _eval_oracle(ds, feats, p, rp, dp)
    top2 = np.sort(ref, 1)[:, -2:]
    assert float((top2[:, 1] - top2[:, 0]).min()) > 1e-3          # the seed's property: no argmax within the bar of a tie
    m_loader, m_dense = [PRF1(label_names=ds.classes)], [PRF1(label_names=ds.classes)]
    res_a, gt_a = evaluate_model(m, DataLoader(ds, batch_size=16), ds, m_loader)
    res_b, gt_b = evaluate_windows(m, ds, m_dense)
    assert list(res_a) == list(res_b) and gt_a == gt_b
    keys = [ds.get_image_path(ds._frames_dir, s[0], s[1]) for s in ds._samples]
    a, b = np.stack([res_a[k] for k in keys]), np.stack([res_b[k] for k in keys])
    e_a, e_b = float(np.abs(a - ref).max()), float(np.abs(b - ref).max())
    report["evaluate_windows_logits_maxabs"], report["evaluate_model_window_logits_maxabs"] = e_b, e_a
    report["evaluate_windows_vs_model_maxabs"] = float(np.abs(a - b).max())
    assert e_a < BAR and e_b < BAR
    assert np.array_equal(m_loader[0].mat, m_dense[0].mat) and m_dense[0].mat.sum() == len(ds)
    # the matrix handed over instead of the files
    res_c, _ = evaluate_windows(m, ds, [PRF1(label_names=ds.classes)], features=feats)
    assert all(np.array_equal(res_b[k], res_c[k]) for k in keys)


def test_window_head_abi_errors():
    from tennis_amd import _lib
    from tennis_amd import weights as W
    from tennis_amd.engine import WindowHead, temporal_pool_windows
    p = W.make_rnn_weights(1, "gru", 32, 16, "w_gru0_")
    p.update(W.make_dense_weights(2, CLASSES, 32, "w_dense0_"))
    head = WindowHead("gru", 32, 16, CLASSES, p, "w_gru0_", "w_dense0_", max_rows=8, max_samples=4)
    idx = np.zeros(3, np.int32)
    with pytest.raises(RuntimeError, match="project"):
        head.forward(idx, idx, idx, 7)                                       # forward before project
    with pytest.raises(RuntimeError, match="max_rows"):
        head.project(torch.zeros((9, 32), device="cuda"))                    # 9 rows > max_rows 8
    with pytest.raises(RuntimeError, match="project"):
        head.forward(idx, idx, idx, 7)                                       # ... and a refused project leaves nothing projected
    with pytest.raises(ValueError):
        head.project(torch.zeros((4, 31), device="cuda"))                    # feature size mismatch
    head.project(torch.zeros((8, 32), device="cuda"))
    with pytest.raises(RuntimeError, match="max_samples"):
        head.forward(np.zeros(5, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32), 7)
    with pytest.raises(RuntimeError, match="window and stride"):
        head.forward(idx, idx, idx, 0)
    with pytest.raises(RuntimeError, match="window and stride"):
        head.forward(idx, idx, idx, 7, 0)
    assert head.forward(idx, idx, idx, 7).shape == (3, CLASSES)
    lib = _lib.load()
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, device="cuda")
    for args in ((None, _lib.ptr(d), _lib.ptr(d), _lib.ptr(d), 3, 7, 1, None, _lib.ptr(out)),
                 (head.handle, None, _lib.ptr(d), _lib.ptr(d), 3, 7, 1, None, _lib.ptr(out)),
                 (head.handle, _lib.ptr(d), None, _lib.ptr(d), 3, 7, 1, None, _lib.ptr(out)),
                 (head.handle, _lib.ptr(d), _lib.ptr(d), None, 3, 7, 1, None, _lib.ptr(out)),
                 (head.handle, _lib.ptr(d), _lib.ptr(d), _lib.ptr(d), 3, 7, 1, None, None)):
        assert lib.tn_window_head_forward(*args) == -1 and b"null" in lib.tn_last_error()
    assert lib.tn_window_head_project(head.handle, None, 4) == -1 and b"null" in lib.tn_last_error()
    assert lib.tn_window_head_project(None, _lib.ptr(out), 4) == -1 and b"null" in lib.tn_last_error()
    h = C.c_void_p()
    assert lib.tn_window_head_create(None, 0, 32, 16, CLASSES, None, 0, b"a", b"b", 8, 4, C.byref(h)) == -1
    q = dict(p)
    del q["w_dense0_bias"]
    with pytest.raises(RuntimeError, match="w_dense0_bias"):
        WindowHead("gru", 32, 16, CLASSES, q, "w_gru0_", "w_dense0_")
    with pytest.raises(RuntimeError):
        WindowHead("gru", 32, 1000, CLASSES, p, "w_gru0_", "w_dense0_")      # 3 * hidden > 1024
    x = torch.zeros((8, 32), device="cuda")
    with pytest.raises(RuntimeError, match="window and stride"):
        temporal_pool_windows(x, idx, idx, idx, 0, 1, "max")
    with pytest.raises(RuntimeError, match="window and stride"):
        temporal_pool_windows(x, idx, idx, idx, 7, 0, "mean")
    ctx = _lib.default_context()
    assert lib.tn_temporal_pool_windows(ctx.handle, None, 8, 32, _lib.ptr(d), _lib.ptr(d), _lib.ptr(d), 3, 7, 1, 0, _lib.ptr(out)) == -1
    assert b"null" in lib.tn_last_error()
    assert lib.tn_temporal_pool_windows(ctx.handle, _lib.ptr(x), 8, 32, _lib.ptr(d), _lib.ptr(d), _lib.ptr(d), 3, 7, 1, 5, _lib.ptr(out)) == -1
