"""-m gpu: temporal activation maps of the windowed heads (csrc/step_maps.hip, the ARG form of csrc/rnn_window.hip, the *_tam and
*_arg calls, engine / CNNRNN / TemporalPooling ``return_tam``, evaluate --save_tams).

References: tests/tools/step_maps_ref.py in float64 - the head's whole hidden sequence, first-maximum steps, and maps from given
pooled values and steps - and, for what must be the same bits, the calls without maps and numpy's own first arg-max.

Error bounds (u = 2^-24, fp32 round to nearest).
  * The kernel keeps ONE accumulator per (b, c, t), starts it at 0 and adds the bucket's terms W[c][k] * pooled[b][k] in ascending
    k with fmaf: the product is exact inside the fmaf, every step rounds once, so after n_t terms the computed sum is
    sum_k term_k * prod_{j >= k} (1 + d_j), |d_j| <= u, and |error| <= gamma_{n_t} * sum |term_k| with gamma_n = n u / (1 - n u)
    <= (n + 2) u for n <= 4096 (n^2 u <= 2).  The test compares against float64 of the SAME fp32 pooled / steps / W (its own error
    is 2^-29 of that bound): |tam - ref| <= (n_t + 2) u sum_bucket |W pooled|.
  * bias + sum_t tam against the logit: two fp32 evaluations of the same K-term sum plus bias in different orders, each within
    (K + 2) u (|bias| + sum_k |W pooled|) of the real value whatever the order: 2 (K + 2) u (|bias| + sum_k |W pooled|); the sum
    over t is taken on the host in float64.
Measured / bound go to the parity report."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_gpu_window_head import BAR, CLASSES, _features, _index_arrays, _model, host_rows
from test_gpu_window_rows import _free_table
from tools import step_maps_ref as SR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TIE = 2e-4            # twice the 1e-4 bar tests/test_gpu_window_head.py holds pooled to
FEAT = 64
CELLS = [(m, h) for m in ("gru", "lstm") for h in (128, 32, 8)]      # register-resident DPP, streamed DPP, plain


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


# ---- (a) the kernel alone ------------------------------------------------------------------------------------------------------

# every K of {16, 256, 1000, 4096}, C of {1, 11, 33}, T of {1, 2, 7, 30, 65}, B of {1, 3, 130}
SHAPES = [(16, 1, 1, 1), (16, 11, 30, 3), (256, 11, 30, 130), (256, 33, 7, 3), (1000, 11, 65, 3), (1000, 1, 2, 130), (4096, 11, 30, 3),
          (4096, 33, 65, 1), (4096, 1, 7, 3)]


def _step_patterns(rng, B, K, T):
    random = rng.integers(0, T, (B, K))
    one = np.full((B, K), T - 1 if T > 1 else 0)
    one[0] = 0
    once = np.where(rng.random((B, K)) < 0.5, -1, T)            # every step named at most once, everything else out of range
    for b in range(B):
        at = rng.permutation(K)[:min(K, T)]
        once[b, at] = rng.permutation(T)[:len(at)]
    holes = random.copy()
    holes[rng.random((B, K)) < 0.2] = -1
    holes[rng.random((B, K)) < 0.2] = T
    holes[:, 0] = -2_000_000_000
    holes[:, -1] = 2_000_000_000
    return dict(random=random, one_step=one, once=once, out_of_range=holes)


@pytest.mark.parametrize("K,Cn,T,B", SHAPES)
def test_step_maps_kernel_against_float64(K, Cn, T, B, report):
    from tennis_amd.engine import Dense
    rng = np.random.default_rng(K + 7 * Cn + 13 * T + B)
    w = rng.normal(0, 1, (Cn, K)).astype(np.float32)
    dense = Dense(w, rng.normal(0, 1, Cn).astype(np.float32))
    worst = 0.0
    for name, steps in _step_patterns(rng, B, K, T).items():
        pooled = rng.normal(0, 1, (B, K)).astype(np.float32)
        got = dense.step_maps(torch.from_numpy(pooled).cuda(), torch.from_numpy(steps.astype(np.int32)).cuda(), T).cpu().numpy()
        assert got.shape == (B, Cn, T) and got.dtype == np.float32
        ref = SR.step_maps(pooled, steps, w, T)
        mass, sizes = SR.step_maps_abs(pooled, steps, w, T)
        bound = (sizes[:, None, :] + 2) * U * mass
        err = np.abs(got - ref)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print(f"K={K} C={Cn} T={T} B={B} {name}: measured / bound {ratio:.3f}")
        assert np.all(err <= bound), (name, ratio)
        empty = np.broadcast_to((sizes == 0)[:, None, :], got.shape)
        assert np.all(got[empty] == 0.0) and not np.any(np.signbit(got[empty])), name      # exact +0.0f
        if name == "once":
            assert sizes.max() == 1 and np.all(sizes.sum(1) == min(K, T))
        if name == "out_of_range":       # the entries outside [0, T) contribute nothing: the same bits with their pooled values wrecked
            wreck = pooled.copy()
            wreck[(steps < 0) | (steps >= T)] = 1e30
            again = dense.step_maps(torch.from_numpy(wreck).cuda(), torch.from_numpy(steps.astype(np.int32)).cuda(), T).cpu().numpy()
            assert np.array_equal(again, got)
    report[f"step_maps_K{K}_C{Cn}_T{T}_B{B}_measured_over_bound"] = worst


def test_step_maps_do_not_depend_on_the_batch():
    from tennis_amd.engine import Dense
    rng = np.random.default_rng(3)
    K, Cn, T, B = 256, 11, 30, 130
    dense = Dense(rng.normal(0, 1, (Cn, K)).astype(np.float32), None)
    pooled = torch.from_numpy(rng.normal(0, 1, (B, K)).astype(np.float32)).cuda()
    steps = torch.from_numpy(rng.integers(-1, T + 1, (B, K)).astype(np.int32)).cuda()
    full = dense.step_maps(pooled, steps, T).cpu().numpy()
    for b in (0, 77, 129):
        assert np.array_equal(dense.step_maps(pooled[b:b + 1], steps[b:b + 1], T).cpu().numpy()[0], full[b]), b
    assert np.array_equal(dense.step_maps(pooled[64:67], steps[64:67], T).cpu().numpy(), full[64:67])


# ---- (b) the windowed head -------------------------------------------------------------------------------------------------------

def _head(mode, hidden, tag, feats):
    from tennis_amd.engine import WindowHead
    m, p, rp, dp = _model(mode, FEAT, hidden, f"tam_{tag}_{mode}{hidden}")
    rows = feats.shape[0]
    head = WindowHead(mode, FEAT, hidden, CLASSES, p, rp, dp, max_rows=rows, max_samples=max(rows, 64))
    return head.project(torch.from_numpy(feats).cuda()), m, p, rp, dp


def _judge_steps(h64, steps, cap, what):
    """the two judgements of the steps against the float64 sequence h64 (S, T, K); -> (share left out of the exact check, worst
    shortfall of the chosen step's float64 value below the float64 maximum)"""
    ref_steps, ref_pooled = SR.first_max(h64)
    chosen = np.take_along_axis(h64, steps[:, None, :].astype(np.int64), 1)[:, 0]
    short = float((ref_pooled - chosen).max())
    assert steps.min() >= 0 and steps.max() < h64.shape[1], what
    assert short <= TIE, (what, short)
    clear = SR.margin(h64) > TIE
    assert np.array_equal(steps[clear], ref_steps[clear]), what
    out = 1.0 - float(clear.mean())
    assert out <= cap, (what, out, cap)
    return out, short


def _check_maps(pooled, steps, tam, p, dp, window):
    wd = p[dp + "weight"]
    mass, sizes = SR.step_maps_abs(pooled, steps, wd, window)
    err = np.abs(tam - SR.step_maps(pooled, steps, wd, window))
    bound = (sizes[:, None, :] + 2) * U * mass
    assert np.all(err <= bound)
    assert np.all(tam[np.broadcast_to((sizes == 0)[:, None, :], tam.shape)] == 0.0)
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("mode,hidden", CELLS)
def test_window_head_steps_and_maps_on_clamped_windows(mode, hidden, report):
    centre, lo, hi, rows = _index_arrays()
    feats = _features(rows, FEAT)
    head, m, p, rp, dp = _head(mode, hidden, "win", feats)
    worst_out, worst_ratio = 0.0, 0.0
    for window in (2, 7, 30):
        for stride in (1, 3):
            what = (mode, hidden, window, stride)
            want_l, want_p = _np(*head.forward(centre, lo, hi, window, stride, return_pooled=True))
            l, pl, tam, steps = _np(*head.forward(centre, lo, hi, window, stride, return_pooled=True, return_tam=True, return_steps=True))
            assert tam.shape == (rows, CLASSES, window) and steps.shape == (rows, 2 * hidden) and steps.dtype == np.int32
            assert np.array_equal(l, want_l) and np.array_equal(pl, want_p), what           # the bits of the call without maps
            only_l, only_t = _np(*head.forward(centre, lo, hi, window, stride, return_tam=True))
            assert np.array_equal(only_l, want_l) and np.array_equal(only_t, tam), what
            idx = host_rows(centre, lo, hi, window, stride, rows)
            rl, rp_, rt, rs = _np(*head.forward_rows(idx, return_pooled=True, return_tam=True, return_steps=True))
            assert np.array_equal(rl, want_l) and np.array_equal(rp_, want_p), what
            assert np.array_equal(rs, steps) and np.array_equal(rt, tam), what              # the table form: the same steps and maps
            h64 = SR.head_sequence(feats[idx], p, mode, rp)
            out, short = _judge_steps(h64, steps, 0.25, what)
            worst_out = max(worst_out, out)
            worst_ratio = max(worst_ratio, _check_maps(pl, steps, tam, p, dp, window))
            print(f"{mode} H={hidden} window={window} stride={stride}: left out {out:.4f} shortfall {short:.2e}")
            if mode == "lstm":       # the windowed LSTM kernel is bit-equal to the sample route: the materialised sequence itself
                seq = m.rnn(feats[idx]).cpu().numpy()
                assert np.array_equal(np.take_along_axis(seq, steps[:, None, :].astype(np.int64), 1)[:, 0], pl), what
                assert np.array_equal(steps, np.argmax(seq, axis=1)), what
    report[f"window_head_tam_{mode}_H{hidden}_clamped_left_out"] = worst_out
    report[f"window_head_tam_{mode}_H{hidden}_clamped_measured_over_bound"] = worst_ratio


def _free_table_tam(rng, samples, window, rows):
    """the free tables of tests/test_gpu_window_rows.py with one row replaced: its constant table row (every step reads row 5) lets
    the state converge exactly as a clamped window does - at window 30 half of that sample's units end within 2e-4 of a tie, and the
    float64 head alone then leaves up to 3.04 % of a table's units out of the exact check (LSTM H = 8), over the 3 % cap.  Converging
    windows are the clamped test's ground, under its own cap; here the row reads pairs of repeated rows instead.  Float64 head alone
    with this generator, measured on the CPU: at most 1.86 % left out (LSTM H = 8, window 30)."""
    idx = _free_table(rng, samples, window, rows)
    idx[2] = np.repeat(rng.integers(0, rows, (window + 1) // 2), 2)[:window]
    return idx


@pytest.mark.parametrize("mode,hidden", CELLS)
def test_window_head_steps_and_maps_on_free_tables(mode, hidden, report):
    _, _, _, rows = _index_arrays()
    feats = _features(rows, FEAT, seed=2)
    head, m, p, rp, dp = _head(mode, hidden, "free", feats)
    rng = np.random.default_rng(11)
    worst_out = 0.0
    for window in (2, 7, 30):
        idx = _free_table_tam(rng, 37, window, rows)
        want_l, want_p = _np(*head.forward_rows(idx, return_pooled=True))
        l, pl, tam, steps = _np(*head.forward_rows(idx, return_pooled=True, return_tam=True, return_steps=True))
        assert np.array_equal(l, want_l) and np.array_equal(pl, want_p), window
        out, short = _judge_steps(SR.head_sequence(feats[idx], p, mode, rp), steps, 0.03, (mode, hidden, window))
        worst_out = max(worst_out, out)
        _check_maps(pl, steps, tam, p, dp, window)
        print(f"{mode} H={hidden} window={window}: left out {out:.4f} shortfall {short:.2e}")
        if mode == "lstm":
            seq = m.rnn(feats[idx]).cpu().numpy()
            assert np.array_equal(np.take_along_axis(seq, steps[:, None, :].astype(np.int64), 1)[:, 0], pl), window
            assert np.array_equal(steps, np.argmax(seq, axis=1)), window
    report[f"window_head_tam_{mode}_H{hidden}_free_left_out"] = worst_out


@pytest.mark.parametrize("mode,hidden", CELLS)
def test_sample_counts_around_the_rows_per_workgroup(mode, hidden):
    """one below, at and one above each rows-per-workgroup value (the plain LSTM form keeps its steps at 4 rows whatever is asked):
    a sample's steps and maps do not depend on how many samples the call carries or how they are grouped"""
    centre, lo, hi, rows = _index_arrays()
    head, *_ = _head(mode, hidden, "nb", _features(rows, FEAT))
    window, stride = 7, 1
    idx = host_rows(centre, lo, hi, window, stride, rows)
    full = _np(*head.forward(centre, lo, hi, window, stride, return_pooled=True, return_tam=True, return_steps=True))
    for nb in (4, 6 if mode == "gru" else 8):
        head._set_rows_per_group(nb)
        for n in (nb - 1, nb, nb + 1, 2 * nb + 1):
            a = _np(*head.forward(centre[:n], lo[:n], hi[:n], window, stride, return_pooled=True, return_tam=True, return_steps=True))
            b = _np(*head.forward_rows(idx[:n], return_pooled=True, return_tam=True, return_steps=True))
            for got_a, got_b, want in zip(a, b, full):
                assert np.array_equal(got_a, want[:n]) and np.array_equal(got_b, want[:n]), (nb, n)
            plain = _np(*head.forward(centre[:n], lo[:n], hi[:n], window, stride, return_pooled=True))      # this grouping's kernel without maps
            assert np.array_equal(plain[0], a[0]) and np.array_equal(plain[1], a[1]), (nb, n)


# ---- (c) the identity through every route ----------------------------------------------------------------------------------------

def _identity(logits, tam, pooled, wd, bias, what, report=None, key=None):
    """|bias + sum_t tam - logit| <= 2 (K + 2) u (|bias| + sum_k |W pooled|), the sum over t in float64 on the host"""
    K = pooled.shape[1]
    wd, bias = wd.astype(np.float64), bias.astype(np.float64)
    err = np.abs(bias + tam.astype(np.float64).sum(2) - logits)
    bound = 2 * (K + 2) * U * (np.abs(bias) + np.abs(pooled.astype(np.float64)) @ np.abs(wd).T)
    ratio = float((err / bound).max())
    print(f"{what}: identity measured / bound {ratio:.4f}")
    if report is not None:
        report[key] = max(report.get(key, 0.0), ratio)
    assert np.all(err <= bound), (what, ratio)
    return ratio


@pytest.mark.parametrize("mode", ["gru", "lstm"])
def test_identity_through_every_cnnrnn_route(mode, report):
    from tennis_amd.engine import temporal_pool
    centre, lo, hi, rows = _index_arrays()
    feats = _features(rows, FEAT)
    m, p, rp, dp = _model(mode, FEAT, 128, f"tam_routes_{mode}")
    wd, bias = p[dp + "weight"], p[dp + "bias"]
    videos = [v for v, n in enumerate((5, 40, 17, 1)) for _ in range(n)]
    key = f"tam_identity_cnnrnn_{mode}_measured_over_bound"
    for window, stride in ((7, 1), (30, 3)):
        idx = host_rows(centre, lo, hi, window, stride, rows)
        # forward on the materialised windows
        x = feats[idx]
        logits, tam = _np(*m.forward(x, return_tam=True))
        assert tam.shape == (rows, CLASSES, window)
        assert np.array_equal(logits, m(x).cpu().numpy())
        pooled = temporal_pool(m.rnn(x), "max").cpu().numpy()
        _identity(logits, tam, pooled, wd, bias, (mode, "forward", window), report, key)
        # forward_windows, whole and cut at the video boundaries
        want = m.forward_windows(feats, centre, lo, hi, window, stride).cpu().numpy()
        logits, tam = _np(*m.forward_windows(feats, centre, lo, hi, window, stride, return_tam=True))
        assert np.array_equal(logits, want)
        pooled = m._engine.forward(centre, lo, hi, window, stride, return_pooled=True)[1].cpu().numpy()
        _identity(logits, tam, pooled, wd, bias, (mode, "forward_windows", window), report, key)
        cut_l, cut_t = _np(*m.forward_windows(feats, centre, lo, hi, window, stride, max_rows=45, return_tam=True))
        assert np.array_equal(cut_l, m.forward_windows(feats, centre, lo, hi, window, stride, max_rows=45).cpu().numpy())
        assert np.array_equal(cut_t, tam)                       # a sample's pooled vector, steps and maps do not depend on the cut
        _identity(cut_l, cut_t, pooled, wd, bias, (mode, "forward_windows cut", window), report, key)
        # forward_table, whole and in two pieces
        tl, tt = _np(*m.forward_table(feats, idx, return_tam=True))
        assert np.array_equal(tl, m.forward_table(feats, idx).cpu().numpy()) and np.array_equal(tt, tam)
        _identity(tl, tt, pooled, wd, bias, (mode, "forward_table", window), report, key)
        pl, pt = _np(*m.forward_table(feats, idx, max_rows=45, row_videos=videos, return_tam=True))
        assert np.array_equal(pl, m.forward_table(feats, idx, max_rows=45, row_videos=videos).cpu().numpy()) and np.array_equal(pt, tam)
        _identity(pl, pt, pooled, wd, bias, (mode, "forward_table cut", window), report, key)


@pytest.mark.parametrize("feat", [64, 1000])
def test_identity_through_every_temporal_pooling_route(feat, report):
    from tennis_amd import weights as W
    from tennis_amd.engine import temporal_pool, temporal_pool_rows, temporal_pool_windows
    from tennis_amd.models.vision.definitions import TemporalPooling
    centre, lo, hi, rows = _index_arrays()
    feats = np.random.default_rng(5).normal(0, 1, (rows, feat)).astype(np.float32)
    x = torch.from_numpy(feats).cuda()
    pre = f"tamtp_{feat}_"
    tp = TemporalPooling(None, num_classes=CLASSES, pool="max", feats=True, prefix=pre)
    tp.initialize()
    q = W.make_dense_weights(6, CLASSES, feat, pre + "dense0_")
    tp.set_params(q)
    wd, bias = q[pre + "dense0_weight"], q[pre + "dense0_bias"]
    videos = [v for v, n in enumerate((5, 40, 17, 1)) for _ in range(n)]
    key = f"tam_identity_temporal_pooling_F{feat}_measured_over_bound"
    for window, stride in ((2, 1), (7, 3), (30, 1)):
        idx = host_rows(centre, lo, hi, window, stride, rows)
        win = feats[idx]
        first = np.argmax(win, axis=1)                          # a maximum is exact: numpy's first arg-max, exactly
        for y, steps in (temporal_pool(torch.from_numpy(win).cuda(), "max", return_steps=True),
                         temporal_pool_windows(x, centre, lo, hi, window, stride, "max", return_steps=True),
                         temporal_pool_rows(x, idx, "max", return_steps=True)):
            assert steps.dtype == torch.int32 and np.array_equal(steps.cpu().numpy(), first), (window, stride)
            assert np.array_equal(y.cpu().numpy(), win.max(1))
        assert np.array_equal(temporal_pool_windows(x, centre, lo, hi, window, stride, "max").cpu().numpy(), win.max(1))
        tam0 = None
        for what, call in (("forward", lambda **k: tp.forward(win, **k)),
                           ("forward_windows", lambda **k: tp.forward_windows(feats, centre, lo, hi, window, stride, **k)),
                           ("forward_windows cut", lambda **k: tp.forward_windows(feats, centre, lo, hi, window, stride, max_rows=45, **k)),
                           ("forward_table", lambda **k: tp.forward_table(feats, idx, **k)),
                           ("forward_table cut", lambda **k: tp.forward_table(feats, idx, max_rows=45, row_videos=videos, **k))):
            logits, tam = _np(*call(return_tam=True))
            assert tam.shape == (rows, CLASSES, window)
            assert np.array_equal(logits, call().cpu().numpy()), what
            _identity(logits, tam, win.max(1), wd, bias, (feat, what, window), report, key)
            tam0 = tam if tam0 is None else tam0
            assert np.array_equal(tam, tam0), what              # one pooled vector, one set of steps: one set of maps
    with pytest.raises(ValueError, match="max pool"):
        temporal_pool(x[None], "mean", return_steps=True)
    with pytest.raises(ValueError, match="max pool"):
        temporal_pool_rows(x, idx, "mean", return_steps=True)
    with pytest.raises(ValueError, match="max pool"):
        temporal_pool_windows(x, centre, lo, hi, 7, 1, "mean", return_steps=True)


# ---- (d) CNNRNN on frames --------------------------------------------------------------------------------------------------------

def test_cnnrnn_on_frames(report):
    from tennis_amd import weights as W
    from tennis_amd.engine import temporal_pool
    from tennis_amd.model_zoo import get_model
    from tennis_amd.models.vision.definitions import CNNRNN, FrameModel
    fm = FrameModel(get_model("DenseNet121", pretrained=True, seed=0).features, CLASSES, prefix="framemodel0_")
    pre = "tamframes_"
    m = CNNRNN(fm, num_classes=CLASSES, type="gru", hidden_size=128, prefix=pre)
    m.initialize()
    q = W.make_densenet121_weights(0)
    q.update(W.make_dense_weights(1, CLASSES, 1024, "framemodel0_dense0_"))
    q.update(W.make_rnn_weights(3, "gru", 1024, 128, pre + "gru0_"))
    q.update(W.make_dense_weights(4, CLASSES, 256, pre + "dense0_"))
    m.set_params(q)
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(8, 224)).reshape(2, 4, 3, 224, 224)
    logits, tam = _np(*m.forward(x, return_tam=True))
    assert logits.shape == (2, CLASSES) and tam.shape == (2, CLASSES, 4)
    assert np.array_equal(logits, m.forward(x).cpu().numpy())
    pooled = temporal_pool(m.rnn(m.td(x)), "max").cpu().numpy()
    _identity(logits, tam, pooled, q[pre + "dense0_weight"], q[pre + "dense0_bias"], "cnnrnn on frames", report,
              "tam_identity_cnnrnn_frames_measured_over_bound")


# ---- (e) the driver --------------------------------------------------------------------------------------------------------------

def _scores(out):
    """the confusion matrix and the [Finished] line without its time"""
    text = out[out.index("Test set:"):]
    return text[:text.index("Time Taken")]


@pytest.mark.parametrize("dense", [False, True])
def test_evaluate_main_save_tams(tmp_path, capsys, monkeypatch, dense, report):
    from tennis_amd import evaluate as ev
    from tennis_amd.dataset import TennisSet
    from tennis_amd.engine import temporal_pool
    from tennis_amd.models.vision import definitions as D
    made, init = [], D.CNNRNN.__init__

    def recording(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(D.CNNRNN, "__init__", recording)
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    args = ["--root", root, "--frames_per_video", "9", "--data_shape", "224", "--window", "4", "--stride", "2", "--temp_pool", "gru",
            "--batch_size", "4", "--exp_root", exp] + (["--dense_windows"] if dense else [])
    tams_file = os.path.join(exp, "0000", "test_tams.npz")
    assert ev.main(args) == 0
    plain = capsys.readouterr().out
    assert not os.path.exists(tams_file)
    assert ev.main(args + ["--save_tams"]) == 0
    out = capsys.readouterr().out
    assert _scores(out) == _scores(plain)                                        # the metrics and every printed score
    assert os.path.exists(tams_file) and "temporal activation maps" in out
    ds = TennisSet(root=root, window=4, stride=2, frames_per_video=9, data_shape=224, split="test", balance=False)
    d = ev.load_tams(tams_file)
    n = len(ds)
    assert all(len(d[k]) == n for k in ev.TAM_COLUMNS) and d["tam"].shape == (n, 4) and d["frames"].shape == (n, 4)
    frames, idx = ds.window_table()
    assert np.array_equal(d["frames"], np.asarray([[frames[r][1] for r in row] for row in idx]))
    assert all(frames[r][0] == v for row, v in zip(idx, d["video"]) for r in row)
    assert list(d["video"]) == [s[0] for s in ds._samples] and list(d["frame"]) == [int(s[1]) for s in ds._samples]
    assert list(d["label"]) == [ds.classes.index(s[2]) for s in ds._samples]
    # the identity, with the route's own pooled vectors recomputed from the model the driver built (the encoder is batch independent)
    m = made[-1]
    table = ev.encode_table(m.td.model, ds, frames, batch_size=4)
    if dense:
        logits, pooled = _np(*m._engine.project(table).forward_rows(idx, return_pooled=True))
    else:
        pooled = temporal_pool(m.rnn(table[torch.from_numpy(idx).long().cuda()]), "max")
        logits, pooled = _np(m.classes(pooled), pooled)
    at = np.arange(n)
    assert np.array_equal(d["pred"], logits.argmax(1)) and np.array_equal(d["logit"], logits[at, d["pred"]])
    wd = np.asarray(m.classes._own_params[m.classes.prefix + "weight"].data, np.float32)
    bias = np.asarray(m.classes._own_params[m.classes.prefix + "bias"].data, np.float32).reshape(-1)
    assert np.array_equal(d["bias"], bias[d["pred"]])
    err = np.abs(d["bias"].astype(np.float64) + d["tam"].astype(np.float64).sum(1) - d["logit"])
    bound = 2 * (pooled.shape[1] + 2) * U * (np.abs(d["bias"].astype(np.float64)) + (np.abs(pooled.astype(np.float64)) * np.abs(wd[d["pred"]].astype(np.float64))).sum(1))
    ratio = float((err / bound).max())
    report[f"save_tams_{'dense' if dense else 'loader'}_identity_measured_over_bound"] = ratio
    assert np.all(err <= bound), ratio


# ---- (f) ABI errors --------------------------------------------------------------------------------------------------------------

def test_abi_errors():
    from tennis_amd import _lib
    from tennis_amd import weights as W
    from tennis_amd.engine import Dense, WindowHead
    p = W.make_rnn_weights(1, "gru", 32, 16, "w_gru0_")
    p.update(W.make_dense_weights(2, CLASSES, 32, "w_dense0_"))
    head = WindowHead("gru", 32, 16, CLASSES, p, "w_gru0_", "w_dense0_", max_rows=8, max_samples=4)
    lib = _lib.load()
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    st = torch.zeros(4 * 32, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, device="cuda")
    tam = torch.zeros(4 * CLASSES * 7, device="cuda")
    P = _lib.ptr

    def refused(rc, text):
        return rc == -1 and text in lib.tn_last_error()
    fwd = lambda **k: lib.tn_window_head_forward_tam(k.get("h", head.handle), k.get("c", P(d)), k.get("lo", P(d)), k.get("hi", P(d)), k.get("n", 3),
                                                     k.get("w", 7), k.get("s", 1), None, k.get("l", P(out)), k.get("st", P(st)), k.get("tam", P(tam)))
    rws = lambda **k: lib.tn_window_head_forward_rows_tam(k.get("h", head.handle), k.get("idx", P(d)), k.get("n", 3), k.get("w", 7), None,
                                                          k.get("l", P(out)), k.get("st", P(st)), k.get("tam", P(tam)))
    assert refused(fwd(), b"project") and refused(rws(), b"project")             # before project
    head.project(torch.zeros((8, 32), device="cuda"))
    for bad in (dict(h=None), dict(c=None), dict(lo=None), dict(hi=None), dict(l=None), dict(tam=None)):
        assert refused(fwd(**bad), b"null"), bad
    for bad in (dict(h=None), dict(idx=None), dict(l=None), dict(tam=None)):
        assert refused(rws(**bad), b"null"), bad
    assert refused(fwd(n=5), b"max_samples") and refused(fwd(n=0), b"max_samples") and refused(rws(n=5), b"max_samples")
    assert refused(fwd(w=0), b"window") and refused(fwd(s=0), b"stride") and refused(rws(w=0), b"window")
    assert fwd() == 0 and rws() == 0 and fwd(st=None) == 0 and rws(st=None) == 0      # steps may be NULL: the handle's own buffer
    ctx = _lib.default_context()
    x = torch.zeros((8, 32), device="cuda")
    arg = torch.zeros(3 * 32, dtype=torch.int32, device="cuda")
    y = torch.zeros(3 * 32, device="cuda")
    pa = lambda **k: lib.tn_temporal_pool_arg(k.get("ctx", ctx.handle), k.get("x", P(x)), k.get("b", 2), k.get("t", 4), k.get("f", 32), k.get("y", P(y)),
                                              k.get("arg", P(arg)))
    pw = lambda **k: lib.tn_temporal_pool_windows_arg(k.get("ctx", ctx.handle), k.get("x", P(x)), k.get("rows", 8), 32, k.get("c", P(d)), k.get("lo", P(d)),
                                                      k.get("hi", P(d)), k.get("n", 3), k.get("w", 7), k.get("s", 1), k.get("y", P(y)), k.get("arg", P(arg)))
    pr = lambda **k: lib.tn_temporal_pool_rows_arg(k.get("ctx", ctx.handle), k.get("x", P(x)), k.get("rows", 8), 32, k.get("idx", P(d)), k.get("n", 3),
                                                   k.get("w", 7), k.get("y", P(y)), k.get("arg", P(arg)))
    for bad in (dict(ctx=None), dict(x=None), dict(y=None), dict(arg=None)):
        assert refused(pa(**bad), b"null") and refused(pw(**bad), b"null") and refused(pr(**bad), b"null"), bad
    assert refused(pw(c=None), b"null") and refused(pw(lo=None), b"null") and refused(pw(hi=None), b"null") and refused(pr(idx=None), b"null")
    assert refused(pa(t=0), b"shape") and refused(pa(b=0), b"shape") and refused(pw(rows=0), b"shape") and refused(pr(n=0), b"shape")
    assert refused(pw(w=0), b"window") and refused(pw(s=0), b"stride") and refused(pr(w=0), b"window")
    assert pa() == 0 and pw() == 0 and pr() == 0
    dense = Dense(p["w_dense0_weight"], p["w_dense0_bias"])
    pooled = torch.zeros((3, 32), device="cuda")
    sm = lambda **k: lib.tn_dense_step_maps(k.get("d", dense.handle), k.get("p", P(pooled)), k.get("st", P(st)), k.get("b", 3), k.get("w", 7),
                                            k.get("tam", P(tam)))
    for bad in (dict(d=None), dict(p=None), dict(st=None), dict(tam=None)):
        assert refused(sm(**bad), b"null"), bad
    assert refused(sm(w=0), b"window") and refused(sm(b=0), b"batch") and sm() == 0
    with pytest.raises(ValueError, match="pooled and steps"):
        dense.step_maps(pooled[:, :31], st[:96].reshape(3, 32), 7)
    torch.cuda.synchronize()
