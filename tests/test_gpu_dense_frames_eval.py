"""-m gpu: dense evaluation of temporal models ON FRAMES (evaluate.encode_table / evaluate_table, CNNRNN / TemporalPooling
.forward_table, evaluate --dense_windows without --feats_model): every distinct frame the windows read is decoded and encoded once,
the windows are gathered on the GPU from the table of its feature rows.

References: the loader route (evaluate_model over DataLoader: every window materialised, every frame encoded once per window that
reads it) and the float64 head of tests/test_gpu_window_head.py evaluated on the device's own feature rows; bar 1e-4, that file's
figure for the head.  The encoder is batch independent (a stated property of the project), so the table's rows must be the bits of
the backbone applied to the same frames in one batch.  224 x 224 frames (the encoder's smallest size), at most 30 distinct frames."""
import numpy as np
import pytest
import torch

from test_gpu_window_head import BAR, oracle_f64

pytestmark = pytest.mark.gpu

CLASSES = 11
SPLITS = {"plain": dict(stride=2), "no_window_rows": dict(every=2, stride=3, split_first=4)}


@pytest.fixture(scope="module")
def zoo():
    from tennis_amd import weights as W
    from tennis_amd.model_zoo import get_model
    from tennis_amd.models.vision.definitions import FrameModel
    backbone = get_model("DenseNet121", pretrained=True, seed=0).features
    fm = FrameModel(backbone, CLASSES, prefix="framemodel0_")
    fm.initialize(); fm.hybridize()
    p = W.make_densenet121_weights(0)
    p.update(W.make_dense_weights(1, CLASSES, 1024, "framemodel0_dense0_"))
    fm.set_params(p)
    return fm, p


def _dataset(tmp_path, split):
    from tennis_amd.dataset import TennisSet
    return TennisSet(root=str(tmp_path), synthetic=True, videos=("V1", "V2"), frames_per_video=9, window=4, data_shape=224,
                     balance=False, **SPLITS[split])


def _cnnrnn(zoo, mode):
    from tennis_amd import weights as W
    from tennis_amd.models.vision.definitions import CNNRNN
    fm, p = zoo
    pre = f"densefr_{mode}_"
    m = CNNRNN(fm, num_classes=CLASSES, type=mode, hidden_size=128, prefix=pre)
    m.initialize()
    q = dict(p)
    q.update(W.make_rnn_weights(3, mode, 1024, 128, f"{pre}{mode}0_"))
    q.update(W.make_dense_weights(4, CLASSES, 256, f"{pre}dense0_"))
    m.set_params(q)
    return m, q, f"{pre}{mode}0_", f"{pre}dense0_"


def _stack(res, keys):
    return np.stack([res[k] for k in keys])


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("mode", ["gru", "lstm"])
def test_cnnrnn_dense_frames_route(zoo, tmp_path, report, mode, split):
    from tennis_amd.dataset import DataLoader
    from tennis_amd.evaluate import encode_table, evaluate_model, evaluate_table
    from tennis_amd.metrics.vision import PRF1
    ds = _dataset(tmp_path, split)
    if split == "no_window_rows":
        with pytest.raises(ValueError):
            ds.window_rows()
    frames, idx = ds.window_table()
    assert len(frames) <= 30
    if split == "no_window_rows":
        assert set(frames) - {(s[0], s[1]) for s in ds._samples}                 # windows reach frames that are no sample
    m, q, rp, dp = _cnnrnn(zoo, mode)
    # the table: every frame once, in batches of 4, the bits of one batch of all of them
    table = encode_table(m.td.model, ds, frames, batch_size=4)
    assert table.shape == (len(frames), 1024) and table.dtype == torch.float32 and table.is_cuda
    one = m.td.model(np.stack([ds._load(v, f) for v, f in frames])).cpu().numpy()
    assert np.array_equal(table.cpu().numpy(), one)
    ref = oracle_f64(one[idx], q, mode, rp, dp)[1]                             # float64 head on the device's own feature rows
    m_loader, m_dense = [PRF1(label_names=ds.classes)], [PRF1(label_names=ds.classes)]
    res_a, gt_a = evaluate_model(m, DataLoader(ds, batch_size=4), ds, m_loader)
    res_b, gt_b = evaluate_table(m, ds, m_dense, batch_size=4)
    assert list(res_a) == list(res_b) and gt_a == gt_b
    keys = [ds.get_image_path(ds._frames_dir, s[0], s[1]) for s in ds._samples]
    assert list(res_b) == keys
    a, b = _stack(res_a, keys), _stack(res_b, keys)
    e_a, e_b = float(np.abs(a - ref).max()), float(np.abs(b - ref).max())
    print(f"{mode} {split}: loader {e_a:.3e} dense {e_b:.3e} |a-b| {float(np.abs(a - b).max()):.3e}")
    report[f"dense_frames_{mode}_{split}_loader_logits_maxabs"], report[f"dense_frames_{mode}_{split}_dense_logits_maxabs"] = e_a, e_b
    report[f"dense_frames_{mode}_{split}_routes_maxabs"] = float(np.abs(a - b).max())      # recorded, not asserted
    if mode == "lstm":
        report[f"dense_frames_lstm_{split}_routes_bit_equal"] = bool(np.array_equal(a, b))  # recorded, not asserted
    assert e_a < BAR and e_b < BAR, (e_a, e_b)
    gt = np.asarray([gt_b[k] for k in keys])
    host = np.zeros((CLASSES, CLASSES))
    np.add.at(host, (gt, b.argmax(1)), 1)
    assert np.array_equal(m_dense[0].mat, host) and m_dense[0].mat.sum() == len(ds)
    # the table handed over: nothing is encoded again, the same bits
    res_c, _ = evaluate_table(m, ds, [PRF1(label_names=ds.classes)], features=table, frames_idx=(frames, idx))
    assert np.array_equal(_stack(res_c, keys), b)
    with pytest.raises(ValueError, match="recurrent layer takes"):
        m.forward_table(table[:, :512], idx)
    with pytest.raises(NotImplementedError):                                     # forward_windows keeps its refusal on frames
        m.forward_windows(table, idx[:, 0], idx[:, 0], idx[:, 0], 4)


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_temporal_pooling_dense_frames_route_gives_the_loader_routes_bits(zoo, tmp_path, pool):
    from tennis_amd.dataset import DataLoader
    from tennis_amd.evaluate import evaluate_model, evaluate_table
    from tennis_amd.metrics.vision import PRF1
    from tennis_amd.models.vision.definitions import TemporalPooling
    fm, _ = zoo
    for split in SPLITS:
        ds = _dataset(tmp_path, split)
        tp = TemporalPooling(fm, pool=pool, num_classes=0, feats=False)          # evaluate.py:242-244: the frame model's Dense
        assert tp.classes is fm.classes and tp.td.model is fm.backbone
        m_loader, m_dense = [PRF1(label_names=ds.classes)], [PRF1(label_names=ds.classes)]
        res_a, gt_a = evaluate_model(tp, DataLoader(ds, batch_size=4), ds, m_loader)
        res_b, gt_b = evaluate_table(tp, ds, m_dense, batch_size=4)
        assert list(res_a) == list(res_b) and gt_a == gt_b
        keys = list(res_a)
        assert np.array_equal(_stack(res_a, keys), _stack(res_b, keys)), (pool, split)      # t ascending on both routes
        assert np.array_equal(m_loader[0].mat, m_dense[0].mat) and m_dense[0].mat.sum() == len(ds)
    with pytest.raises(NotImplementedError):
        tp.forward_windows(np.zeros((4, 1024), np.float32), [0], [0], [3], 4)


def test_evaluate_main_dense_windows_on_frames(tmp_path, capsys, monkeypatch):
    from tennis_amd import engine
    from tennis_amd import evaluate as ev
    from tennis_amd.dataset import TennisSet
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    encoded = []
    call = engine.DenseNet121Features.__call__

    def counting(self, x, out=None):
        encoded.append(int(x.shape[0]))
        return call(self, x, out=out)
    monkeypatch.setattr(engine.DenseNet121Features, "__call__", counting)
    args = ["--root", root, "--frames_per_video", "9", "--data_shape", "224", "--window", "4", "--stride", "2", "--temp_pool", "gru",
            "--batch_size", "4", "--exp_root", exp]
    assert ev.main(args + ["--dense_windows"]) == 0
    out = capsys.readouterr().out
    ds = TennisSet(root=root, window=4, stride=2, frames_per_video=9, data_shape=224, split="test", balance=False)
    frames, _ = ds.window_table()
    finished = [ln for ln in out.splitlines() if ln.startswith("[Finished]")]
    assert len(finished) == 1 and "# Samples: %d," % len(ds) in finished[0]
    assert sum(encoded) == len(frames) and max(encoded) <= 4                     # every distinct frame once, in batches of 4
    assert len(frames) < len(ds) * 4                                             # (the loader route encodes window x the samples)
    # what is still refused, with the reason
    for bad, why in ((["--window", "1"], "--window W"), (["--temp_pool", "none"], "--temp_pool")):
        with pytest.raises(SystemExit, match=why):
            ev.main(args + ["--dense_windows"] + bad)
