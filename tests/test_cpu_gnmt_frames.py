"""No GPU: the float64 oracle tool of the frame-mode captioner step pinned to oracle/gnmt_train_torch.py, the caption dataset's frame
source and its batching, and train_gnmt's frame-mode assembly."""
import os

import numpy as np
import pytest

from oracle import gnmt_train_torch as gt
from tools import gnmt_frames_train_torch as ft
from tools import tiny_dataset


def _case(seed, B, T, F, H, E, V, L, cell, nl, nbi):
    from tennis_amd import weights as W
    p = W.make_gnmt_weights(seed, cell, F, H, E, V, num_layers=nl, num_bi_layers=nbi)
    rng = np.random.default_rng(seed)
    p["gnmt_tgt_embed_weight"] = rng.normal(0, 0.5, (V, E)).astype(np.float32)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    svl = rng.integers(max(1, T // 2), T, B).astype(np.int32)
    svl[0] = T
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0] = 2
    tvl = rng.integers(3, L + 1, B).astype(np.int32)
    tvl[0] = L
    for b in range(B):
        tgt[b, tvl[b] - 1] = 3
        tgt[b, tvl[b]:] = 1
    return p, src, svl, tgt, tvl


@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("nl,nbi,res", [(2, 1, False), (3, 1, True)])
def test_oracle_tool_restates_forward_loss(cell, nl, nbi, res):
    """on detached random features the tool's forward for a tensor source gives forward_loss's loss, logits and parameter gradients;
    its source gradient is 0 at and past the valid length and agrees with a finite difference"""
    B, T, F, H, E, V, L = 3, 7, 10, 8, 6, 14, 6
    p, src, svl, tgt, tvl = _case(31 + nl, B, T, F, H, E, V, L, cell, nl, nbi)
    rng = np.random.default_rng(3)
    masks = {"enc": [(rng.random((B, T, (2 if i < nbi else 1) * H)) > 0.25) / 0.75 for i in range(nl)],
             "dec": {j: (rng.random((L - 1, B, H)) > 0.25) / 0.75 for j in range(1, nl)}}
    for m in (None, masks):
        kw = dict(cell=cell, masks=m, num_layers=nl, num_bi_layers=nbi, use_residual=res)
        rl, rlog, rg = gt.loss_and_grads(p, src, svl, tgt, tvl, H, **kw)
        loss, logits, g, dsrc = ft.captioner_loss_and_grads(p, src, svl, tgt, tvl, H, **kw)
        assert abs(loss - rl) < 1e-10 and np.abs(logits - rlog).max() < 1e-10
        assert set(g) == set(rg)
        for k in rg:
            assert np.abs(g[k] - rg[k]).max() < 1e-10, k
        for b in range(B):
            assert np.all(dsrc[b, int(svl[b]):] == 0.0) and np.abs(dsrc[b, :int(svl[b])]).max() > 0
        d = rng.normal(0, 1, src.shape)
        eps = 1e-5
        lp = gt.loss_and_grads(p, src.astype(np.float64) + eps * d, svl, tgt, tvl, H, **kw)[0]
        lm = gt.loss_and_grads(p, src.astype(np.float64) - eps * d, svl, tgt, tvl, H, **kw)[0]
        assert abs((lp - lm) / (2 * eps) - float((dsrc * d).sum())) < 1e-6 * max(1.0, abs(float((dsrc * d).sum())))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tiny") / "data")
    info = tiny_dataset.write(root, np.random.default_rng(0), frames_per_point=5)
    return root, info


def test_caption_frame_source_on_disk(tiny):
    from tennis_amd.captions import CaptionSet, bucketed_batches, pad_batchify
    from tennis_amd.dataset import TennisSet
    root, info = tiny
    ds = TennisSet(root=root, captions=True, split="train", every=1)                 # no feats_model: the frames are the source
    assert isinstance(ds, CaptionSet) and len(ds) == len(info["points"]["train"])
    imgs, cap, n, lc = ds[0]
    assert imgs.shape == (5, 3, 48, 64) and imgs.dtype == np.float32 and n == 5 and lc == len(cap)      # default transform: per frame
    assert not np.array_equal(imgs[0], imgs[1])
    pid, vid, start, end, _ = info["points"]["train"][0]
    ts = TennisSet(root=root, split="train", balance=False)
    assert np.array_equal(imgs[2], ts._load(vid, start + 2))                          # TennisSet's frame reading and transform
    for every, want in ((2, 3), (3, 2)):
        d2 = TennisSet(root=root, captions=True, split="train", every=every, vocab=ds.vocab)
        it = d2[1]
        assert it[0].shape == (want, 3, 48, 64) and it[2] == want
        assert np.array_equal(it[0][1], ds[1][0][every])
        assert d2.get_clip_lens() == [want] * len(d2)
    for d in (ds, TennisSet(root=root, captions=True, split="val", every=2, vocab=ds.vocab, inference=True)):
        lens, clips = d.get_data_lens(), d.get_clip_lens()
        for i in range(len(d)):
            item = d[i]
            assert clips[i] == item[0].shape[0] == item[2] and lens[i][1] == len(item[1]) == item[3]
            assert abs(lens[i][0] - clips[i]) <= 1                                    # the reference's rounding (dataset.py:235-247)
    assert len(d[0]) == 5 and d[0][4] == 0                                            # inference: the instance id travels along
    # Pad() on 4-D items: exactly as on (T, F) items
    a, b = ds[0], TennisSet(root=root, captions=True, split="train", every=2, vocab=ds.vocab)[1]
    src, tgt, svl, tvl = pad_batchify([a, b])
    assert src.shape == (2, 5, 3, 48, 64) and src.dtype == np.float32 and list(svl) == [5, 3]
    assert np.array_equal(src[0], a[0]) and np.array_equal(src[1, :3], b[0]) and np.all(src[1, 3:] == 0.0)
    assert tgt.shape == (2, max(len(a[1]), len(b[1]))) and list(tvl) == [len(a[1]), len(b[1])]
    fa, fb = np.ones((4, 7), np.float32), np.ones((2, 7), np.float32)
    fsrc = pad_batchify([(fa, a[1], 4, len(a[1])), (fb, b[1], 2, len(b[1]))])[0]
    assert fsrc.shape == (2, 4, 7) and fsrc.dtype == np.float32 and np.all(fsrc[1, 2:] == 0.0)
    assert sum(bt[0].shape[0] for bt in bucketed_batches(ds, 2)) == len(ds)
    # a device-batched transform is not run per frame: the item is the decoded clip
    class Batched:
        device_batched = True
    du = CaptionSet(root=root, split="train", frames=True, transform=Batched())
    with pytest.raises(ValueError, match="frames=True"):
        CaptionSet(root=root, split="train")                                          # built directly: features or frames must be asked for
    assert du[0][0].shape == (5, 48, 64, 3) and du[0][0].dtype == np.uint8
    u = pad_batchify([du[0], TennisSet(root=root, captions=True, split="train", every=2, transform=Batched())[1]])[0]
    assert u.dtype == np.uint8 and u.shape == (2, 5, 48, 64, 3) and np.all(u[1, 3:] == 0)


def test_caption_frame_source_synthetic():
    from tennis_amd.captions import CaptionSet
    ds = CaptionSet(root=None, frames=True, data_shape=32, n_points=3, mean_frames=6)
    imgs, cap, n, lc = ds[0]
    assert imgs.shape == (n, 3, 32, 32) and imgs.dtype == np.float32 and n == ds.get_clip_lens()[0]
    flat = imgs.reshape(n, -1)
    assert len({f.tobytes() for f in flat}) == n                                      # distinct per (video, frame)
    assert np.array_equal(ds[0][0], imgs) and not np.array_equal(ds[1][0][0], imgs[0])
    feats = CaptionSet(root=None, n_points=3, mean_frames=6)[0][0]                    # the feature source is what it was
    assert feats.ndim == 2 and feats.shape[1] == 1024


def test_train_gnmt_frame_mode_assembly(tiny, tmp_path, monkeypatch):
    from tennis_amd import train_gnmt as tg
    from tennis_amd.utils.layers import TimeDistributed
    root, info = tiny
    base = ["--data_root", root, "--data_shape", "32", "--num_hidden", "8", "--emb_size", "6", "--emb_file", "", "--every", "2"]
    assert tg.build_parser().parse_args([]).data_shape == 512 and not tg.build_parser().parse_args([]).freeze_backbone
    flags = tg.build_parser().parse_args(base)
    data_train, data_val, data_test, model, translator = tg.build(flags)
    assert isinstance(model.src_embed, TimeDistributed) and model._input_size == 1024
    assert any(k.startswith("densenet0_") for k in model.collect_params()) and "gnmt_enc_rnn0_l_i2h_weight" in model.collect_params()
    assert model.collect_params()["gnmt_enc_rnn0_l_i2h_weight"].data.shape == (3 * 8, 1024)
    assert any(k.startswith("src_embed.model.") for k in model._structural_params())
    assert data_train._transform.train and not data_val._transform.train and not data_test._transform.train
    assert data_train._transform.crop == 32 and data_val._transform.crop == 32 and data_val._transform.resize == 64
    item = data_train[0]
    assert item[0].dtype == np.uint8 and item[0].shape == (3, 48, 64, 3)                # decoded clips; the transform runs per batch
    assert tg.frame_capacity(data_train, 2, 5) == 6
    flags = tg.build_parser().parse_args(base + ["--no_augment"])
    assert not tg.build(flags)[0]._transform.train
    # --backbone_from_id: the experiment folder must exist (reference train_gnmt.py:161-162)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="0006"):
        tg.build(tg.build_parser().parse_args(base + ["--backbone_from_id", "0006"]))
    os.makedirs(os.path.join("models", "vision", "experiments", "0006"))
    assert tg.build(tg.build_parser().parse_args(base + ["--backbone_from_id", "0006"]))[3].src_embed is not None   # empty: nothing loaded
    # feature mode is what it was: no CNN in the model, the features' width is the input size
    flags = tg.build_parser().parse_args(["--feats_model", "0006", "--feature_dim", "48", "--num_hidden", "8", "--emb_size", "6", "--n_points", "4"])
    dt, dv, _, fm, _ = tg.build(flags)
    assert fm.src_embed is None and fm._input_size == 48 and dt[0][0].shape[1] == 48 and not any(k.startswith("densenet0_") for k in fm.collect_params())
    flags = tg.build_parser().parse_args(["--feature_dim", "48", "--num_hidden", "8", "--emb_size", "6", "--n_points", "4"])
    assert tg.build(flags)[3].src_embed is None                                         # synthetic without --frames: features
