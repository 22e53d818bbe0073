"""-m gpu: the five training handles against the device-free parameter table (tn_dbg_trainer_params, tests/test_cpu_trainer_params.py):
straight after create ``state_dict()`` is what was passed in, every flat row of the table is where the handle really keeps that
parameter (``params[offset : offset + count]`` is ``get(name)``), and after one step the same holds for the gradients.  Exact
comparisons: nothing here computes, it only moves floats.  Shapes as small as the handles take (64x64 frames, batch 2, 2 steps)."""
import numpy as np
import pytest
import torch

from tennis_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

SIDE, B, T, L, CLASSES = 64, 2, 2, 4, 11
GATES = {"gru": 3, "lstm": 4}


@pytest.fixture(scope="module")
def backbone():
    return W.make_densenet121_weights(0, fp16_model=False)


def head_weights(kind, F, H):
    p = W.make_rnn_weights(1, kind, F, H, f"cnnrnn0_{kind}0_")
    p.update(W.make_dense_weights(2, CLASSES, 2 * H, "cnnrnn0_dense0_"))
    return p


def head_table(kind, F, H):
    return _lib.trainer_params(_lib.TRAINER_HEAD, (GATES[kind], F, H, CLASSES), f"cnnrnn0_{kind}0_", "cnnrnn0_dense0_")


def gnmt_table(kind, F, H, E, V, layers=2, bi=1):
    return _lib.trainer_params(_lib.TRAINER_GNMT, (GATES[kind], F, H, E, V, layers, bi), "gnmt_")


def backbone_table(classes=0):
    return _lib.trainer_params(_lib.TRAINER_BACKBONE, (classes,), "densenet0_", "framemodel0_dense0_" if classes else None)


def caption_batch(rng, V):
    tgt = torch.from_numpy(rng.integers(4, V, (B, L)).astype(np.int32)).cuda()
    return torch.tensor([T, 1], dtype=torch.int32).cuda(), tgt, torch.tensor([L, L - 1], dtype=torch.int32).cuda()


def flat_of(a):
    """a parameter as the flat buffers keep it: convolution weights (O, I, kh, kw) in (O, kh, kw, I) order"""
    return (a.transpose(0, 2, 3, 1) if a.ndim == 4 else a).ravel()


def rows_match(tr, tables, buffers, gradient):
    """every flat row of each part's table against the part's flat buffer"""
    buffers = buffers if isinstance(buffers, tuple) else (buffers,)
    assert len(buffers) <= len(tables)
    for (rows, numel, _), buf in zip(tables[-len(buffers):], buffers):       # (a frozen backbone's gradients are left out)
        flat = buf.cpu().numpy()
        assert flat.shape == (numel,)
        for name, where, off, count in rows:
            if where == _lib.PARAM_FLAT:
                assert np.array_equal(flat[off:off + count], flat_of(tr.get(name, gradient=gradient))), (name, gradient)


def check(tr, params, tables, step):
    sd = tr.state_dict()
    assert set(sd) == set(params)
    for k, v in params.items():
        assert sd[k].shape == v.shape and np.array_equal(sd[k], v), k
    rows_match(tr, tables, tr.params, False)
    step()
    rows_match(tr, tables, tr.grads, True)
    g = tr.grads
    assert all(float(t.abs().max()) > 0 for t in (g if isinstance(g, tuple) else (g,)))     # a step did run


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_head(kind):
    from tennis_amd.engine import TemporalHeadTrainer
    p = head_weights(kind, 32, 16)
    tr = TemporalHeadTrainer(p, 32, 16, CLASSES, max_batch=B, max_steps=T, type=kind)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((B, T, 32)).astype(np.float32)).cuda()
    check(tr, p, [head_table(kind, 32, 16)], lambda: tr.forward_backward(x, torch.tensor([1, 5], dtype=torch.int32).cuda()))


@pytest.mark.parametrize("kind, layers", [("gru", 2), ("lstm", 3)])
def test_captioner(kind, layers):
    from tennis_amd.engine import GNMTTrainer
    p = W.make_gnmt_weights(0, kind, 16, 8, 6, 12, layers, 1)
    tr = GNMTTrainer(p, 16, 8, 6, 12, max_batch=B, max_src_len=T, max_tgt_len=L, cell_type=kind, num_layers=layers, num_bi_layers=1)
    rng = np.random.default_rng(4)
    src = torch.from_numpy(rng.standard_normal((B, T, 16)).astype(np.float32)).cuda()
    svl, tgt, tvl = caption_batch(rng, 12)
    check(tr, p, [gnmt_table(kind, 16, 8, 6, 12, layers, 1)], lambda: tr.forward_backward(src, svl, tgt, tvl))


def test_backbone(backbone):
    from tennis_amd.engine import FrameModelTrainer
    p = dict(backbone)
    p.update(W.make_dense_weights(1, CLASSES, 1024, "framemodel0_dense0_"))
    tr = FrameModelTrainer(p, SIDE, CLASSES, batch=B)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, SIDE, SIDE, 3)).astype(np.float32)).cuda()
    check(tr, p, [backbone_table(CLASSES)], lambda: tr.forward_backward(x, torch.tensor([1, 5], dtype=torch.int32).cuda()))


@pytest.mark.parametrize("frozen", [False, True], ids=["trainable", "frozen"])
def test_cnnrnn(backbone, frozen):
    from tennis_amd.engine import CNNRNNTrainer
    p = dict(backbone)
    p.update(head_weights("gru", 1024, 16))
    tr = CNNRNNTrainer(p, SIDE, CLASSES, batch=B, steps=T, freeze_backbone=frozen)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((B, T, SIDE, SIDE, 3)).astype(np.float32)).cuda()
    check(tr, p, [backbone_table(), head_table("gru", 1024, 16)],
          lambda: tr.forward_backward(x, torch.tensor([1, 5], dtype=torch.int32).cuda()))
    assert len(tr.grads) == (1 if frozen else 2) and len(tr.params) == 2


@pytest.mark.parametrize("frozen", [False, True], ids=["trainable", "frozen"])
def test_frames_captioner(backbone, frozen):
    from tennis_amd.engine import GNMTFramesTrainer
    p = dict(backbone)
    p.update(W.make_gnmt_weights(0, "gru", 1024, 8, 6, 12))
    tr = GNMTFramesTrainer(p, 8, 6, 12, size=SIDE, max_batch=B, max_src_len=T, max_tgt_len=L, max_frames=B * T, freeze_backbone=frozen)
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((B, T, SIDE, SIDE, 3)).astype(np.float32)).cuda()
    svl, tgt, tvl = caption_batch(rng, 12)
    check(tr, p, [backbone_table(), gnmt_table("gru", 1024, 8, 6, 12)], lambda: tr.forward_backward(x, svl, tgt, tvl))
    assert len(tr.grads) == (1 if frozen else 2) and len(tr.params) == 2
