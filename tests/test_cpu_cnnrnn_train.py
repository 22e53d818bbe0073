"""-m "not gpu": the end-to-end CNN-RNN training route - the float64 oracle of its step (tests/tools/cnnrnn_train_torch.py)
against oracle/train_np.py and finite differences, the driver's routing, and the all-reduce of a trainer with several
gradient buffers on gloo."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import train_np as tn
from tools import cnnrnn_train_torch as ct


def _head_params(cell, F, H, C, seed=3):
    rng = np.random.default_rng(seed)
    G = 3 if cell == "gru" else 4
    pre = f"cnnrnn0_{cell}0_"
    p = {}
    for d in ("l0_", "r0_"):
        p[pre + d + "i2h_weight"] = rng.normal(0, 0.3, (G * H, F))
        p[pre + d + "h2h_weight"] = rng.normal(0, 0.3, (G * H, H))
        p[pre + d + "i2h_bias"] = rng.normal(0, 0.1, G * H)
        p[pre + d + "h2h_bias"] = rng.normal(0, 0.1, G * H)
    p["cnnrnn0_dense0_weight"] = rng.normal(0, 0.3, (C, 2 * H))
    p["cnnrnn0_dense0_bias"] = rng.normal(0, 0.1, C)
    return p


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_oracle_head_matches_train_np(cell):
    """on fixed features the torch restatement of the head equals oracle/train_np's loss, logits and every head gradient"""
    B, T, F, H, C = 3, 5, 12, 8, 4
    p = _head_params(cell, F, H, C)
    x = np.random.default_rng(7).normal(0, 1, (B, T, F))
    y = np.array([0, 3, 1], np.int32)
    loss, logits, g, _ = ct.head_loss_and_grads(x, y, p, cell)
    rl, rlog, rg = tn.forward_backward(x, y, p, cell=cell)
    assert np.abs(loss - rl).max() < 1e-10 and np.abs(logits - rlog).max() < 1e-10
    assert set(g) == set(rg)
    for k in rg:
        assert np.abs(g[k] - rg[k]).max() < 1e-10 * max(1.0, np.abs(rg[k]).max()), k


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_oracle_input_gradient_matches_finite_differences(cell):
    """the gradient with respect to the features - what the step hands to the backbone - against central differences of
    train_np's summed loss"""
    B, T, F, H, C = 2, 4, 6, 4, 3
    p = _head_params(cell, F, H, C, seed=11)
    x = np.random.default_rng(5).normal(0, 1, (B, T, F))
    y = np.array([2, 0], np.int32)
    _, _, _, dx = ct.head_loss_and_grads(x, y, p, cell)
    eps = 1e-6
    fd = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += eps
        xm[idx] -= eps
        fd[idx] = (tn.forward_backward(xp, y, p, cell=cell)[0].sum() - tn.forward_backward(xm, y, p, cell=cell)[0].sum()) / (2 * eps)
    assert np.abs(dx - fd).max() < 1e-7 * max(1.0, np.abs(fd).max()), np.abs(dx - fd).max()


def _flags(*args):
    from tennis_amd.train import build_parser
    return build_parser().parse_args(list(args))


@pytest.mark.parametrize("extra", [[], ["--freeze_backbone"]])
@pytest.mark.parametrize("pool", ["gru", "lstm"])
def test_route_accepts_cnnrnn_on_frames(pool, extra):
    from tennis_amd.train import check_frames_route
    check_frames_route(_flags("--window", "4", "--temp_pool", pool, *extra))          # no exit
    check_frames_route(_flags("--window", "1"))                                       # the frame classifier, as before
    check_frames_route(_flags("--window", "4", "--temp_pool", pool, "--feats_model", "0001", *extra))


@pytest.mark.parametrize("args", [["--window", "4", "--temp_pool", "mean"], ["--window", "4", "--temp_pool", "max"],
                                  ["--window", "4"], ["--window", "1", "--freeze_backbone"], ["--window", "0"]])
def test_route_refuses_the_other_combinations(args):
    from tennis_amd.train import check_frames_route
    with pytest.raises(SystemExit) as e:
        check_frames_route(_flags(*args))
    assert isinstance(e.value.code, str) and e.value.code      # a message, not a bare status


def test_main_refuses_mean_pool_on_frames_before_any_work(tmp_path):
    from tennis_amd import train as tr
    with pytest.raises(SystemExit, match="temp_pool gru"):
        tr.main(["--root", str(tmp_path / "data"), "--window", "4", "--temp_pool", "max", "--exp_root", str(tmp_path / "exp")])


def test_help_says_the_ragged_batch_is_dropped():
    from tennis_amd.train import build_parser
    assert "drops a ragged last batch" in " ".join(build_parser().format_help().split())


class _TwoBufferTrainer:
    """the surface allreduce_and_step uses: grads as a tuple of flat buffers, step(batch_size, lr, momentum, wd)"""

    def __init__(self, rank):
        self.bb = torch.arange(6, dtype=torch.float32) + 10 * rank
        self.head = torch.full((3,), 1.0 + rank)
        self.steps = []

    @property
    def grads(self):
        return self.bb, self.head

    def step(self, batch_size, lr, momentum, wd):
        self.steps.append((batch_size, lr, momentum, wd))


def _allreduce_worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tennis_amd.train import allreduce_and_step
    t = _TwoBufferTrainer(rank)
    allreduce_and_step(t, 16, 0.01, 0.9, 1e-4)
    ret[rank] = (t.bb.numpy().copy(), t.head.numpy().copy(), list(t.steps))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_and_step_sums_every_buffer_world2():
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_allreduce_worker, args=(2, 29547, ret), nprocs=2, join=True)
        for r in range(2):
            bb, head, steps = ret[r]
            assert np.array_equal(bb, 2 * np.arange(6, dtype=np.float32) + 10)
            assert np.array_equal(head, np.full(3, 3.0, np.float32))
            assert steps == [(16, 0.01, 0.9, 1e-4)]
