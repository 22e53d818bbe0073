"""-m gpu: every instantiation of the recurrent training kernels - rnn.hip's forward kernel writing `save`, rnn_bptt.hip's
rnn_bptt_kernel reading it - against float64, for both cells.  The shapes come from
tests/tools/rnn_train_shapes.py, which tests/test_cpu_rnn_routes.py proves to reach every route of the dispatch policy
(csrc/rnn.h rnn_route): the three prefixes, no prefix, registers + LDS + stream, four rows per workgroup, with the 4-wide tail and the
16-wide streamed loop behind a prefix, near-full blocks and the padded rows of a last 4-row workgroup.

  * the temporal head's step (bidirectional, no valid_len) vs oracle/train_np.py, the comparison and bars of
    test_gpu_train.py::test_gradients_and_sgd_step: loss and logits 1e-4, every gradient 2e-4 of the parameter's max|g|;
  * the captioner's step (valid_len, final-state gradients dh_last / dc_last; one row at the full length and one of valid length 1,
    whose only step carries the final-state gradient) vs oracle/gnmt_train_torch.py, the comparison and bars of
    test_gpu_gnmt_train.py::test_loss_and_gradients_match_autograd: loss and logits 1e-4, every gradient 2e-3 of max|g|.

Each case's worst errors go to the report, keyed by cell, route and shape."""
import numpy as np
import pytest
import torch

from oracle import gnmt_train_torch as gt
from oracle import train_np as tn
from test_gpu_gnmt_train import _case
from test_gpu_train import _setup
from tools import rnn_train_shapes as RS

pytestmark = pytest.mark.gpu

HEAD_BAR, HEAD_GRAD_BAR = 1e-4, 2e-4
GNMT_BAR, GNMT_GRAD_BAR = 1e-4, 2e-3


def _lib():
    from tennis_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("cell,B,T,F,H", RS.head_cases())
def test_head_step_on_every_route(report, cell, B, T, F, H):
    from tennis_amd.engine import TemporalHeadTrainer
    C_ = 11
    route = RS.route_name(_lib(), cell, B, H, 2)
    p, x, y = _setup(4, B, T, F, H, C_, cell)
    tr = TemporalHeadTrainer(p, F, H, C_, max_batch=B, max_steps=T, type=cell)
    loss, logits = tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    rl, rlg, rg = tn.forward_backward(x, y, p, cell=cell)
    fwd = max(np.abs(loss.cpu().numpy() - rl).max(), np.abs(logits.cpu().numpy() - rlg).max())
    errs = {k: np.abs(tr.get(k, gradient=True).reshape(g.shape) - g).max() / max(1e-6, np.abs(g).max()) for k, g in rg.items()}
    worst = max(errs, key=errs.get)
    key = f"rnn_route_head_{cell}_{route}_B{B}_T{T}_F{F}_H{H}"
    report[key + "_fwd_abs_err"] = float(fwd)
    report[key + "_grad_rel_err"] = float(errs[worst])
    print(f"{key}: loss/logits {fwd:.3e} grad {errs[worst]:.3e} ({worst})")
    assert fwd < HEAD_BAR, (key, fwd)
    for k, e in errs.items():
        assert e < HEAD_GRAD_BAR, (key, k, e)


@pytest.mark.parametrize("cfg", RS.gnmt_cases(), ids=lambda c: f"{c['cell']}-B{c['B']}-T{c['T']}-H{c['H']}-nbi{c['nbi']}")
def test_captioner_step_on_every_route(report, cfg):
    from tennis_amd.engine import GNMTTrainer
    cell, B, T, H, L, nl, nbi = (cfg[k] for k in ("cell", "B", "T", "H", "L", "nl", "nbi"))
    routes = "+".join(RS.route_name(_lib(), cell, B, H, d) for d in RS.gnmt_layer_dirs(cfg))
    p, src, svl, tgt, tvl = _case(**cfg)
    svl[1] = 1                              # row 0 runs the full length, row 1 one step: its final-state gradient enters at s = 0
    assert svl[0] == T and svl.min() >= 1 and svl.max() <= T
    tr = GNMTTrainer(p, cfg["F"], H, cfg["E"], cfg["V"], max_batch=B, max_src_len=T, max_tgt_len=L, cell_type=cell, num_layers=nl,
                     num_bi_layers=nbi)
    loss, logits = tr.forward_backward(torch.from_numpy(src).cuda(), torch.from_numpy(svl).cuda(), torch.from_numpy(tgt).cuda(),
                                       torch.from_numpy(tvl).cuda(), return_logits=True)
    rl, rlog, rg = gt.loss_and_grads(p, src, svl, tgt, tvl, H, cell=cell, num_layers=nl, num_bi_layers=nbi)
    assert np.isfinite(rl) and all(np.isfinite(g).all() for g in rg.values())
    eloss = abs(float(loss) - rl) / max(1.0, abs(rl))
    elog = np.abs(logits.cpu().numpy() - rlog).max()
    errs = {k: np.abs(tr.get(k, gradient=True) - g).max() / max(1e-7, np.abs(g).max()) for k, g in rg.items()}
    worst = max(errs, key=errs.get)
    key = f"rnn_route_gnmt_{cell}_{routes}_B{B}_T{T}_H{H}_nbi{nbi}"
    report[key + "_fwd_abs_err"] = float(max(eloss, elog))
    report[key + "_grad_rel_err"] = float(errs[worst])
    print(f"{key}: loss {eloss:.3e} logits {elog:.3e} grad {errs[worst]:.3e} ({worst}, max|g| {np.abs(rg[worst]).max():.3e})")
    assert eloss < GNMT_BAR, (key, float(loss), rl)
    assert elog < GNMT_BAR, (key, elog)
    for k, e in errs.items():
        assert e < GNMT_GRAD_BAR, (key, k, e, np.abs(rg[k]).max())
