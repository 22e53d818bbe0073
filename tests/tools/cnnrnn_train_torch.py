"""ORACLE (test infrastructure only) - one end-to-end training step of ``CNNRNN(FrameModel(DenseNet121.features))`` over
``TimeDistributed`` frames on the CPU with torch autograd (float64), as reference train.py:197-236 drives it with
``--window > 1 --temp_pool gru|lstm`` and no ``--feats_model``:

  backbone  oracle/densenet_train_torch.py::forward over all batch x steps frames at once (TimeDistributed merges them,
            utils/layers.py:38-46; BatchNorm in training mode over all of them), with an identity 1024 x 1024 classifier and a
            zero bias, so that its "logits" are the features, in frame order b * steps + t
  head      bi-GRU / bi-LSTM (MXNet gate order: GRU [r, z, n], LSTM [i, f, g, o]) -> max over T (first maximum) -> Dense
            (definitions.py:93-109)
  loss      SoftmaxCrossEntropyLoss per sample, backward of their SUM (train.py:324,419-421)

``frozen=True`` detaches the features (--freeze_backbone, train.py:231-233): only the head gets gradients.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import densenet_train_torch as dt


def _cell_dir(x, wi, wh, bi, bh, cell, reverse):
    """one direction over x (B, T, F) -> (B, T, H)"""
    B, T, _ = x.shape
    H = wh.shape[1]
    h = x.new_zeros((B, H))
    c = x.new_zeros((B, H))
    out = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gi = x[:, t] @ wi.T + bi
        gh = h @ wh.T + bh
        if cell == "gru":
            r = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (1 - z) * n + z * h
        else:
            a = gi + gh
            i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
        out[t] = h
    return torch.stack(out, 1)


def head_forward(feats, w, cell, rnn_prefix, dense_prefix):
    """feats (B, T, F) tensor, w: dict of leaf tensors -> logits (B, C)"""
    seqs = [_cell_dir(feats, w[rnn_prefix + d + "i2h_weight"], w[rnn_prefix + d + "h2h_weight"], w[rnn_prefix + d + "i2h_bias"],
                      w[rnn_prefix + d + "h2h_bias"], cell, rev) for d, rev in (("l0_", False), ("r0_", True))]
    seq = torch.cat(seqs, 2)                                    # (B, T, 2H)
    arg = torch.argmax(seq.detach(), dim=1, keepdim=True)       # first maximum (MXNet max's gradient goes to one element)
    pooled = torch.gather(seq, 1, arg)[:, 0]
    return pooled @ w[dense_prefix + "weight"].T + w[dense_prefix + "bias"]


def head_loss_and_grads(feats, labels, params, cell="gru", rnn_prefix=None, dense_prefix="cnnrnn0_dense0_"):
    """The head alone on fixed features (B, T, F) -> (loss, logits, grads of the head's parameters, dfeats (B, T, F))"""
    rnn_prefix = rnn_prefix or f"cnnrnn0_{cell}0_"
    w = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in params.items()
         if k.startswith((rnn_prefix, dense_prefix))}
    x = torch.tensor(np.asarray(feats), dtype=torch.float64, requires_grad=True)
    logits = head_forward(x, w, cell, rnn_prefix, dense_prefix)
    loss = F.cross_entropy(logits, torch.tensor(np.asarray(labels), dtype=torch.long), reduction="none")
    loss.sum().backward()
    return (loss.detach().numpy(), logits.detach().numpy(), {k: v.grad.numpy() for k, v in w.items()}, x.grad.numpy())


def loss_and_grads(params, x_nchw, labels, steps, cell="gru", frozen=False, prefix="densenet0_", rnn_prefix=None,
                   dense_prefix="cnnrnn0_dense0_"):
    """x_nchw (batch * steps, 3, S, S) in frame order b * steps + t, labels (batch,) ->
    (loss (batch,), logits (batch, C), grads {name: array} (the head's only when frozen), batch statistics {bn: (mean, var)})"""
    rnn_prefix = rnn_prefix or f"cnnrnn0_{cell}0_"
    bb = {k: v for k, v in params.items() if k.startswith(prefix)}
    eye = "_cnnrnn_identity_"
    bb[eye + "weight"] = np.eye(1024)
    bb[eye + "bias"] = np.zeros(1024)
    feats, wb, stats = dt.forward(bb, x_nchw, prefix, eye)
    n = feats.shape[0]
    feats = feats.reshape(n // steps, steps, -1)
    if frozen:
        feats = feats.detach()
    w = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in params.items()
         if k.startswith((rnn_prefix, dense_prefix))}
    logits = head_forward(feats, w, cell, rnn_prefix, dense_prefix)
    loss = F.cross_entropy(logits, torch.tensor(np.asarray(labels), dtype=torch.long), reduction="none")
    loss.sum().backward()
    g = {k: v.grad.numpy() for k, v in w.items()}
    if not frozen:
        g.update({k: v.grad.numpy() for k, v in wb.items() if v.requires_grad and not k.startswith(eye)})
    return loss.detach().numpy(), logits.detach().numpy(), g, stats
