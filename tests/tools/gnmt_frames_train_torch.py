"""ORACLE (test infrastructure only) - one frame-mode training step of the captioner on the CPU with torch autograd (float64), as
reference train_gnmt.py drives it without ``--feats_model`` (:148-203, 328-337):

  frames    the slots behind a clip's valid length set to zero, what ``btf.Pad()`` leaves there (utils/captioning.py:33)
  backbone  oracle/densenet_train_torch.py::forward over all batch x steps frames at once (TimeDistributed merges them,
            utils/layers.py:38-46; BatchNorm in training mode over all of them, the zero frames included), with an identity
            1024 x 1024 classifier and a zero bias so that its "logits" are the features, in frame order b * steps + t - as
            tests/tools/cnnrnn_train_torch.py uses it
  captioner oracle/gnmt_train_torch.py::forward_loss.  That function detaches its source (``torch.tensor(np.asarray(src))``), so
            ``forward_loss_src`` below restates it for a tensor source with the oracle's own cells and directions;
            tests/test_cpu_gnmt_frames.py pins the restatement to ``forward_loss``.

``frozen=True`` detaches the features (--freeze_backbone, train_gnmt.py:164-166): only the captioner gets gradients.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import densenet_train_torch as dt
from oracle import gnmt_train_torch as gt


def forward_loss_src(w, x, src_vl, tgt, tgt_vl, hidden, prefix="gnmt_", masks=None, cell="gru", num_layers=2, num_bi_layers=1,
                     use_residual=False):
    """``gnmt_train_torch.forward_loss`` on leaf tensors ``w`` and a source TENSOR x (B, T, F) that may carry a graph ->
    (loss scalar tensor, logits (B, L-1, V))."""
    dtype = x.dtype
    vl = torch.tensor(np.asarray(src_vl), dtype=torch.long)
    B, T, _ = x.shape
    H, NL, NBI = hidden, num_layers, num_bi_layers
    if masks is not None and not isinstance(masks, dict):
        assert NL == 2
        masks = {"enc": [masks[0], masks[1]], "dec": {1: masks[2]}}
    tt = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    pe = prefix + "enc_"
    inputs = x
    h_init, c_init = [], []
    for i in range(NL):
        if i < NBI:
            fo, _, _ = gt._direction(inputs, w, f"{pe}rnn{i}_l_", False, vl, cell)
            bo, bh, bc = gt._direction(inputs, w, f"{pe}rnn{i}_r_", True, vl, cell)
            out = torch.cat([fo, bo], dim=2)
            h_init.append(bh); c_init.append(bc)
        else:
            out, hh, cc = gt._direction(inputs, w, f"{pe}rnn{i}_", False, vl, cell)
            h_init.append(hh); c_init.append(cc)
        if masks is not None:
            out = out * tt(masks["enc"][i])
        if use_residual and i > NBI:
            out = out + inputs
        inputs = out
    mem = inputs
    keyproj = mem @ w[prefix + "dec_attention_key_weight"].T
    mask = (torch.arange(T)[None, :] < vl[:, None])
    tg = torch.tensor(np.asarray(tgt), dtype=torch.long)
    tvl = torch.tensor(np.asarray(tgt_vl), dtype=torch.long) - 1
    L = tg.shape[1] - 1
    hs, cs = list(h_init), list(c_init)
    att = torch.zeros((B, H), dtype=dtype)
    pd = prefix + "dec_"
    cw = lambda j: (w[f"{pd}rnn{j}_i2h_weight"], w[f"{pd}rnn{j}_h2h_weight"], w[f"{pd}rnn{j}_i2h_bias"], w[f"{pd}rnn{j}_h2h_bias"])
    logits = []
    for i in range(L):
        emb = w[prefix + "tgt_embed_weight"][tg[:, i].clamp(min=0)]
        hs[0], cs[0] = gt._cell(cell, torch.cat([emb, att], dim=1), hs[0], cs[0], *cw(0))
        q = hs[0] / np.sqrt(H)
        score = torch.einsum("bh,bth->bt", q, keyproj)
        score = torch.where(mask, score, torch.full_like(score, -1e18))
        wts = torch.softmax(score, dim=1) * mask.to(dtype)
        att = torch.einsum("bt,bth->bh", wts, mem)
        rnn_out = hs[0]
        for j in range(1, NL):
            cur = rnn_out
            hs[j], cs[j] = gt._cell(cell, torch.cat([cur, att], dim=1), hs[j], cs[j], *cw(j))
            rnn_out = hs[j]
            if masks is not None:
                rnn_out = rnn_out * tt(masks["dec"][j][i])
            if use_residual:
                rnn_out = rnn_out + cur
        logits.append(rnn_out @ w[prefix + "tgt_proj_weight"].T + w[prefix + "tgt_proj_bias"])
    logits = torch.stack(logits, dim=1)
    logp = torch.log_softmax(logits, dim=2)
    nll = -torch.gather(logp, 2, tg[:, 1:, None]).squeeze(2)
    m = (torch.arange(L)[None, :] < tvl[:, None]).to(dtype)
    loss = (nll * m).mean(dim=1).mean() * L / tvl.to(dtype).mean()
    return loss, logits


def _leaves(params, prefix):
    return {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in params.items() if k.startswith(prefix)}


def _grads(w):
    return {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in w.items()}


def captioner_loss_and_grads(params, src, src_vl, tgt, tgt_vl, hidden, prefix="gnmt_", **kw):
    """The captioner alone on fixed features src (B, T, F) -> (loss, logits, grads of its parameters, d loss / d src (B, T, F))"""
    w = _leaves(params, prefix)
    x = torch.tensor(np.asarray(src), dtype=torch.float64, requires_grad=True)
    loss, logits = forward_loss_src(w, x, src_vl, tgt, tgt_vl, hidden, prefix, **kw)
    loss.backward()
    return float(loss.detach()), logits.detach().numpy(), _grads(w), x.grad.numpy()


def loss_and_grads(params, frames_nchw, src_vl, tgt, tgt_vl, hidden, frozen=False, prefix="gnmt_", backbone_prefix="densenet0_", **kw):
    """frames_nchw (B, T, 3, S, S) -> (loss, logits (B, L-1, V), grads {name: array} of both parts (the captioner's only when
    frozen), batch statistics {bn: (mean, var)}, d loss / d src (B, T, F))"""
    x = np.array(frames_nchw, dtype=np.float64)
    B, T = x.shape[:2]
    for b in range(B):
        x[b, int(src_vl[b]):] = 0.0                      # Pad(): zeros of the normalised tensor
    bb = {k: v for k, v in params.items() if k.startswith(backbone_prefix)}
    eye = "_frames_identity_"
    bb[eye + "weight"] = np.eye(1024)
    bb[eye + "bias"] = np.zeros(1024)
    feats, wb, stats = dt.forward(bb, x.reshape((B * T,) + x.shape[2:]), backbone_prefix, eye)
    feats = feats.reshape(B, T, -1)
    src = feats.detach().clone().requires_grad_(True) if frozen else feats
    if not frozen:
        src.retain_grad()
    w = _leaves(params, prefix)
    loss, logits = forward_loss_src(w, src, src_vl, tgt, tgt_vl, hidden, prefix, **kw)
    loss.backward()
    g = _grads(w)
    if not frozen:
        g.update({k: v.grad.numpy() for k, v in wb.items() if v.requires_grad and not k.startswith(eye)})
    return float(loss.detach()), logits.detach().numpy(), g, stats, src.grad.numpy()
