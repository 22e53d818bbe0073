"""-m gpu: the wide recurrent kernels - rnn.hip's rnn_recurrent_wide_kernel, rnn_bptt.hip's rnn_bptt_wide_kernel: two gate rows per
thread, 1024 < gates*H <= 2048 (LSTM up to H = 512, GRU up to H = 680) - against float64, for both cells.  The shapes come from
tests/tools/rnn_wide_shapes.py, which tests/test_cpu_rnn_wide_routes.py proves to reach every path of the kernels (rows per workgroup
1 | 4, a full or a ragged second row, with and without the 4-wide tail).

  * forward: BiRNN with and without valid_length (one row of valid length 1) vs oracle/rnn_np.py: seq, h_last, c_last < 1e-4, the bar of
    test_gpu_kernels.py::test_birnn;
  * the temporal head's step vs oracle/train_np.py, the comparison and bars of test_gpu_rnn_train_routes.py: loss / logits 1e-4, every
    gradient 2e-4 of its max|g| - at seeds whose oracle shows no near tie in the max over T (one flipped argmax is 3e-3 of max|g|);
  * the captioner's step (valid_len, final-state gradients, a row of valid length 1) vs oracle/gnmt_train_torch.py: 1e-4, gradients 2e-3
    of max|g| with the 1e-7 floor;
  * inference: encode + beam search vs oracle/gnmt_np.py: mem and scores 1e-4, ids and lengths equal - at cases whose oracle ids are
    shown, in the test, not to move under a 1e-5 relative perturbation of the source (no near tie can pass as a kernel error);
  * bit identity: under tn_dbg_rnn_force_wide the narrow shapes run the wide kernels and give the bits of the default routes - outputs,
    final states, gradients and updated parameters.  One accumulator per gate row over ascending k in every kernel: no tolerance;
  * what stays refused: gates*H > 2048, and the windowed head past 1024.

Each case's worst errors go to the report, keyed by cell, path and shape."""
import numpy as np
import pytest
import torch

from oracle import gnmt_np as gn
from oracle import gnmt_train_torch as gt
from oracle import rnn_np as rn
from oracle import train_np as tn
from test_gpu_gnmt_train import _case as _gnmt_case
from test_gpu_train import _setup
from tools import rnn_wide_shapes as WS

pytestmark = pytest.mark.gpu

FWD_BAR = 1e-4
HEAD_BAR, HEAD_GRAD_BAR = 1e-4, 2e-4
GNMT_BAR, GNMT_GRAD_BAR = 1e-4, 2e-3


def _lib():
    from tennis_amd import _lib as L
    return L.load()


def _cuda(a):
    return torch.from_numpy(a).cuda()


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def _birnn_inputs(cell, B, T, F, H, use_vl, seed=3):
    from tennis_amd import weights as W
    p = W.make_rnn_weights(seed, cell, F, H, "rnn_")
    rng = np.random.default_rng(7)
    x = rng.normal(0, 1, (B, T, F)).astype(np.float32)
    vl = None
    if use_vl:
        vl = rng.integers(1, T + 1, B).astype(np.int32)
        vl[0], vl[1] = T, 1                      # the full length, and a row whose only step is also its last
    return p, x, vl


def _birnn_run(cell, B, T, F, H, dirs, p, x, vl):
    from tennis_amd.engine import BiRNN
    net = BiRNN(cell, F, H, p, "rnn_", dirs == 2, max_rows=B * T)
    seq, hl, cl = net(_cuda(x), None if vl is None else _cuda(vl), True)
    return seq.cpu().numpy(), hl.cpu().numpy(), cl.cpu().numpy() if cell == "lstm" else None


@pytest.mark.parametrize("use_vl", [False, True], ids=["full", "vl"])
@pytest.mark.parametrize("cell,B,T,F,H,dirs", WS.cases())
def test_forward_matches_the_oracle(report, cell, B, T, F, H, dirs, use_vl):
    route = WS.route_name(_lib(), cell, B, H, dirs)
    p, x, vl = _birnn_inputs(cell, B, T, F, H, use_vl)
    seq, hl, cl = _birnn_run(cell, B, T, F, H, dirs, p, x, vl)
    if dirs == 2:
        ref, (fh, fc), (bh, bc) = rn.birnn_layer(x, p, "rnn_", cell, vl)
        rh, rc = np.stack([fh, bh]), (np.stack([fc, bc]) if cell == "lstm" else None)
    else:
        ref, fh, fc = rn.rnn_direction(x, p, "rnn_l0_", cell, False, vl)
        rh, rc = fh[None], (fc[None] if cell == "lstm" else None)
    assert seq.shape == ref.shape and hl.shape == rh.shape
    err, errh = np.abs(seq - ref).max(), np.abs(hl - rh).max()
    errc = np.abs(cl - rc).max() if cell == "lstm" else 0.0
    key = f"rnn_wide_fwd_{cell}_{route}_B{B}_T{T}_F{F}_H{H}_d{dirs}_{'vl' if use_vl else 'full'}"
    report[key + "_abs_err"] = float(max(err, errh, errc))
    print(f"{key}: seq {err:.3e} h_last {errh:.3e} c_last {errc:.3e}")
    assert err < FWD_BAR and errh < FWD_BAR and errc < FWD_BAR, (key, err, errh, errc)
    if use_vl:                                   # steps at or past a row's valid length emit zeros
        for b in range(B):
            assert not seq[b, vl[b]:].any()


# ---- training steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,B,T,F,H", WS.head_cases())
def test_head_step_matches_the_oracle(report, cell, B, T, F, H):
    from tennis_amd.engine import TemporalHeadTrainer
    C_ = 11
    route = WS.route_name(_lib(), cell, B, H, 2)
    p, x, y = _setup(WS.head_seed(cell, B, H), B, T, F, H, C_, cell)
    # the case is no near tie of the max over T (tools/rnn_wide_shapes.py HEAD_MIN_GAP): shown on the oracle, before anything is compared
    top2 = np.sort(rn.birnn_layer(x, p, f"cnnrnn0_{cell}0_", cell)[0].astype(np.float64), axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() >= WS.HEAD_MIN_GAP, (cell, B, H, (top2[:, 1] - top2[:, 0]).min())
    tr = TemporalHeadTrainer(p, F, H, C_, max_batch=B, max_steps=T, type=cell)
    loss, logits = tr.forward_backward(_cuda(x), _cuda(y))
    rl, rlg, rg = tn.forward_backward(x, y, p, cell=cell)
    fwd = max(np.abs(loss.cpu().numpy() - rl).max(), np.abs(logits.cpu().numpy() - rlg).max())
    errs = {k: np.abs(tr.get(k, gradient=True).reshape(g.shape) - g).max() / max(1e-6, np.abs(g).max()) for k, g in rg.items()}
    worst = max(errs, key=errs.get)
    key = f"rnn_wide_head_{cell}_{route}_B{B}_T{T}_F{F}_H{H}"
    report[key + "_fwd_abs_err"] = float(fwd)
    report[key + "_grad_rel_err"] = float(errs[worst])
    print(f"{key}: loss/logits {fwd:.3e} grad {errs[worst]:.3e} ({worst})")
    assert fwd < HEAD_BAR, (key, fwd)
    for k, e in errs.items():
        assert e < HEAD_GRAD_BAR, (key, k, e)


def _gnmt_trainer(cfg, p):
    from tennis_amd.engine import GNMTTrainer
    return GNMTTrainer(p, cfg["F"], cfg["H"], cfg["E"], cfg["V"], max_batch=cfg["B"], max_src_len=cfg["T"], max_tgt_len=cfg["L"],
                       cell_type=cfg["cell"], num_layers=cfg["nl"], num_bi_layers=cfg["nbi"])


@pytest.mark.parametrize("cfg", WS.GNMT_CASES, ids=lambda c: f"{c['cell']}-T{c['T']}-H{c['H']}-nl{c['nl']}")
def test_captioner_step_matches_the_oracle(report, cfg):
    cell, B, T, H, nl, nbi = (cfg[k] for k in ("cell", "B", "T", "H", "nl", "nbi"))
    p, src, svl, tgt, tvl = _gnmt_case(**cfg)
    svl[1] = 1                              # row 0 runs the full length, row 1 one step: its final-state gradient enters at s = 0
    assert svl[0] == T and svl.min() >= 1 and svl.max() <= T
    tr = _gnmt_trainer(cfg, p)
    loss, logits = tr.forward_backward(_cuda(src), _cuda(svl), _cuda(tgt), _cuda(tvl), return_logits=True)
    rl, rlog, rg = gt.loss_and_grads(p, src, svl, tgt, tvl, H, cell=cell, num_layers=nl, num_bi_layers=nbi)
    assert np.isfinite(rl) and all(np.isfinite(g).all() for g in rg.values())
    eloss = abs(float(loss) - rl) / max(1.0, abs(rl))
    elog = np.abs(logits.cpu().numpy() - rlog).max()
    errs = {k: np.abs(tr.get(k, gradient=True) - g).max() / max(1e-7, np.abs(g).max()) for k, g in rg.items()}
    worst = max(errs, key=errs.get)
    key = f"rnn_wide_gnmt_{cell}_B{B}_T{T}_H{H}_nl{nl}_nbi{nbi}"
    report[key + "_fwd_abs_err"] = float(max(eloss, elog))
    report[key + "_grad_rel_err"] = float(errs[worst])
    print(f"{key}: loss {eloss:.3e} logits {elog:.3e} grad {errs[worst]:.3e} ({worst}, max|g| {np.abs(rg[worst]).max():.3e})")
    assert eloss < GNMT_BAR, (key, float(loss), rl)
    assert elog < GNMT_BAR, (key, elog)
    for k, e in errs.items():
        assert e < GNMT_GRAD_BAR, (key, k, e, np.abs(rg[k]).max())


# ---- inference ------------------------------------------------------------------------------------------------------------------------
def _beam_inputs(seed, B, T, F, H, E, V, proj_scale, cell, nl=2, nbi=1, **_):
    from tennis_amd import weights as W
    p = W.make_gnmt_weights(seed, cell, F, H, E, V, num_layers=nl, num_bi_layers=nbi)
    p["gnmt_tgt_proj_weight"] = (p["gnmt_tgt_proj_weight"] * proj_scale).astype(np.float32)   # peakier word distribution
    rng = np.random.default_rng(seed)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    vl = rng.integers(max(1, T // 3), T + 1, B).astype(np.int32)
    vl[0] = T
    return p, src, vl


def _beam_oracle(p, src, vl, H, beam, max_length, cell, nl=2, nbi=1, **_):
    rmem, rstates = gn.encoder(src, vl, p, cell, H, num_layers=nl, num_bi_layers=nbi, use_residual=False)
    dec = gn.Decoder(p, H, num_layers=nl, cell=cell, use_residual=False)
    rs, rsc, rvl = gn.beam_search(dec, rmem, rstates, vl, 2, 3, beam, 1.0, 5, max_length)
    return rmem, rs, rsc, rvl


@pytest.mark.parametrize("cfg", WS.BEAM_CASES, ids=lambda c: f"seed{c['seed']}-{c['cell']}-H{c['H']}")
def test_beam_search_matches_the_oracle(report, cfg):
    from tennis_amd.engine import GNMTCaptioner
    cell, B, T, H = (cfg[k] for k in ("cell", "B", "T", "H"))
    nl, nbi = cfg.get("nl", 2), cfg.get("nbi", 1)
    p, src, vl = _beam_inputs(**cfg)
    rmem, rs, rsc, rvl = _beam_oracle(p, src, vl, **cfg)
    # the case is no near tie: the oracle's own ids and lengths do not move under a 1e-5 relative perturbation of the source
    moved = 0.0
    for eps in (1e-5, -1e-5):
        _, qs, qsc, qvl = _beam_oracle(p, (src * np.float32(1.0 + eps)).astype(np.float32), vl, **cfg)
        assert qs.shape == rs.shape and np.array_equal(qs, rs) and np.array_equal(qvl, rvl), (cfg["seed"], eps)
        moved = max(moved, float(np.abs(qsc - rsc).max()))
    cap = GNMTCaptioner(p, cfg["F"], H, cfg["E"], cfg["V"], beam=cfg["beam"], max_length=cfg["max_length"], max_batch=B, max_src_len=T,
                        cell_type=cell, num_layers=nl, num_bi_layers=nbi)
    mem = cap.encode(_cuda(src), _cuda(vl)).cpu().numpy()
    samples, scores, vlen = cap.beam_search(2, 3, 1.0, 5.0)
    s, sc, v = samples.cpu().numpy(), scores.cpu().numpy(), vlen.cpu().numpy()
    emem, esc = np.abs(mem - rmem).max(), np.abs(sc - rsc).max()
    key = f"rnn_wide_beam_{cell}_seed{cfg['seed']}_B{B}_T{T}_H{H}_nl{nl}_nbi{nbi}"
    report[key + "_mem_abs_err"] = float(emem)
    report[key + "_score_abs_err"] = float(esc)
    print(f"{key}: mem {emem:.3e} scores {esc:.3e} (the oracle's scores move {moved:.3e} under the perturbation)")
    assert emem < 1e-4, (key, emem)
    assert s.shape == rs.shape, (s.shape, rs.shape)
    assert np.array_equal(v, rvl)
    assert np.array_equal(s, rs)                       # caption token ids equal
    assert esc < 1e-4, (key, esc)


# ---- the wide kernels on narrow shapes: the bits of the default routes -------------------------------------------------------------
def _wide_launches():
    import ctypes as C
    n = C.c_int64(-1)
    assert _lib().tn_dbg_rnn_wide_launches(C.byref(n)) == 0
    return n.value


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _head_step(cell, B, T, F, H, p, x, y):
    from tennis_amd.engine import TemporalHeadTrainer
    tr = TemporalHeadTrainer(p, F, H, 11, max_batch=B, max_steps=T, type=cell)
    loss, logits = tr.forward_backward(_cuda(x), _cuda(y))
    grads = tr.grads.cpu().numpy().copy()
    tr.step(B, 1e-2, 0.9, 1e-4)
    return loss.cpu().numpy(), logits.cpu().numpy(), grads, tr.params.cpu().numpy().copy()


def _captioner_step(cfg, p, src, svl, tgt, tvl):
    tr = _gnmt_trainer(cfg, p)
    loss, logits = tr.forward_backward(_cuda(src), _cuda(svl), _cuda(tgt), _cuda(tvl), return_logits=True)
    grads = tr.grads.cpu().numpy().copy()
    tr.step(1e-3)
    return np.float32(float(loss)), logits.cpu().numpy(), grads, tr.params.cpu().numpy().copy()


@pytest.mark.parametrize("cell,B,T,F,H", WS.FORCED_CASES)
def test_forced_wide_kernels_give_the_bits_of_the_default_routes(report, cell, B, T, F, H):
    p, x, vl = _birnn_inputs(cell, B, T, F, H, True)
    hp, hx, hy = _setup(4, B, T, F, H, 11, cell)
    cfg = dict(seed=27, cell=cell, B=B, T=T, F=F, H=H, E=6, V=12, L=4, nl=2, nbi=1)
    gp, src, svl, tgt, tvl = _gnmt_case(**cfg)
    svl[1] = 1
    n0 = _wide_launches()
    default = (_birnn_run(cell, B, T, F, H, 2, p, x, vl), _birnn_run(cell, B, T, F, H, 1, p, x, None),
               _head_step(cell, B, T, F, H, hp, hx, hy), _captioner_step(cfg, gp, src, svl, tgt, tvl))
    n1 = _wide_launches()
    try:
        assert _lib().tn_dbg_rnn_force_wide(1) == 0
        wide = (_birnn_run(cell, B, T, F, H, 2, p, x, vl), _birnn_run(cell, B, T, F, H, 1, p, x, None),
                _head_step(cell, B, T, F, H, hp, hx, hy), _captioner_step(cfg, gp, src, svl, tgt, tvl))
    finally:
        _lib().tn_dbg_rnn_force_wide(0)
    # which family ran: none of the wide kernels by default; under the hook the two forward calls, the head's forward + BPTT and the
    # captioner's two encoder layers, forward + BPTT each
    assert n1 == n0 and _wide_launches() - n1 == 2 + 2 + 4, (n0, n1, _wide_launches())
    names = (("birnn_vl", ("seq", "h_last", "c_last")), ("rnn_uni", ("seq", "h_last", "c_last")),
             ("head", ("loss", "logits", "grads", "params")), ("captioner", ("loss", "logits", "grads", "params")))
    differ = []
    for (what, parts), d, w in zip(names, default, wide):
        for name, a, b in zip(parts, d, w):
            if a is None and b is None:
                continue
            assert np.isfinite(a).all() and np.abs(a).max() > 0, (what, name)       # something was computed
            if not _same_bits(a, b):
                differ.append((what, name, float(np.abs(a - b).max())))
    report[f"rnn_wide_forced_{cell}_B{B}_T{T}_F{F}_H{H}_tensors_differing"] = len(differ)
    assert not differ, (cell, B, H, differ)


# ---- what stays refused ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from tennis_amd import weights as W
    from tennis_amd.engine import BiRNN, GNMTTrainer, TemporalHeadTrainer, WindowHead
    with pytest.raises(RuntimeError, match="2048"):
        BiRNN("gru", 32, 684, W.make_rnn_weights(0, "gru", 32, 684, "r_"), "r_")             # 2052 gate rows
    with pytest.raises(RuntimeError, match="2048"):
        BiRNN("lstm", 32, 516, W.make_rnn_weights(0, "lstm", 32, 516, "r_"), "r_")           # 2064
    hp, _, _ = _setup(4, 3, 4, 8, 516, 11, "lstm")
    with pytest.raises(RuntimeError, match="2048"):
        TemporalHeadTrainer(hp, 8, 516, 11, max_batch=3, max_steps=4, type="lstm")
    gp = W.make_gnmt_weights(1, "gru", 8, 684, 6, 12, num_layers=2, num_bi_layers=1)
    with pytest.raises(RuntimeError, match="2048"):
        GNMTTrainer(gp, 8, 684, 6, 12, max_batch=3, max_src_len=4, max_tgt_len=4, cell_type="gru")
    # dense windowed evaluation keeps the one-row-per-thread limit, and says whose limit it is
    p = W.make_rnn_weights(0, "gru", 32, 344, "w_gru0_")
    p.update(W.make_dense_weights(1, 11, 2 * 344, "w_dense0_"))
    with pytest.raises(RuntimeError, match="windowed kernel"):
        WindowHead("gru", 32, 344, 11, p, "w_gru0_", "w_dense0_")
    BiRNN("gru", 32, 344, W.make_rnn_weights(0, "gru", 32, 344, "r_"), "r_")                 # ... which the plain layer no longer has
