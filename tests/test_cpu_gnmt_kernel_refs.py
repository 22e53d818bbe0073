"""No GPU: the references tests/test_gpu_gnmt_kernels.py rests on (tests/tools/gnmt_kernel_refs.py).

  * the NumPy formulas against torch autograd in float64: ds, dq, d mem and d keyproj of a hand-built attention forward, the
    cross-entropy gradient against log_softmax, the embedding gradient against an index_add;
  * the input recipe: every attention case's scores spread by 1 to 2 over the valid steps (clearly non-uniform, not saturated);
  * the mutant condition: every deliberate defect moves the output it damages by at least 10 bars, so the GPU test can fail;
  * the five hooks are declared in the debug header, bound in tennis_amd/_lib.py and defined in csrc/gnmt_dbg.hip."""
import os
import re

import numpy as np
import pytest
import torch

from tools import gnmt_kernel_refs as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ["tn_dbg_gnmt_attention_fwd", "tn_dbg_gnmt_attention_bwd", "tn_dbg_gnmt_attention_outer", "tn_dbg_gnmt_ce", "tn_dbg_gnmt_emb_grad"]
ATT_IDS = [c[0] for c in KR.ATT_CASES]


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


# ---- the formulas against autograd ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["T5_H8", "T129_H20", "T214_H64"])
def test_attention_backward_matches_autograd(name):
    """loss = sum(ctx * dctx) with ctx = softmax(h . kp / sqrt(H)) mem over the valid steps: d loss / d scores = ds, d loss / d h =
    dh0; summed over `steps` hand-built decoder steps, d loss / d mem and d loss / d keyproj are the outer kernel's two outputs"""
    _, T, H, vl, cells, _ = KR.ATT_BY_NAME[name]
    fin = KR.case_inputs(name, cells[0])
    B = len(vl)
    rng = np.random.default_rng(3)
    steps = 3
    mem, kp = _t(fin["mem"], True), _t(fin["keyproj"], True)
    mask = torch.arange(T)[None, :] < torch.tensor(KR.clamp_len(vl, T))[:, None]
    aw, ds, dctx_all, h_all = [], [], [], []
    loss = 0.0
    for _ in range(steps):
        h = _t(rng.standard_normal((B, H)).astype(np.float32), True)
        c0 = rng.standard_normal((B, H + 4)).astype(np.float32)
        c1 = rng.standard_normal((B, 2 * H + 8)).astype(np.float32)
        score = torch.einsum("bh,bth->bt", h / np.sqrt(H), kp)
        score.retain_grad()
        w = torch.softmax(torch.where(mask, score, torch.full_like(score, -1e18)), dim=1) * mask
        ctx = torch.einsum("bt,bth->bh", w, mem)
        step_loss = (ctx * _t(c0[:, :H] + c1[:, :H].astype(np.float64))).sum()
        g_score, g_h = torch.autograd.grad(step_loss, [score, h], retain_graph=True)
        loss = loss + step_loss
        w64 = w.detach().numpy()                             # float64 throughout: the formulas are compared, not a rounding
        out = KR.attention_bwd(dict(aw=w64, mem=fin["mem"], keyproj=fin["keyproj"], c0=c0, c1=c1, valid_len=fin["valid_len"]))
        assert KR.err("ds", g_score.numpy(), out) < 1e-12 and KR.err("dh0", g_h.numpy(), out) < 1e-12
        assert np.array_equal(out["dctx"], c0[:, :H].astype(np.float64) + c1[:, :H])
        aw.append(w64); ds.append(out["ds"]); dctx_all.append(out["dctx"]); h_all.append(h.detach().numpy())
    loss.backward()
    outer = KR.attention_outer(dict(aw=np.stack(aw), ds=np.stack(ds), dctx=np.stack(dctx_all), h0=np.stack(h_all)))
    assert KR.err("dmem", mem.grad.numpy(), outer) < 1e-12 and KR.err("dkp", kp.grad.numpy(), outer) < 1e-12


@pytest.mark.parametrize("V,L", [(3, 1), (257, 7), (1000, 7)])
def test_cross_entropy_matches_log_softmax(V, L):
    inp = KR.ce_inputs(V, L)
    out = KR.ce(inp)
    z = _t(inp["logits"], True)
    lab = torch.tensor(inp["labels"][:, :L].astype(np.int64))
    vl = torch.tensor(inp["valid_len"].astype(np.int64))
    nll = -torch.gather(torch.log_softmax(z, dim=2), 2, lab[:, :, None]).squeeze(2)
    m = (torch.arange(L)[None, :] < vl[:, None]).to(torch.float64)
    ntok = float(vl.clamp(0, L).sum())
    loss = (nll * m).sum() / ntok
    loss.backward()
    assert abs(float(loss.detach()) - out["loss"]) < 1e-12 * max(1.0, abs(float(loss.detach())))
    assert np.abs(z.grad.numpy().transpose(1, 0, 2) - out["dlogits"]).max() < 1e-14
    assert np.abs((nll * m).mean(dim=1).detach().numpy() - out["masked_loss"]).max() < 1e-11
    assert np.abs(out["loss_rows"].sum() - out["loss"]) < 1e-12
    zero = KR.ce(KR.ce_inputs(V, L, all_masked=True))
    assert all(not np.any(zero[k]) for k in ("dlogits", "loss_rows", "loss", "masked_loss"))


def test_embedding_gradient_matches_index_add():
    inp = KR.emb_inputs(65, 300)
    out = KR.emb_grad(inp)
    ref = torch.zeros((300, 65), dtype=torch.float64)
    tok = torch.tensor(inp["tgt"][:, :inp["L"]].astype(np.int64)).clamp(min=0)
    for i in range(inp["L"]):
        ref.index_add_(0, tok[:, i], _t(inp["dx0"][i, :, :65]))
    assert np.abs(ref.numpy() - out["demb"]).max() < 1e-13
    used = set(np.maximum(inp["tgt"][:, :inp["L"]], 0).ravel().tolist())
    assert {0, 3}.issubset(used) and (inp["tgt"][:, :inp["L"]] < 0).any() and len(used) < 6
    assert not out["demb"][[v for v in range(300) if v not in used]].any()


# ---- the recipe -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ATT_IDS)
def test_scores_are_spread_not_uniform_not_saturated(name):
    _, T, H, vl, cells, spread = KR.ATT_BY_NAME[name]
    for cell in cells:
        ref = KR.attention_fwd(KR.case_inputs(name, cell))
        sds = KR.score_spread(ref["scores"])
        assert sds, name
        if KR.is_saturated(name):
            assert all(20.0 < s < 40.0 for s in sds), sds
            assert max(float(ref["w"][0].max()), float(ref["w"][1].max())) > 0.99       # one-hot: the other steps carry no weight
        else:
            assert all(1.0 <= s <= 2.0 for s in sds), (name, cell, sds)
        assert np.isfinite(ref["w"]).all() and np.allclose(ref["w"].sum(axis=1), 1.0, atol=1e-12)


def test_beam_case_scores_are_spread():
    """five rows share a clip's key projection, so only the clip's mean spread can be set: it is 1 to 2, and no row of 16 to 21
    steps leaves 0.5 to 3 (its own |q| and the sample's noise move it) - still neither uniform nor saturated"""
    c = KR.BEAM_CASE
    vl = tuple(int(v) for v in KR.beam_valid_len())
    sds = KR.score_spread(KR.attention_fwd(KR.attention_inputs(c["T"], c["H"], vl, False, 1.5, c["beam"]))["scores"])
    assert len(sds) == c["beam"] * c["clips"] and all(0.5 <= s <= 3.0 for s in sds), sds
    assert all(1.0 <= m <= 2.0 for m in np.asarray(sds).reshape(c["clips"], c["beam"]).mean(axis=1))


# ---- the mutant condition ---------------------------------------------------------------------------------------------------------

def _applies(mutant, T, vl):
    v = KR.clamp_len(vl, T)
    return {"drop_last": (v >= 2).any(), "drop_128": (v > 128).any(), "extra_step": ((v >= 1) & (v < T)).any(), "drop_dq16": True}[mutant]


def _assert_mutant(tag, keys, ref64, ref32, mut):
    for k in keys:
        b, moved = KR.bar(k, ref64, ref32), KR.err(k, mut[k], ref64)
        assert moved >= KR.MUTANT_FACTOR * b, (tag, k, moved, b, moved / b)


@pytest.mark.parametrize("name", [n for n in ATT_IDS if not KR.is_saturated(n)])
def test_forward_mutants_are_ten_bars_away(name):
    _, T, H, vl, cells, _ = KR.ATT_BY_NAME[name]
    for cell in cells:
        inp = KR.case_inputs(name, cell)
        ref64, ref32 = KR.attention_fwd(inp), KR.attention_fwd(inp, np.float32)
        for m in KR.FWD_MUTANTS:
            if _applies(m, T, vl):
                _assert_mutant((name, cell, m), ("w", "ctx"), ref64, ref32, KR.attention_fwd(inp, mutant=m))


@pytest.mark.parametrize("name", [n for n in ATT_IDS if not KR.is_saturated(n)])
def test_backward_mutants_are_ten_bars_away(name):
    _, T, H, vl, _, _ = KR.ATT_BY_NAME[name]
    inp = KR.attention_bwd_inputs(name)
    ref64, ref32 = KR.attention_bwd(inp), KR.attention_bwd(inp, np.float32)
    for m in KR.BWD_MUTANTS:
        if _applies(m, T, vl):
            _assert_mutant((name, m), ("dh0",) if m == "drop_dq16" else ("ds", "dh0"), ref64, ref32, KR.attention_bwd(inp, mutant=m))
    # one addend absent: the other must carry the whole gradient
    one = KR.attention_bwd(inp, use_c1=False)
    assert KR.err("dctx", one["dctx"], ref64) > 0.1


@pytest.mark.parametrize("steps,T,H", KR.OUTER_CASES)
def test_outer_mutants_are_ten_bars_away(steps, T, H):
    inp = KR.attention_outer_inputs(steps, T, H)
    ref64, ref32 = KR.attention_outer(inp), KR.attention_outer(inp, np.float32)
    for m in KR.OUTER_MUTANTS:
        if m != "drop_128" or T > 128:
            _assert_mutant((steps, T, H, m), ("dmem", "dkp"), ref64, ref32, KR.attention_outer(inp, mutant=m))


@pytest.mark.parametrize("V,L", KR.CE_CASES)
def test_cross_entropy_mutant_is_ten_bars_away(V, L):
    inp = KR.ce_inputs(V, L)
    ref64, ref32 = KR.ce(inp), KR.ce(inp, np.float32)
    assert np.isfinite(ref32["dlogits"]).all() and np.isfinite(ref32["loss"])
    _assert_mutant((V, L), ("dlogits", "loss_rows", "loss", "masked_loss"), ref64, ref32, KR.ce(inp, mutant="drop_last_column"))
    # the recipe's edges: a row whose maximum sits in the last column, a label at V - 1, rows shifted by +100
    assert int(inp["logits"][3, L - 1].argmax()) == V - 1 and inp["labels"][0, L - 1] == V - 1 and inp["logits"][0, 0].min() > 80


def test_bars_come_from_the_reference_alone():
    """a bar is max(GEMM_TOL of the magnitude, 16 x the float32 evaluation's error): finite, positive, and far below a visible error"""
    inp = KR.case_inputs("T260_H256", "gru")
    ref64, ref32 = KR.attention_fwd(inp), KR.attention_fwd(inp, np.float32)
    for k in ("h", "w", "ctx"):
        b = KR.bar(k, ref64, ref32)
        assert KR.floor(k, ref64) <= b < 1e-4, (k, b)
    assert KR.err("ctx", ref64["ctx"], ref64) == 0.0


# ---- the hooks exist --------------------------------------------------------------------------------------------------------------

def test_hooks_are_declared_bound_and_defined():
    from tennis_amd import _lib
    header = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    source = open(os.path.join(ROOT, "tennis_amd", "csrc", "gnmt_dbg.hip")).read()
    for name in HOOKS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r'extern "C" int ' + name + r"\s*\(", source), name
        assert name in _lib.declared_symbols(), name
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in HOOKS:
            assert hasattr(lib, name), name
