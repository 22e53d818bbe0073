"""No GPU: the references tests/test_gpu_linear_lat.py and tests/test_gpu_gnmt_beam_step.py rest on (tests/tools/gnmt_step_refs.py).

  * the formulas: the GEMM against float64 torch (both K ranges), the beam step against oracle/gnmt_np.py for one decoder step of a
    real search (scores, words, parents, lengths, alive flags; GRU and LSTM, with and without the residual);
  * the recipe: in every beam case float64's gaps between consecutive winners and behind the last one clear two bars (exact twins
    apart, which only the two tie cases have), the directed states are what their names say;
  * the mutant condition: every deliberate defect sits at least 10 bars from the reference in at least one compared output of every
    case it applies to, so the GPU tests can fail;
  * the launchers' slice arithmetic restated (step_groups, KQ, kn, NLD, nch, kbeg): the shape lists reach every named path, and a
    list with a row deleted misses one;
  * the two hooks are declared in the debug header, bound in tennis_amd/_lib.py and defined in csrc/gnmt_dbg.hip / csrc/dbg.hip."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import gnmt_np as gn
from tools import gnmt_step_refs as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ["tn_dbg_gnmt_beam_step", "tn_dbg_linear_lat"]
BEAM_IDS = [c["name"] for c in SR.BEAM_CASES]


# ---- the GEMM -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K,nsplit,K2", [(17, 356, 1024, None, None), (3, 30, 132, None, None)] + SR.LAT2_CASES)
def test_gemm_matches_float64_torch(M, N, K, nsplit, K2):
    inp = SR.lat_inputs(M, N, K)
    out = SR.lat_gemm(inp, nsplit=nsplit, K2=K2)
    X, W, b = (torch.tensor(inp[k].astype(np.float64)) for k in ("X", "W", "b"))
    ref = X @ W.T + b
    if nsplit is not None:
        ref[:, nsplit:] = X[:, :K2] @ W[nsplit:, :K2].T + b[nsplit:]
    assert np.abs(out["y"] - ref.numpy()).max() < 1e-12
    mag = X.abs() @ W.abs().T + b.abs()
    if nsplit is None:
        assert np.abs(out["y_mag"] - mag.numpy()).max() < 1e-11
    assert SR.rel_err(out["y"], out["y"], out["y_mag"]) == 0.0


@pytest.mark.parametrize("K,M,N", SR.LAT_SHAPES)
def test_gemm_mutants_are_ten_bars_away(K, M, N):
    inp = SR.lat_inputs(M, N, K)
    r64, r32 = SR.lat_gemm(inp), SR.lat_gemm(inp, np.float32)
    bar = SR.rel_bar(r64["y"], r32["y"], r64["y_mag"])
    assert SR.GEMM_TOL <= bar < 1e-4, bar
    for m in SR.LAT_MUTANTS:
        if SR.lat_mutant_applies(m, M, N, K):
            moved = SR.rel_err(SR.lat_gemm(inp, mutant=m)["y"], r64["y"], r64["y_mag"])
            assert moved >= SR.MUTANT_FACTOR * bar, (m, moved, bar)


@pytest.mark.parametrize("M,N,K,nsplit,K2", SR.LAT2_CASES)
def test_two_range_mutants_are_ten_bars_away(M, N, K, nsplit, K2):
    inp = SR.lat_inputs(M, N, K)
    r64, r32 = SR.lat_gemm(inp, nsplit=nsplit, K2=K2), SR.lat_gemm(inp, np.float32, nsplit=nsplit, K2=K2)
    bar = SR.rel_bar(r64["y"], r32["y"], r64["y_mag"])
    for m in SR.LAT_MUTANTS:
        if SR.lat_mutant_applies(m, M, N, K, nsplit) and SR.lat_mutant_applies(m, M, N, K2, nsplit):
            moved = SR.rel_err(SR.lat_gemm(inp, mutant=m, nsplit=nsplit, K2=K2)["y"], r64["y"], r64["y_mag"])
            assert moved >= SR.MUTANT_FACTOR * bar, (m, moved, bar)


def test_small_integer_operands_are_exact_in_float32():
    """the recipe behind the GPU test's bit-equality: integer products whose sums stay below 2^24"""
    for K, M, N in SR.LAT_SHAPES:
        inp = SR.lat_inputs(M, N, K, small_int=True)
        r64, r32 = SR.lat_gemm(inp), SR.lat_gemm(inp, np.float32)
        assert r64["y_mag"].max() < 2 ** 24 and np.array_equal(r64["y"], r32["y"].astype(np.float64))


def test_gemm_shapes_reach_every_path():
    reached = set().union(*(SR.lat_paths(M, N, K) for K, M, N in SR.LAT_SHAPES))
    assert reached >= SR.LAT_REQUIRED, SR.LAT_REQUIRED - reached
    for axis, want in ((0, (128, 132, 356, 384, 388, 612, 768, 772, 1024)), (1, (1, 3, 16, 17, 20, 160)), (2, (16, 30, 254, 356, 1024))):
        assert {s[axis] for s in SR.LAT_SHAPES} == set(want)
    # the list can miss: without the K = 132 row no wave lies wholly past K, without the K >= 772 rows no third round runs
    without = lambda drop: set().union(*(SR.lat_paths(M, N, K) for K, M, N in SR.LAT_SHAPES if K not in drop))
    assert "wave_past_K" not in without({132}) and "rounds3" not in without({772, 1024})
    assert SR.lat_slices(132) == dict(nch=3, kbeg=[0, 48, 96, 144], rounds=1)
    assert SR.lat_slices(388)["rounds"] == 2 and SR.lat_slices(768)["rounds"] == 2 and SR.lat_slices(772)["rounds"] == 3
    # the route cases sit on either side of K = 128 and of 4096 tiles
    tiles = {t: ((N + 15) // 16) * ((M + 15) // 16) for t, M, N, K, off, route in SR.LAT_ROUTE_CASES}
    assert tiles["tiles4096"] == 4096 and tiles["tiles4160"] == 4160


def test_k_group_major_layout_round_trips():
    a = np.arange(3 * 8, dtype=np.float32).reshape(3, 8)
    b = SR.k4(a, 5)
    assert b.shape == (2, 5, 4) and b[1, 2, 3] == a[2, 7] and b.reshape(-1)[((5 >> 2) * 5 + 1) * 4 + (5 & 3)] == a[1, 5]
    assert np.array_equal(SR.unk4(b.reshape(-1), 3, 8), a)


# ---- the beam step against the oracle's sampler ---------------------------------------------------------------------------------------

def _search_state(cell, res, n, seed, proj_scale, eos_bias):
    """n steps of oracle/gnmt_np.py's search, then the (n + 1)-th with its decoder call recorded -> (inputs of beam_step, oracle's
    results for that step)"""
    from tennis_amd import weights as W
    B, T, F, H, E, V, beam, bos, eos = 4, 9, 24, 16, 12, 30, 4, 2, 3
    p = W.make_gnmt_weights(seed, cell, F, H, E, V)
    p["gnmt_tgt_proj_weight"] = (p["gnmt_tgt_proj_weight"] * proj_scale).astype(np.float32)       # (flat logits end every beam at once)
    p["gnmt_tgt_proj_bias"][eos] += eos_bias
    rng = np.random.default_rng(seed)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    vl = np.array([T, 5, 7, 3], dtype=np.int32)
    mem, states = gn.encoder(src, vl, p, cell, H)
    dec = gn.Decoder(p, H, cell=cell, use_residual=res)
    sA, scA, vlA = gn.beam_search(dec, mem, states, vl, bos, eos, beam, 1.0, 5, n)
    calls = []
    step0 = dec.step

    def recording(tokens, rnn_states, att, rows):
        r = step0(tokens, rnn_states, att, rows)
        calls.append(([s.copy() for s in rnn_states], r))
        return r
    dec.step = recording
    sB, scB, vlB = gn.beam_search(dec, mem, states, vl, bos, eos, beam, 1.0, 5, n + 1)
    assert sA.shape[2] == n + 2 and sB.shape[2] == n + 3 and len(calls) == n + 1, "the search ended early"
    alive_n = sA[:, :, -1] == eos
    rnn_in, (logp, new_states, ctx) = calls[-1]
    lstm = cell == "lstm"
    hprev, c1 = (rnn_in[2], rnn_in[3]) if lstm else (rnn_in[1], None)
    h0 = new_states[0]
    x = np.concatenate([h0, ctx], axis=1).astype(np.float64)
    gi = x @ p["gnmt_dec_rnn1_i2h_weight"].T.astype(np.float64) + p["gnmt_dec_rnn1_i2h_bias"]
    gh = hprev.astype(np.float64) @ p["gnmt_dec_rnn1_h2h_weight"].T.astype(np.float64) + p["gnmt_dec_rnn1_h2h_bias"]
    g1 = gi + gh if lstm else np.concatenate([gi[:, :2 * H] + gh[:, :2 * H], gi[:, 2 * H:], gh[:, 2 * H:]], axis=1)
    lp, prev_lp = SR.length_penalties(n + 1)
    R = B * beam
    inp = dict(beam=beam, lstm=lstm, residual=res, form="x0_rm", step=n + 1, lp=lp, prev_lp=prev_lp, eos=eos, KQ=16,
               g1=g1.astype(np.float32), hprev=hprev, c1=c1, xin=h0, xctx=ctx, wp=p["gnmt_tgt_proj_weight"], bp=p["gnmt_tgt_proj_bias"],
               scores=scA.reshape(-1), alive=alive_n.reshape(-1).astype(np.int32), vlen=(vlA - alive_n).reshape(-1).astype(np.int32),
               emb=p["gnmt_tgt_embed_weight"], ctxv=ctx, h0n=h0, c0n=new_states[1] if lstm else np.zeros((R, H), np.float32))
    alive_n1 = sB[:, :, -1] == eos
    want = dict(scores=scB.reshape(-1), word=sB[:, :, n + 1].reshape(-1), vlen=(vlB - alive_n1).reshape(-1), alive=alive_n1.reshape(-1),
                prefix_before=sA[:, :, :n + 1], prefix_after=sB[:, :, :n + 1], h1=new_states[2 if lstm else 1])
    return inp, want


# (projection scale, eos bias) at which the fifth step of the search sees finished and unfinished beams side by side
@pytest.mark.parametrize("cell,res,proj_scale,eos_bias", [("gru", False, 40.0, 1.0), ("lstm", False, 40.0, 0.0), ("gru", True, 40.0, 1.0),
                                                          ("lstm", True, 10.0, 0.0)])
def test_beam_step_matches_the_oracle_sampler(cell, res, proj_scale, eos_bias):
    inp, want = _search_state(cell, res, n=4, seed=2, proj_scale=proj_scale, eos_bias=eos_bias)
    al = inp["alive"].astype(bool)
    assert al.any() and not al.all(), "the recorded step should see finished and unfinished beams"
    beam = inp["beam"]
    for dt, tol in ((np.float32, 2e-5), (np.float64, 2e-5)):
        out = SR.beam_step(inp, dt)
        assert np.abs(out["scores"] - want["scores"]).max() < tol
        for k in ("word", "vlen", "alive"):
            assert np.array_equal(out[k], want[k].astype(out[k].dtype)), k
        B = want["prefix_before"].shape[0]
        flat = out["par"].reshape(B, beam) + np.arange(B)[:, None] * beam
        assert np.array_equal(want["prefix_before"].reshape(B * beam, -1)[flat], want["prefix_after"])
        assert np.abs(out["h"] - want["h1"]).max() < 1e-5          # the cell's new state, before the gather
        assert (out["word"] == -1).any() and out["flag"] == int(want["alive"].any())
        assert np.array_equal(out["x0"][:, :inp["emb"].shape[1]], inp["emb"][np.maximum(out["word"], 0)])


# ---- the beam cases -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BEAM_IDS)
def test_beam_case_winners_are_separated_and_states_are_as_named(name):
    c = SR.BEAM_BY_NAME[name]
    beam, V = c["beam"], c["V"]
    for cell in SR.BEAM_CELLS:
        inp, r64, r32, seed = SR.beam_inputs(name, cell)
        bars = SR.beam_bars(r64, r32)
        assert SR.GEMM_TOL <= bars["scores"] < 1e-4 and SR.GEMM_TOL <= bars["h"] < 1e-4, bars
        gap, zeros = SR.beam_gaps(r64, bars["scores"], beam)
        assert gap > SR.GAP_BARS and (zeros > 0) == (c["tie"] is not None), (name, cell, gap, zeros)
        # float32 selects as float64 does: the bars' own evaluation agrees on the discrete outputs
        assert all(np.array_equal(r64[k], r32[k]) for k in ("par", "word", "vlen", "alive")) and r64["flag"] == r32["flag"]
        assert max(SR.ratio(*v) for v in SR.beam_compare(SR.as_got(r32, inp), inp, r64, r32).values()) <= 1.0 / SR.MARGIN + 1e-12
        B = c["B"]
        word, par, al = r64["word"].reshape(B, beam), r64["par"].reshape(B, beam), inp["alive"].reshape(B, beam)
        st = c["state"]
        if st == "step1":
            assert inp["prev_lp"] == 1.0 and (par == 0).all() and (word >= 0).all()
        if st == "mixed":
            assert (word == -1).any() and (word >= 0).any() and r64["flag"] == 1 and (al.sum(axis=1) < beam).all()
        if st == "all_finished":
            assert r64["flag"] == 0 and (word == -1).all() and not r64["alive"].any()
            assert np.array_equal(r64["scores"].reshape(B, beam), -np.sort(-inp["scores"].reshape(B, beam).astype(np.float64), axis=1))
            assert (par != np.arange(beam)[None, :]).any()          # the beams come out in score order, not in place
        if st == "eos_wins":
            assert (word[:, 0] == inp["eos"]).all() and (r64["alive"].reshape(B, beam)[:, 0] == 0).all() and r64["flag"] == 1
        if st == "single_alive":
            assert (al.sum(axis=1) == 1).all() and (word == -1).any() and (par[word >= 0] == beam - 1).all()
        if c["maxcol"] is not None:
            logits = r64["out"] @ inp["wp"].astype(np.float64).T + inp["bp"]
            assert (logits.argmax(axis=1) == inp["maxcol"]).all()
            Vp = (V + 3) & ~3
            want = {0: 0, 63: 63, 64: 64, "last": V - 1}.get(c["maxcol"])
            assert inp["maxcol"] == want if want is not None else Vp - 4 <= inp["maxcol"] < V - 1 and V % 4 != 0
        if c["tie"] == "rows":
            assert ((par[:, 0] == 1) & (par[:, 1] == 2) & (word[:, 0] == word[:, 1])).all()
            assert (r64["scores"].reshape(B, beam)[:, 0] == r64["scores"].reshape(B, beam)[:, 1]).all()
        if c["tie"] == "cols":
            assert (word[:, 0] == 5).all() and (word[:, 1] == 40).all() and (par[:, 0] == par[:, 1]).all()


@pytest.mark.parametrize("name", BEAM_IDS)
def test_beam_mutants_are_ten_bars_away(name):
    c = SR.BEAM_BY_NAME[name]
    for cell in SR.BEAM_CELLS:
        inp, r64, r32, _ = SR.beam_inputs(name, cell)
        for m in SR.BEAM_MUTANTS:
            if not SR.beam_mutant_applies(m, c, cell):
                continue
            res = SR.beam_compare(SR.as_got(SR.beam_step(inp, mutant=m), inp), inp, r64, r32)
            worst = max(SR.ratio(*v) for v in res.values())
            assert worst >= SR.MUTANT_FACTOR, (name, cell, m, {k: SR.ratio(*v) for k, v in res.items()})


def test_every_beam_mutant_applies_somewhere():
    for m in SR.BEAM_MUTANTS:
        assert sum(SR.beam_mutant_applies(m, c, cell) for c in SR.BEAM_CASES for cell in SR.BEAM_CELLS) >= 2, m


def test_beam_shapes_reach_every_path():
    reached = set().union(*(SR.beam_paths(c) for c in SR.BEAM_CASES))
    assert reached >= SR.BEAM_REQUIRED, SR.BEAM_REQUIRED - reached
    without = lambda name: set().union(*(SR.beam_paths(c) for c in SR.BEAM_CASES if c["name"] != name))
    assert "max_col0" not in without("b4_H260_V256") and "twin_cols" not in without("b5_H8_V61_twin_cols")
    assert SR.beam_paths(SR.BEAM_BY_NAME["b10_H256_V254_lowered"]) >= {"lowered_split", "KQ8", "NBM16", "max_col_last4"}
    assert "NLD16_vec_then_tail" in SR.beam_paths(SR.BEAM_BY_NAME["b4_H260_V256"])
    # the arithmetic itself, at the shapes the issue names
    L = SR.beam_launch(4, 260, 256)
    assert (L["nbm"], L["KQ"], L["kn"], L["NLD"]) == (4, 16, 17, 16) and all((s["vec"], s["tail"]) == (1, 1) for s in L["slices"][:15])
    L = SR.beam_launch(4, 256, 254)
    assert L["kn"] == 16 and all((s["vec"], s["tail"]) == (1, 0) for s in L["slices"])
    L = SR.beam_launch(5, 100, 254)
    assert L["kn"] == 7 and L["slices"][15]["k0"] == 105 and L["slices"][15]["n"] == 0 and L["slices"][14] == dict(k0=98, n=2, vec=0, tail=2)
    L = SR.beam_launch(10, 256, 254)
    assert L["natural"] == 8 and L["KQ"] == 8 and SR.beam_lds_bytes(256, 254, 10, 16) > SR.STEP_LDS_MAX >= L["lds"]
    assert SR.beam_launch(5, 100, 254, 4)["KQ"] == 4 and SR.beam_launch(5, 100, 254, 1)["KQ"] == 1
    assert [SR.beam_launch(b, 40, v)["KQ"] for b, v in ((4, 256), (4, 257), (4, 512), (4, 516), (4, 1000))] == [16, 8, 8, 4, 4]
    assert [SR.beam_nbm(b) for b in (1, 3, 4, 5, 6, 7, 8, 9, 16)] == [4, 4, 4, 5, 8, 8, 8, 16, 16]
    assert all(SR.beam_launch(c["beam"], c["H"], c["V"], c["split_cap"])["lds"] <= SR.STEP_LDS_MAX for c in SR.BEAM_CASES)
    assert SR.step_groups(16, 16) == 64 and SR.step_groups(65, 16) == 128 and SR.step_groups(129, 16) == 256 and SR.step_groups(16, 4) == 256


def test_restated_arithmetic_matches_the_source():
    """the constants restated in tools/gnmt_step_refs.py are the ones the kernels are built with"""
    cap = "".join(open(os.path.join(ROOT, "tennis_amd", "csrc", f)).read() for f in ("gnmt_kernels.h", "gnmt_kernels.hip"))
    lin =open(os.path.join(ROOT, "tennis_amd", "csrc", "linear.h")).read()
    assert "constexpr int NLD = NBM <= 5 ? 16 : NBM <= 8 ? 8 : 2;" in cap
    assert "constexpr size_t kStepLdsMax = 152 * 1024;" in cap and "constexpr float kNeg = -1e18f;" in cap
    assert "const int g = n4 <= 64 ? 64 : n4 <= 128 ? 128 : 256, floor_g = 1024 / split;" in cap
    assert "return beam <= 4 ? 4 : beam == 5 ? 5 : beam <= 8 ? 8 : 16;" in cap
    assert "constexpr int kLatGroup = 6;" in lin and "const int nch = (K + 63) / 64;" in lin and "const int kbeg = wq * nch * 16;" in lin


# ---- the hooks exist ------------------------------------------------------------------------------------------------------------------

def test_hooks_are_declared_bound_and_defined():
    from tennis_amd import _lib
    header = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    source = "".join(open(os.path.join(ROOT, "tennis_amd", "csrc", f)).read() for f in ("gnmt_dbg.hip", "dbg.hip"))
    for name in HOOKS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r'extern "C" int ' + name + r"\s*\(", source), name
        assert name in _lib.declared_symbols(), name
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in HOOKS:
            assert hasattr(lib, name), name
