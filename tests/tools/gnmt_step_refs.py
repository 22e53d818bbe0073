"""Shapes, input recipes and plain NumPy references for the two pieces of the decoder's hot path that tests/tools/gnmt_kernel_refs.py
leaves out (tests only): what tests/test_cpu_gnmt_step_refs.py checks on the CPU and tests/test_gpu_linear_lat.py /
tests/test_gpu_gnmt_beam_step.py run through tn_dbg_linear_lat / tn_dbg_gnmt_beam_step.

  lat_gemm     Y = X W^T + b, optionally with two K ranges      (csrc/linear.h lat_tile_f32 behind launch_linear_f32_lat2 / _lat_wk4)
  beam_step    last decoder cell, residual, projection, log-softmax, length-penalised candidates, finished beams, stable top-`beam`,
               the sampler's bookkeeping and the re-gather by parent     (csrc/gnmt_kernels.hip dec_beam_kernel<NBM>)

Each formula is written once and evaluated in float64 (the reference) and in float32 (whose distance n from float64 sets the bar,
max(GEMM_TOL, MARGIN * n) of the magnitude of an element's terms).  Both take ``mutant``: a deliberate defect of the kind the
kernels' loop bounds and branches produce; the CPU test shows every mutant at least MUTANT_FACTOR bars away.

``lat_paths`` and ``beam_paths`` restate the launchers' slice arithmetic (step_groups, KQ, kn, NLD, nch, kbeg) and name the code
paths a shape reaches; the CPU test asserts that the shape lists below reach every path in LAT_REQUIRED / BEAM_REQUIRED."""
from __future__ import annotations

import functools

import numpy as np

from tools.gnmt_kernel_refs import GEMM_TOL, MARGIN, MUTANT_FACTOR, TINY, cell0     # noqa: F401  (re-exported)

K_NEG = np.float32(-1e18)          # gnmt_kernels.hip kNeg

# ---- the latency GEMM ---------------------------------------------------------------------------------------------------------------
LAT_GROUP = 6                      # linear.h kLatGroup: 16-wide k chunks a wave requests per round
LAT_FORMS = ("rm", "wk4", "wk4xk4")       # row-major operands; W k-group-major; W and X k-group-major
# (K, M, N): every K, M and N of the issue at least once; each form runs all nine
LAT_SHAPES = [(128, 1, 16), (132, 3, 30), (356, 16, 254), (384, 17, 356), (388, 20, 1024), (612, 160, 30), (768, 1, 254),
              (772, 3, 16), (1024, 17, 356)]
LAT_LDW_PAD, LAT_LDX_PAD, LAT_LDY_PAD, LAT_XROWS_PAD = 16, 8, 7, 5      # ldw = K + 16, ldx = K + 8, ldy = N + 7, X rows = M + 5
LAT2_CASES = [(20, 64, 384, 32, 256), (20, 64, 384, 32, 132)]           # (M, N, K, nsplit, K2): the two-range form
# both sides of each dispatch boundary: (tag, M, N, K, X offset in floats, expected route 0 lat / 2 fallback)
LAT_ROUTE_CASES = [("K124", 3, 16, 124, 0, 2), ("K128", 3, 16, 128, 0, 0), ("X_one_float_off", 3, 16, 128, 1, 2),
                   ("tiles4096", 1024, 1024, 128, 0, 0), ("tiles4160", 1025, 1024, 128, 0, 2)]
LAT_MUTANTS = ("drop_last4", "drop_chunk6_wave0", "drop_quarter", "drop_bias", "full_K_past_nsplit", "drop_last_row", "drop_last_col")
LAT_REQUIRED = {"rounds1", "rounds2", "rounds3", "wave_past_K", "quarter_cut_by_K", "row_clamp", "col_clamp", "full_tile_rows",
                "full_tile_cols", "many_row_tiles"}


def lat_slices(K):
    """lat_tile_f32's split of K: nch 16-wide chunks per wave, wave wq starts at kbeg[wq], rounds of LAT_GROUP chunks"""
    nch = (K + 63) // 64
    return dict(nch=nch, kbeg=[wq * nch * 16 for wq in range(4)], rounds=(nch + LAT_GROUP - 1) // LAT_GROUP)


def lat_paths(M, N, K):
    s = lat_slices(K)
    p = {f"rounds{s['rounds']}"}
    if any(kb >= K for kb in s["kbeg"]):
        p.add("wave_past_K")
    if any(kb < K < kb + s["nch"] * 16 for kb in s["kbeg"]):
        p.add("quarter_cut_by_K")
    p.add("row_clamp" if M % 16 else "full_tile_rows")
    p.add("col_clamp" if N % 16 else "full_tile_cols")
    if M > 16:
        p.add("many_row_tiles")
    return p


@functools.lru_cache(maxsize=None)
def lat_inputs(M, N, K, small_int=False):
    rng = np.random.default_rng(100000 + 1000 * M + 7 * N + K + (1 if small_int else 0))
    if small_int:       # every product and partial sum is an integer below 2^24: any summation order gives the same bits
        f = lambda *shape: rng.integers(-3, 4, shape).astype(np.float32)
    else:
        f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(X=f(M, K), W=f(N, K), b=f(N))


def _lat_keep(K, mutant):
    """the k values a (possibly defective) tile contracts"""
    keep = np.ones(K, dtype=bool)
    s = lat_slices(K)
    if mutant == "drop_last4":
        keep[K - 4:] = False
    elif mutant == "drop_chunk6_wave0":           # the first chunk of the second round of wave 0
        keep[LAT_GROUP * 16:min(LAT_GROUP * 16 + 16, K, s["nch"] * 16)] = False
    elif mutant == "drop_quarter":                # wave 1's quarter
        keep[s["kbeg"][1]:min(s["kbeg"][2], K)] = False
    return keep


def lat_mutant_applies(mutant, M, N, K, nsplit=None):
    if mutant == "drop_chunk6_wave0":
        return lat_slices(K)["nch"] > LAT_GROUP
    if mutant == "full_K_past_nsplit":
        return nsplit is not None and nsplit < N
    return True


def lat_gemm(inp, dt=np.float64, mutant=None, nsplit=None, K2=None, bias=True):
    """-> dict(y (M,N), y_mag): columns from nsplit on contract only k < K2"""
    X, W, b = inp["X"].astype(dt), inp["W"].astype(dt), inp["b"].astype(dt)
    M, K = X.shape
    N = W.shape[0]
    y, mag = np.zeros((M, N), dtype=dt), np.zeros((M, N), dtype=dt)
    ranges = [(0, N, K)] if nsplit is None or nsplit >= N else [(0, nsplit, K), (nsplit, N, K if mutant == "full_K_past_nsplit" else K2)]
    for n0, n1, kk in ranges:
        keep = _lat_keep(kk, mutant)
        y[:, n0:n1] = X[:, :kk][:, keep] @ W[n0:n1, :kk][:, keep].T
        mag[:, n0:n1] = np.abs(X[:, :kk][:, keep]) @ np.abs(W[n0:n1, :kk][:, keep]).T
    if bias and mutant != "drop_bias":
        y += b[None, :]
    if bias:
        mag += np.abs(b)[None, :]
    if mutant == "drop_last_row":
        y[M - 1] = 0
    if mutant == "drop_last_col":
        y[:, N - 1] = 0
    return dict(y=y.astype(dt), y_mag=mag)


def rel_err(got, ref, mag):
    """worst |got - ref| / magnitude; an element without terms (magnitude 0) must be exactly 0"""
    g, r, m = (np.asarray(a, dtype=np.float64) for a in (got, ref, mag))
    d = np.abs(g - r)
    if (d[m == 0] != 0).any() or not np.isfinite(g).all():
        return float("inf")
    return float((d[m > 0] / np.maximum(m[m > 0], TINY)).max()) if (m > 0).any() else 0.0


def rel_bar(ref64, ref32, mag, margin=MARGIN):
    """max(GEMM_TOL, margin * n), n the float32 evaluation's distance from float64 in the same metric: from the reference alone"""
    return max(GEMM_TOL, margin * rel_err(ref32, ref64, mag))


def abs_bar(ref64, ref32, margin=MARGIN):
    """the same with magnitude 1 (states in (-1, 1), cell states of order 1)"""
    return max(GEMM_TOL, margin * float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max()))


def k4(a, rows):
    """(m, K) row-major -> k-group-major with `rows` >= m rows: element (m, k) at ((k / 4) * rows + m) * 4 + k % 4; pad rows NaN-free
    sentinels (7.0)"""
    m, K = a.shape
    assert K % 4 == 0 and rows >= m
    out = np.full((K // 4, rows, 4), 7.0, dtype=np.float32)
    out[:, :m, :] = a.reshape(m, K // 4, 4).transpose(1, 0, 2)
    return out


def unk4(buf, m, K):
    return np.ascontiguousarray(buf.reshape(K // 4, -1, 4)[:, :m, :].transpose(1, 0, 2)).reshape(m, K)


# ---- the beam-search step -----------------------------------------------------------------------------------------------------------
PROJ_SCALE = 1.0          # the projection is NOT peaked: every vocabulary column counts in the log-sum-exp
BEAM_STEP, BEAM_K, BEAM_ALPHA = 3, 5.0, 1.0        # a step past the first: prev_lp != 1
BEAM_E = 10
BEAM_CELLS = ("gru", "lstm")


def _c(name, beam, H, V, B, form, state, hstate=False, maxcol=None, tie=None, split_cap=0):
    return dict(name=name, beam=beam, H=H, V=V, B=B, form=form, state=state, hstate=hstate, maxcol=maxcol, tie=tie, split_cap=split_cap)


# form: "tok_k4" token form, x1 k-group-major, p0 tiles beside the clips; "x0_rm" x0 form, x1 row-major; "tok_rm" token form with
# the p0 tiles reading a row-major x1 (no production caller).  maxcol: the column given the largest logit ("last4": the first column of
# the last, partly padded float4).  state: see beam_inputs.
BEAM_CASES = [
    _c("b1_H8_V30", 1, 8, 30, 1, "x0_rm", "alive"),
    _c("b3_H100_V61", 3, 100, 61, 3, "tok_k4", "mixed", hstate=True),
    _c("b4_H256_V254_step1", 4, 256, 254, 12, "tok_k4", "step1"),
    _c("b4_H260_V256", 4, 260, 256, 3, "x0_rm", "mixed", hstate=True, maxcol=0),
    _c("b5_H260_V257", 5, 260, 257, 3, "tok_k4", "mixed", maxcol=63),
    _c("b5_H100_V254_eos", 5, 100, 254, 3, "x0_rm", "eos_wins"),
    _c("b5_H100_V254_split4", 5, 100, 254, 3, "x0_rm", "mixed", split_cap=4),
    _c("b5_H100_V254_split1", 5, 100, 254, 3, "x0_rm", "mixed", split_cap=1),
    _c("b5_H256_V516_single", 5, 256, 516, 1, "tok_k4", "single_alive", hstate=True),
    _c("b6_H132_V1000", 6, 132, 1000, 3, "x0_rm", "mixed", maxcol="last"),
    _c("b7_H132_V254", 7, 132, 254, 3, "tok_k4", "mixed", maxcol=64),
    _c("b8_H132_V30_finished", 8, 132, 30, 12, "x0_rm", "all_finished", hstate=True),
    _c("b8_H132_V257", 8, 132, 257, 1, "tok_k4", "mixed"),
    _c("b9_H40_V61", 9, 40, 61, 3, "tok_k4", "mixed"),
    _c("b16_H40_V1000", 16, 40, 1000, 1, "x0_rm", "mixed", hstate=True),
    _c("b16_H40_V257_step1", 16, 40, 257, 3, "tok_k4", "step1"),
    _c("b10_H256_V254_lowered", 10, 256, 254, 1, "tok_k4", "mixed", maxcol="last4"),
    _c("b4_H8_V30_twin_rows", 4, 8, 30, 3, "x0_rm", "alive", tie="rows"),
    _c("b5_H8_V61_twin_cols", 5, 8, 61, 1, "tok_k4", "alive", tie="cols"),
    _c("b3_H100_V30_tok_rm", 3, 100, 30, 3, "tok_rm", "mixed"),
]
BEAM_BY_NAME = {c["name"]: c for c in BEAM_CASES}
BEAM_MUTANTS = ("drop_last_column", "drop_last_kslice", "drop_beam_row", "drop_zh", "ignore_prev_lp", "finished_no_compete",
                "tie_highest", "vlen_on_finished")
STEP_LDS_MAX = 152 * 1024


def step_groups(n4, split):
    g = 64 if n4 <= 64 else 128 if n4 <= 128 else 256
    return max(g, 1024 // split)


def beam_nbm(beam):
    return 4 if beam <= 4 else 5 if beam == 5 else 8 if beam <= 8 else 16


def beam_lds_bytes(H, V, beam, split):
    nbm, Vp = beam_nbm(beam), (V + 3) & ~3
    return (2 * ((nbm + 3) & ~3) * H + (1 + 1024 // step_groups(Vp // 4, split)) * beam * Vp + 16) * 4


def beam_launch(beam, H, V, split_cap=0):
    """the launcher's arithmetic: NBM, the projection split (natural, then capped), KQ partial sums, kn k-values per slice, NLD loads
    in flight, and per slice the number of vector rounds and tail steps"""
    nbm = beam_nbm(beam)
    natural = 16
    while natural > 1 and beam_lds_bytes(H, V, beam, natural) > STEP_LDS_MAX:
        natural >>= 1
    split = min(natural, split_cap) if split_cap else natural
    Vp = (V + 3) & ~3
    KQ = 1024 // step_groups(Vp // 4, split)
    kn = (H + KQ - 1) // KQ
    NLD = 16 if nbm <= 5 else 8 if nbm <= 8 else 2
    slices = []
    for kq in range(KQ):
        k0 = kq * kn
        n = max(min(H, k0 + kn) - k0, 0)
        slices.append(dict(k0=k0, n=n, vec=n // NLD, tail=n % NLD))
    return dict(nbm=nbm, natural=natural, split=split, KQ=KQ, kn=kn, NLD=NLD, slices=slices, lds=beam_lds_bytes(H, V, beam, split))


BEAM_REQUIRED = ({f"NBM{n}" for n in (4, 5, 8, 16)} | {f"KQ{q}" for q in (16, 8, 4)}
                 | {f"NLD{n}_{w}" for n in (16, 8, 2) for w in ("vec", "vec_then_tail")}
                 | {"tail_only", "vec_only", "slice_past_H", "topk_regs", "topk_lds", "rank_readlane", "rank_lds", "V%4==0", "V%4!=0",
                    "lowered_split", "split_cap4", "split_cap1", "B1", "B3", "B12", "tok_k4", "x0_rm", "tok_rm", "hstate", "no_hstate",
                    "max_col0", "max_col63", "max_col64", "max_col_last", "max_col_last4", "step1", "mixed", "all_finished", "eos_wins",
                    "single_alive", "twin_rows", "twin_cols"}
                 | {f"beam{b}" for b in (1, 3, 4, 5, 6, 7, 8, 9, 16)})


def beam_paths(c):
    L = beam_launch(c["beam"], c["H"], c["V"], c["split_cap"])
    p = {f"NBM{L['nbm']}", f"KQ{L['KQ']}", f"beam{c['beam']}", f"B{c['B']}", c["form"], c["state"], "hstate" if c["hstate"] else "no_hstate"}
    for s in L["slices"]:
        if s["k0"] >= c["H"]:
            p.add("slice_past_H")
        if s["vec"]:
            p.add(f"NLD{L['NLD']}_vec")
            p.add(f"NLD{L['NLD']}_vec_then_tail" if s["tail"] else "vec_only")
        elif s["tail"]:
            p.add("tail_only")
    p.add("topk_regs" if c["V"] <= 256 else "topk_lds")
    p.add("rank_readlane" if c["beam"] ** 2 + c["beam"] <= 64 else "rank_lds")
    p.add("V%4==0" if c["V"] % 4 == 0 else "V%4!=0")
    if L["natural"] < 16:
        p.add("lowered_split")
    if c["split_cap"]:
        p.add(f"split_cap{c['split_cap']}")
    if c["maxcol"] is not None:
        p.add(f"max_col{c['maxcol']}" if isinstance(c["maxcol"], int) else f"max_col_{c['maxcol']}")
    if c["tie"]:
        p.add(f"twin_{c['tie']}")
    return p


def length_penalties(step, K=BEAM_K, alpha=BEAM_ALPHA):
    lp = np.float32(np.float32(K + step) ** np.float32(alpha) / np.float32(K + 1) ** np.float32(alpha))
    prev = np.float32(1.0) if step == 1 else np.float32(np.float32(K + step - 1) ** np.float32(alpha) / np.float32(K + 1) ** np.float32(alpha))
    return lp, prev


def last_kslice(H, KQ):
    """the k values of the last non-empty projection slice"""
    kn = (H + KQ - 1) // KQ
    k0 = ((H - 1) // kn) * kn
    return k0, min(H, k0 + kn)


def beam_step(inp, dt=np.float64, mutant=None):
    """One step of the sampler on R = B * beam rows -> dict of
      h, c (R,H) the last cell's new state; out (R,H) what the projection sees; allc (B, beam*V + beam) every candidate's value,
      amag its magnitude; order (B, beam) the winners' indices into allc;
      scores, alive, vlen, par, word (R) the bookkeeping; flag; h_gather, c_gather (R,H) the states by parent; x0, c0cur (x0 form);
      p0 (token form with w1x)."""
    beam, lstm = inp["beam"], inp["lstm"]
    g1 = inp["g1"]
    R, H = inp["hprev"].shape
    B = R // beam
    wp, bp = inp["wp"].astype(dt), inp["bp"].astype(dt)
    V = wp.shape[0]
    one = dt(1.0)
    h, c = cell0(g1, inp["hprev"], inp["c1"] if lstm else None, lstm, dt)
    if mutant == "drop_zh" and not lstm:
        g = g1.astype(dt)
        r, n_i, n_h = 1.0 / (1.0 + np.exp(-g[:, :H])), g[:, 2 * H:3 * H], g[:, 3 * H:]
        z = 1.0 / (1.0 + np.exp(-g[:, H:2 * H]))
        h = ((one - z) * np.tanh(n_i + r * n_h)).astype(dt)
    out = (h + inp["xin"].astype(dt)).astype(dt) if inp["residual"] else h
    proj_in = out.copy()
    if mutant == "drop_beam_row":
        proj_in[beam - 1::beam] = 0
    kk = np.ones(H, dtype=bool)
    if mutant == "drop_last_kslice":
        k0, k1 = last_kslice(H, inp.get("KQ", 16))
        kk[k0:k1] = False
    logits = (proj_in[:, kk] @ wp[:, kk].T + bp[None, :]).astype(dt)
    lmag = np.abs(proj_in[:, kk]) @ np.abs(wp[:, kk]).T + np.abs(bp)[None, :]
    zz = logits[:, :V - 1] if mutant == "drop_last_column" else logits
    mx = zz.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(zz - mx).sum(axis=1, keepdims=True))).astype(dt)
    osc = inp["scores"].astype(dt)
    al = inp["alive"].astype(bool)
    lp = dt(inp["lp"])
    prev_lp = one if mutant == "ignore_prev_lp" else dt(inp["prev_lp"])
    neg = dt(K_NEG)
    cand = ((osc * prev_lp)[:, None] + (logits - lse)) / lp
    cand = np.where(al[:, None], cand, neg).astype(dt)
    cmag = (np.abs(osc * prev_lp)[:, None] + lmag + np.abs(lse)) / lp
    fin = np.where(al, neg, osc).astype(dt)
    if mutant == "finished_no_compete":
        fin = np.full(R, neg, dtype=dt)
    allc = np.concatenate([cand.reshape(B, beam * V), fin.reshape(B, beam)], axis=1)
    amag = np.concatenate([cmag.reshape(B, beam * V), np.abs(osc).reshape(B, beam)], axis=1)
    if mutant == "tie_highest":
        n = allc.shape[1]
        order = (n - 1 - np.argsort(-allc[:, ::-1], axis=1, kind="stable"))[:, :beam]
    else:
        order = np.argsort(-allc, axis=1, kind="stable")[:, :beam]
    scores = np.take_along_axis(allc, order, axis=1)
    use_prev = order >= beam * V
    word = np.where(use_prev, -1, order % V).astype(np.int32)
    bid = np.where(use_prev, order - beam * V, order // V).astype(np.int32)
    flat = (bid + np.arange(B)[:, None] * beam).reshape(-1)
    adv = 1 if mutant == "vlen_on_finished" else 1 - use_prev.astype(np.int32)
    vlen = (inp["vlen"].astype(np.int32)[flat].reshape(B, beam) + adv).astype(np.int32)
    alive = al[flat].reshape(B, beam) & (word != inp["eos"])
    res = dict(h=h, c=c, out=out, allc=allc, amag=amag, order=order, scores=scores.reshape(-1).astype(dt), alive=alive.reshape(-1).astype(np.int32),
               vlen=vlen.reshape(-1), par=bid.reshape(-1), word=word.reshape(-1), flag=int(alive.any()),
               h_gather=h[flat], c_gather=c[flat] if lstm else None, x0=None, c0cur=None, p0=None, p0_mag=None)
    if inp["form"] == "x0_rm":
        emb = inp["emb"][np.maximum(word.reshape(-1), 0)]
        res["x0"] = np.concatenate([emb, inp["ctxv"][flat], inp["h0n"][flat]], axis=1)       # copies: fp32 bits
        res["c0cur"] = inp["c0n"][flat] if lstm else None
    else:
        xa = np.concatenate([inp["xin"], inp["xctx"]], axis=1).astype(dt)
        wa = inp["w1x"][:, :2 * H].astype(dt)
        res["p0"] = (xa @ wa.T + inp["b1x"].astype(dt)[None, :]).astype(dt)
        res["p0_mag"] = np.abs(xa) @ np.abs(wa).T + np.abs(inp["b1x"].astype(dt))[None, :]
    return res


def beam_bars(ref64, ref32):
    """relative bar of the candidates, absolute bars of h and c: from the two evaluations of the reference alone"""
    b = dict(scores=rel_bar(ref64["allc"], ref32["allc"], ref64["amag"]), h=abs_bar(ref64["h"], ref32["h"]))
    if ref64["c"] is not None:
        b["c"] = abs_bar(ref64["c"], ref32["c"])
    if ref64["p0"] is not None:
        b["p0"] = rel_bar(ref64["p0"], ref32["p0"], ref64["p0_mag"])
    return b


def beam_gaps(ref64, bar, beam):
    """per clip, the gaps of float64 between consecutive winners and between the beam-th and the (beam+1)-th candidate, in units of
    the larger neighbour's absolute bar -> (smallest nonzero gap in bars, number of exactly-zero gaps)"""
    allc, amag = ref64["allc"], ref64["amag"]
    top = np.argsort(-allc, axis=1, kind="stable")[:, :beam + 1]
    v, m = np.take_along_axis(allc, top, axis=1), np.take_along_axis(amag, top, axis=1)
    gap = v[:, :-1] - v[:, 1:]
    unit = bar * np.maximum(np.maximum(m[:, :-1], m[:, 1:]), TINY)
    zero = gap == 0
    g = np.where(zero, np.inf, gap / unit)
    return float(g.min()), int(zero.sum())


GAP_BARS = 2.0            # selection and order must equal float64's wherever its gaps exceed this many bars: every case is built so


def beam_compare(got, inp, ref64, ref32):
    """every output of one kernel launch (`got`, keys as beam_step's) against the float64 reference -> {output: (error, bar)}; integer
    outputs and bit copies carry bar 0 (any difference is an error).  The kernel's own (parent, word) picks the float64 value each
    score is compared with; selection and order themselves are compared with float64's (the gaps are asserted beforehand)."""
    beam, lstm = inp["beam"], inp["lstm"]
    R, H = inp["hprev"].shape
    B, V = R // beam, inp["wp"].shape[0]
    bars = beam_bars(ref64, ref32)
    res = {}
    par, word = np.asarray(got["par"]).astype(np.int64), np.asarray(got["word"]).astype(np.int64)
    ok = (par >= 0) & (par < beam) & (word >= -1) & (word < V)
    res["selection_valid"] = (float((~ok).sum()), 0.0)
    par_c, word_c = np.clip(par, 0, beam - 1), np.clip(word, -1, V - 1)
    idx = np.where(word_c < 0, beam * V + par_c, par_c * V + word_c).reshape(B, beam)
    val, mag = np.take_along_axis(ref64["allc"], idx, axis=1).reshape(-1), np.take_along_axis(ref64["amag"], idx, axis=1).reshape(-1)
    res["scores"] = (rel_err(got["scores"], val, mag), bars["scores"])
    for k in ("par", "word", "alive", "vlen"):
        res[k] = (float((np.asarray(got[k]).astype(np.int64) != ref64[k]).sum()), 0.0)
    res["flag"] = (float(int(got["flag"]) != ref64["flag"]), 0.0)
    if got.get("parent_out") is not None:
        res["parent_out"] = (float((np.asarray(got["parent_out"]) != ref64["par"]).sum()), 0.0)
    if got.get("tok") is not None:
        res["tok"] = (float((np.asarray(got["tok"]) != ref64["word"]).sum()), 0.0)
    flat = (par_c + np.repeat(np.arange(B), beam) * beam)
    res["h_gather"] = (float(np.abs(got["h_gather"] - ref64["h"][flat]).max()), bars["h"])
    if got.get("hstate") is not None:
        res["hstate"] = (float(np.abs(got["hstate"] - ref64["h"]).max()), bars["h"])
    if lstm:
        res["c_gather"] = (float(np.abs(got["c_gather"] - ref64["c"][flat]).max()), bars["c"])
    if inp["form"] == "x0_rm":
        want = np.concatenate([inp["emb"][np.maximum(word_c, 0)], inp["ctxv"][flat], inp["h0n"][flat]], axis=1)
        res["x0"] = (float((np.asarray(got["x0"], dtype=np.float32).view(np.uint32) != want.view(np.uint32)).sum()), 0.0)
        if lstm:
            res["c0cur"] = (float((np.asarray(got["c0cur"], dtype=np.float32).view(np.uint32) != inp["c0n"][flat].view(np.uint32)).sum()), 0.0)
    elif got.get("p0") is not None:
        res["p0"] = (rel_err(got["p0"], ref64["p0"], ref64["p0_mag"]), bars["p0"])
    return res


def ratio(e, b):
    """error in bars; an output with bar 0 is infinitely far once it differs at all"""
    return (float("inf") if e > 0 else 0.0) if b == 0 else e / b


def as_got(res, inp):
    """a reference evaluation in the shape of a kernel's outputs (what beam_compare takes)"""
    g = {k: res[k] for k in ("scores", "alive", "vlen", "par", "word", "flag", "h_gather", "c_gather", "x0", "c0cur", "p0")}
    g["parent_out"], g["tok"], g["hstate"] = res["par"], res["word"], res["h"] if inp["residual"] else None
    return g


def beam_mutant_applies(mutant, c, cell):
    st = c["state"]
    if mutant in ("drop_last_column", "drop_last_kslice"):
        return st != "all_finished"
    if mutant == "drop_beam_row":       # row beam - 1 must be alive and in the running
        return st not in ("all_finished", "step1") and c["tie"] != "rows"     # (behind the twins its candidates do not win)
    if mutant == "drop_zh":
        return cell == "gru" and st != "all_finished"
    if mutant == "ignore_prev_lp":
        return st not in ("all_finished", "step1")
    if mutant in ("finished_no_compete", "vlen_on_finished"):
        return st in ("mixed", "single_alive", "all_finished") and c["beam"] > 1
    if mutant == "tie_highest":
        return c["tie"] is not None
    raise KeyError(mutant)


def _finished_rows(c):
    beam, st = c["beam"], c["state"]
    if st == "mixed":
        return [r for r in range(beam) if r % 3 == 1 and r != beam - 1]
    if st == "single_alive":
        return list(range(beam - 1))
    if st == "all_finished":
        return list(range(beam))
    return []


def _build(c, cell, seed):
    beam, H, V, B = c["beam"], c["H"], c["V"], c["B"]
    R, lstm = B * beam, cell == "lstm"
    rng = np.random.default_rng(7919 * seed + 31 * H + V + 1000 * beam + (1 if lstm else 0))
    f = lambda *shape, s=1.0: (s * rng.standard_normal(shape)).astype(np.float32)
    step = 1 if c["state"] == "step1" else BEAM_STEP
    lp, prev_lp = length_penalties(step)
    eos = 2
    L = beam_launch(beam, H, V, c["split_cap"])
    inp = dict(beam=beam, lstm=lstm, residual=c["hstate"], form=c["form"], step=step, lp=lp, prev_lp=prev_lp, eos=eos, KQ=L["KQ"],
               g1=f(R, 4 * H), hprev=f(R, H, s=0.5), c1=f(R, H), xin=f(R, H, s=0.5), xctx=f(R, H, s=0.5),
               wp=f(V, H, s=PROJ_SCALE / np.sqrt(H)), bp=f(V, s=0.3))
    if c["form"] == "x0_rm":
        inp.update(emb=f(V, BEAM_E), ctxv=f(R, H), h0n=f(R, H), c0n=f(R, H))
    else:
        inp.update(K1p=3 * H + 16, w1x=f(4 * H, 3 * H + 16, s=1.0 / np.sqrt(2 * H)), b1x=f(4 * H, s=0.3))
    if c["maxcol"] is not None:
        col = {"last": V - 1, "last4": ((V + 3) & ~3) - 4}.get(c["maxcol"], c["maxcol"])
        inp["bp"][col] += 6.0
        inp["maxcol"] = col
    if c["state"] == "eos_wins":
        inp["bp"][eos] += 2.5           # ahead in its row, not so far that every winner ends
    if c["tie"] == "cols":          # columns 5 and 40: another lane, another float4; both ahead of the rest
        inp["wp"][40], inp["bp"][40] = inp["wp"][5], inp["bp"][5]
        inp["bp"][[5, 40]] += 4.0
    fin_rows = _finished_rows(c)
    alive = np.ones((B, beam), dtype=np.int32)
    alive[:, fin_rows] = 0
    if c["state"] == "step1":
        scores = np.full((B, beam), K_NEG, dtype=np.float32)
        scores[:, 0] = 0.0
        vlen = np.ones((B, beam), dtype=np.int32)
    else:
        scores = np.sort(rng.uniform(-4.0, -2.0, (B, beam)), axis=1).astype(np.float32)       # ascending: row beam - 1 leads the clip
        vlen = rng.integers(2, 8, (B, beam)).astype(np.int32)
    if c["state"] == "all_finished":
        scores = rng.permuted(scores, axis=1)
    if c["tie"] == "rows":          # rows 1 and 2 of every clip are one hypothesis twice, ahead of the others
        for k in ("g1", "hprev", "c1", "xin", "xctx"):
            a = inp[k].reshape(B, beam, -1)
            a[:, 2] = a[:, 1]
        scores[:, 1] = scores[:, 2] = scores[:, beam - 1] + np.float32(1.0)
    inp.update(scores=scores.reshape(-1), alive=alive.reshape(-1), vlen=vlen.reshape(-1))
    if fin_rows and c["state"] != "all_finished":
        # a finished beam competes with its own score: put the j-th one between the alive candidates of rank 2j and 2j + 1 (the
        # first two of a single alive row's companions; the others far below)
        inp["scores"].reshape(B, beam)[:, fin_rows] = -100.0
        cand = np.sort(beam_step(inp)["allc"][:, :beam * V], axis=1)[:, ::-1]
        for j, r in enumerate(fin_rows):
            v = 0.5 * (cand[:, 2 * j] + cand[:, 2 * j + 1]) if j < 2 or c["state"] == "mixed" else -50.0 - j
            inp["scores"].reshape(B, beam)[:, r] = np.asarray(v, dtype=np.float32)
    return inp


SEED_TRIES = 40


@functools.lru_cache(maxsize=None)
def beam_inputs(name, cell):
    """-> (inputs, float64 reference, float32 evaluation, seed): the first seed at which every gap of float64 between consecutive
    winners and behind the last one clears GAP_BARS bars with room to spare (3x), chosen here, on the CPU, from the reference alone"""
    c = BEAM_BY_NAME[name]
    for seed in range(SEED_TRIES):
        inp = _build(c, cell, seed)
        r64, r32 = beam_step(inp), beam_step(inp, np.float32)
        g, zeros = beam_gaps(r64, beam_bars(r64, r32)["scores"], c["beam"])
        if g > 3 * GAP_BARS and (zeros > 0) == (c["tie"] is not None):
            return inp, r64, r32, seed
    raise AssertionError(f"{name} {cell}: no seed below {SEED_TRIES} separates the winners")
