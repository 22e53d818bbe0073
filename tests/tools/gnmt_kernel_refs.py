"""Shapes, input recipes and plain NumPy references for the captioner's step kernels on their own (tests only): what
tests/test_cpu_gnmt_kernel_refs.py checks on the CPU and tests/test_gpu_gnmt_kernels.py runs through the tn_dbg_gnmt_* hooks.

Five operations of tennis_amd/csrc/gnmt_kernels.hip, each written once and evaluated in float64 (the reference) and in float32 (the
same formula, whose distance from the float64 result sets the bar, see ``bar``):
  attention_fwd    first decoder cell on stacked pre-activations + scaled-Luong attention (dec_attention_kernel<1>)
  attention_bwd    ds, dctx, dh0 of one decoder step's attention                            (trn_att_bwd_kernel)
  attention_outer  d mem and d keyproj summed over the decoder steps                        (trn_att_outer_kernel)
  ce               gradient and value of the token-averaged masked cross-entropy, and the per-sample masked loss
                                                                                            (trn_ce_bwd_kernel, masked_ce_kernel)
  emb_grad         rows of the step-major input gradients summed per token                  (trn_emb_grad_kernel)

Every reference takes ``mutant``: a deliberate defect of the kind a kernel's loop bounds produce (a source step lost, one too many
let in, a decoder step lost, a vocabulary column lost).  A test that cannot tell a mutant from the true reference at its bar
cannot fail, so the CPU test asserts that every mutant is at least 10 bars away.

Error metrics (``err``): a contraction's error is measured per element against the sum of the absolute values of that element's
terms, fully expanded (for ds_s = w_s (dw_s - sum_s' w_s' dw_s') these are the products w_s mem_sh dctx_h and w_s w_s' mem_s'h dctx_h;
dh0 inherits them through |kp|) - the convention of tests/test_gpu_train_kernels.py; weights, cell states, dlogits and losses are
measured absolutely."""
from __future__ import annotations

import functools

import numpy as np

GEMM_TOL = 1e-6        # the project's bar for an fp32 contraction against the magnitude of its terms (test_gpu_train_kernels.py)
MARGIN = 16            # bar = max(floor, MARGIN * n), n the error of the float32 NumPy evaluation of the same formula: covers a
#                        different summation order (16 partial sums, fma chains) and the device's expf / tanhf
MUTANT_FACTOR = 10     # every mutant must sit at least this many bars from the true reference

# ---- attention cases ---------------------------------------------------------------------------------------------------------------
# (name, T, H, valid_len per clip, cells the forward hook runs, target score spread): the smallest shapes at which each loop of the
# two attention kernels takes its other path
ATT_CASES = [
    ("T5_H8", 5, 8, (5, 1, 3), ("gru", "lstm"), 1.5),                  # Tp padding; fewer units than the 16 H-slices
    ("T129_H20", 129, 20, (129, 128, 2), ("gru", "lstm"), 1.5),        # second s0 round; H % 16 tail
    ("T214_H64", 214, 64, (214, 160, 1), ("gru", "lstm"), 1.5),        # the config-C5 length
    ("T260_H256", 260, 256, (260, 241, 256), ("gru", "lstm"), 1.5),    # CG = 128; full 16-step chunks; H-slice of exactly 16
    ("T520_H260", 520, 260, (520, 519, 257), ("gru", "lstm"), 1.5),    # CG = 256; H-slice 16 + 1; U4 = 65: 128 column groups, SG = 8
    ("T1030_H8", 1030, 8, (1030, 1025, 1024), ("gru", "lstm"), 1.5),   # second round of every 1024-stride loop
    ("T300_H680", 300, 680, (300, 257), ("gru",), 1.5),                # 256 column groups, SG = 4; the widest GRU the handles accept
    ("T300_H512", 300, 512, (300, 257), ("lstm",), 1.5),               # the widest LSTM
    ("T214_H64_saturated", 214, 64, (214, 160, 1), ("gru",), 30.0),    # one-hot attention: finiteness and float64 only
]
ATT_BY_NAME = {c[0]: c for c in ATT_CASES}
SPLIT_CAP_CASES = [("T214_H64", 4), ("T214_H64", 1), ("T260_H256", 4), ("T260_H256", 1)]
BEAM_CASE = dict(T=21, H=32, beam=5, clips=12)       # eight clips go through the XCD row mapping, four sit behind it
OUTER_CASES = [(steps, T, H) for steps in (1, 40) for (T, H) in ((5, 8), (214, 64), (302, 260), (31, 680))]
FWD_MUTANTS = ("drop_last", "drop_128", "extra_step")
BWD_MUTANTS = ("drop_last", "drop_128", "extra_step", "drop_dq16")
OUTER_MUTANTS = ("drop_last", "drop_128", "drop_last_decoder_step")

CE_CASES = [(V, L) for V in (3, 254, 256, 257, 300, 1000) for L in (1, 7)]
CE_B = 4
EMB_CASES = [(E, V) for E in (6, 64, 65, 100) for V in (14, 300)]


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def is_saturated(name):
    return name.endswith("saturated")


# ---- attention forward ------------------------------------------------------------------------------------------------------------

def cell0(g0, hprev, cprev, lstm, dt):
    """the first decoder cell on its stacked pre-activations g0 (R,4H): GRU [r, z, n_i2h, n_h2h], LSTM [i, f, g, o] -> (h, c | None)"""
    g0, hprev = g0.astype(dt), hprev.astype(dt)
    H = hprev.shape[1]
    a, b, c, d = (g0[:, i * H:(i + 1) * H] for i in range(4))
    one = dt(1.0)
    if lstm:
        c2 = _sig(b) * cprev.astype(dt) + _sig(a) * np.tanh(c)
        return (_sig(d) * np.tanh(c2)).astype(dt), c2.astype(dt)
    r, z = _sig(a), _sig(b)
    n = np.tanh(c + r * d)
    return ((one - z) * n + z * hprev).astype(dt), None


def clamp_len(vl, T):
    return np.minimum(np.maximum(np.asarray(vl, dtype=np.int64), 0), T)


def _steps(v, T, mutant):
    """the source steps a (possibly defective) softmax / contraction walks for a clip of valid length v"""
    idx = np.arange(v)
    if mutant == "drop_last" and v >= 2:
        idx = idx[:-1]
    elif mutant == "drop_128" and v > 128:
        idx = idx[idx != 128]
    elif mutant == "extra_step" and v < T and v >= 1:
        idx = np.arange(v + 1)
    return idx


def attention_fwd(inp, dt=np.float64, mutant=None):
    """-> dict(h, c, w (R,T), ctx (R,H), ctx_mag (R,H), scores: list per row over its valid steps)"""
    lstm = inp["lstm"]
    h, c = cell0(inp["g0"], inp["hprev"], inp["cprev"] if lstm else None, lstm, dt)
    R, H = h.shape
    B, T, _ = inp["mem"].shape
    beam = R // B
    vl = clamp_len(inp["valid_len"], T)
    q = h * (dt(1.0) / np.sqrt(dt(H)))
    kp, mem = inp["keyproj"].astype(dt), inp["mem"].astype(dt)
    w = np.zeros((R, T), dtype=dt)
    ctx = np.zeros((R, H), dtype=dt)
    mag = np.zeros((R, H), dtype=dt)
    scores = []
    for r in range(R):
        b = r // beam
        idx = _steps(int(vl[b]), T, mutant)
        if idx.size == 0:
            scores.append(np.zeros(0, dtype=dt))
            continue
        s = kp[b, idx] @ q[r]
        e = np.exp(s - s.max())
        wr = (e / e.sum()).astype(dt)
        w[r, idx] = wr
        ctx[r] = wr @ mem[b, idx]
        mag[r] = wr @ np.abs(mem[b, idx])
        scores.append(s)
    return dict(h=h, c=c, w=w, ctx=ctx, ctx_mag=mag, scores=scores)


def score_spread(scores, min_steps=2):
    """standard deviation of each row's scores over its valid steps (rows with fewer than min_steps steps carry no statistic)"""
    return [float(np.std(s)) for s in scores if s.size >= min_steps]


@functools.lru_cache(maxsize=None)
def attention_inputs(T, H, valid_len, lstm, spread, beam=1, seed=0):
    """seeded N(0,1) operands; the key projection of every clip is scaled so that the float64 scores of the clip's rows spread by
    `spread` (their mean standard deviation over the valid steps; a clip of one step takes the longest clip's scale)"""
    B = len(valid_len)
    R = B * beam
    rng = np.random.default_rng(1000 * T + H + 7 * seed + (1 if lstm else 0))
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    inp = dict(g0=f(R, 4 * H), hprev=f(R, H), cprev=f(R, H), mem=f(B, T, H), keyproj=f(B, T, H),
               valid_len=np.asarray(valid_len, dtype=np.int32), lstm=bool(lstm))
    ref = attention_fwd(inp)
    vl = clamp_len(valid_len, T)
    scale = np.ones(B)
    for b in range(B):
        sds = [np.std(ref["scores"][r]) for r in range(b * beam, (b + 1) * beam) if ref["scores"][r].size >= 2]
        scale[b] = spread / np.mean(sds) if sds else np.nan
    scale[np.isnan(scale)] = scale[int(np.argmax(vl))]
    inp["keyproj"] = (inp["keyproj"] * scale[:, None, None]).astype(np.float32)
    return inp


def beam_valid_len():
    """the beam case's 12 clips: the full length first, then lengths from 16 (every row keeps a score statistic) to T"""
    c = BEAM_CASE
    vl = np.random.default_rng(12).integers(16, c["T"] + 1, c["clips"]).astype(np.int32)
    vl[0] = c["T"]
    return vl


def case_inputs(name, cell, beam=1):
    _, T, H, vl, _, spread = ATT_BY_NAME[name]
    return attention_inputs(T, H, tuple(vl), cell == "lstm", spread, beam)


# ---- attention backward -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def attention_bwd_inputs(name):
    """the weights of the case's forward (float64 reference rounded to fp32) with its memory and key projection, and two N(0,1)
    addends of d context at pitches H + 4 and 2 H + 8.  Past valid_len the weights are set to 0.01, not to the 0 the forward kernel
    leaves there: the backward kernel masks by valid_len itself, and a step it let in must show."""
    _, T, H, vl, cells, _ = ATT_BY_NAME[name]
    fin = case_inputs(name, cells[0])
    aw = attention_fwd(fin)["w"].astype(np.float32)
    B = len(vl)
    for b in range(B):
        aw[b, int(clamp_len(vl[b], T)):] = 0.01
    rng = np.random.default_rng(77 + T + H)
    c0 = rng.standard_normal((B, H + 4)).astype(np.float32)
    c1 = rng.standard_normal((B, 2 * H + 8)).astype(np.float32)
    return dict(aw=aw, mem=fin["mem"], keyproj=fin["keyproj"], c0=c0, c1=c1, valid_len=fin["valid_len"])


def attention_bwd(inp, dt=np.float64, mutant=None, use_c0=True, use_c1=True):
    """-> dict(ds (B,T), dctx (B,H), dh0 (B,H)) and the magnitudes ds_mag, dctx_mag, dh0_mag of their terms"""
    aw, mem, kp = inp["aw"].astype(dt), inp["mem"].astype(dt), inp["keyproj"].astype(dt)
    B, T, H = mem.shape
    vl = clamp_len(inp["valid_len"], T)
    z = np.zeros((B, H), dtype=dt)
    a0 = inp["c0"][:, :H].astype(dt) if use_c0 else z
    a1 = inp["c1"][:, :H].astype(dt) if use_c1 else z
    dctx = a0 + a1
    out = dict(dctx=dctx, dctx_mag=np.abs(a0) + np.abs(a1), ds=np.zeros((B, T), dtype=dt), ds_mag=np.zeros((B, T), dtype=dt),
               dh0=np.zeros((B, H), dtype=dt), dh0_mag=np.zeros((B, H), dtype=dt))
    inv = dt(1.0) / np.sqrt(dt(H))
    for b in range(B):
        idx = _steps(int(vl[b]), T, mutant)
        if idx.size == 0:
            continue
        w = aw[b, idx]
        dw = mem[b, idx] @ dctx[b]
        dwm = np.abs(mem[b, idx]) @ np.abs(dctx[b])
        ds = w * (dw - w @ dw)
        dsm = np.abs(w) * (dwm + np.abs(w) @ dwm)
        out["ds"][b, idx], out["ds_mag"][b, idx] = ds, dsm
        k = max(idx.size - 16, 0) if mutant == "drop_dq16" else idx.size
        out["dh0"][b] = (ds[:k] @ kp[b, idx[:k]]) * inv
        out["dh0_mag"][b] = (dsm[:k] @ np.abs(kp[b, idx[:k]])) * inv
    return out


# ---- attention outer products -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def attention_outer_inputs(steps, T, H, B=3):
    rng = np.random.default_rng(5000 + 100 * steps + T + H)
    s = rng.standard_normal((steps, B, T)) * 1.5
    e = np.exp(s - s.max(axis=2, keepdims=True))
    aw = (e / e.sum(axis=2, keepdims=True)).astype(np.float32)
    ds = (aw * rng.standard_normal((steps, B, T))).astype(np.float32)
    dctx = rng.standard_normal((steps, B, H)).astype(np.float32)
    h0 = rng.standard_normal((steps, B, H + 12)).astype(np.float32)        # pitch H + 12
    return dict(aw=aw, ds=ds, dctx=dctx, h0=h0)


def attention_outer(inp, dt=np.float64, mutant=None):
    """-> dict(dmem, dkp (B,T,H), dmem_mag, dkp_mag)"""
    aw, ds, dctx = inp["aw"].astype(dt), inp["ds"].astype(dt), inp["dctx"].astype(dt)
    steps, B, T = aw.shape
    H = dctx.shape[2]
    h0 = inp["h0"][:, :, :H].astype(dt)
    if mutant == "drop_last_decoder_step":
        aw, ds, dctx, h0 = aw[:-1], ds[:-1], dctx[:-1], h0[:-1]
    dsi = ds * (dt(1.0) / np.sqrt(dt(H)))
    out = dict(dmem=np.einsum("lbt,lbh->bth", aw, dctx), dkp=np.einsum("lbt,lbh->bth", dsi, h0),
               dmem_mag=np.einsum("lbt,lbh->bth", np.abs(aw), np.abs(dctx)), dkp_mag=np.einsum("lbt,lbh->bth", np.abs(dsi), np.abs(h0)))
    row = T - 1 if mutant == "drop_last" else 128 if mutant == "drop_128" and T > 128 else None
    if row is not None:
        out["dmem"][:, row], out["dkp"][:, row] = 0, 0
    return {k: v.astype(dt) for k, v in out.items()}


# ---- cross-entropy ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ce_inputs(V, L, all_masked=False):
    """logits N(0,3) (B,L,V); rows (0, 0) and (1, 0) shifted by +100 (a kernel that forgot the maximum overflows); row (3, L-1) has
    its maximum in the last column (>= 256 once V > 256); row (0, L-1) has its label at V - 1; labels at pitch L + 3"""
    B = CE_B
    rng = np.random.default_rng(31 * V + L)
    z = (3.0 * rng.standard_normal((B, L, V))).astype(np.float32)
    z[0, 0] += 100.0
    z[1, 0] += 100.0
    z[3, L - 1, V - 1] = z[3, L - 1].max() + 6.0
    labels = rng.integers(0, V, (B, L + 3)).astype(np.int32)
    labels[0, L - 1] = V - 1
    vl = np.zeros(B, dtype=np.int32) if all_masked else np.array([L, 0, 1, L + 3], dtype=np.int32)
    return dict(logits=z, labels=labels, valid_len=vl)


def ce(inp, dt=np.float64, mutant=None):
    """-> dict(dlogits (L,B,V), loss_rows (L,B), loss, masked_loss (B)); mutant "drop_last_column": the log-sum-exp misses column V-1"""
    z = inp["logits"].astype(dt)
    B, L, V = z.shape
    lab = inp["labels"][:, :L].astype(np.int64)
    vl = inp["valid_len"].astype(np.int64)
    ntok = int(clamp_len(vl, L).sum())
    zz = z[:, :, :V - 1] if mutant == "drop_last_column" and V > 1 else z
    mx = zz.max(axis=2, keepdims=True)
    lse = (mx + np.log(np.exp(zz - mx).sum(axis=2, keepdims=True))).astype(dt)
    valid = np.arange(L)[None, :] < vl[:, None]                                     # (B, L)
    sc = (valid.astype(dt) / dt(ntok)) if ntok > 0 else np.zeros((B, L), dtype=dt)
    p = np.exp(z - lse)
    onehot = np.zeros((B, L, V), dtype=dt)
    np.put_along_axis(onehot, lab[:, :, None], 1.0, axis=2)
    nll = lse[:, :, 0] - np.take_along_axis(z, lab[:, :, None], axis=2)[:, :, 0]
    loss_rows = np.where(valid, nll * sc, 0).astype(dt)
    masked = (np.where(valid, nll, 0).sum(axis=1) / dt(L)).astype(dt)
    return dict(dlogits=np.transpose((p - onehot) * sc[:, :, None], (1, 0, 2)).astype(dt), loss_rows=loss_rows.T.copy(),
                loss=loss_rows.sum(dtype=dt), masked_loss=masked)


# ---- embedding gradient -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def emb_inputs(E, V, L=5, B=4):
    """dx0 (L,B,K0 = E + 5) N(0,1); tokens (B, L + 2) drawn from {-1, 0, 3, 3, 5, V - 1}: ids 0 and -1 (both row 0), repeats, and
    every other row of the vocabulary unused"""
    rng = np.random.default_rng(9 * E + V)
    dx0 = rng.standard_normal((L, B, E + 5)).astype(np.float32)
    pool = np.array([-1, 0, 3, 3, 5, V - 1], dtype=np.int32)
    tgt = pool[rng.integers(0, pool.size, (B, L + 2))]
    tgt[0, 0], tgt[1, 0], tgt[2, 1], tgt[3, 1] = 0, -1, 3, 3
    return dict(dx0=dx0, tgt=tgt, E=E, V=V, L=L, B=B)


def emb_grad(inp, dt=np.float64):
    """-> dict(demb (V,E), demb_mag)"""
    E, V, L, B = inp["E"], inp["V"], inp["L"], inp["B"]
    dx = inp["dx0"][:, :, :E].astype(dt)
    demb, mag = np.zeros((V, E), dtype=dt), np.zeros((V, E), dtype=dt)
    for i in range(L):
        for b in range(B):
            v = max(int(inp["tgt"][b, i]), 0)
            if v < V:
                demb[v] += dx[i, b]
                mag[v] += np.abs(dx[i, b])
    return dict(demb=demb, demb_mag=mag)


# ---- metrics and bars -------------------------------------------------------------------------------------------------------------
# output -> the key of its magnitude (a contraction) or None (absolute error)
METRIC = dict(h=None, c=None, w=None, ctx="ctx_mag", ds="ds_mag", dctx="dctx_mag", dh0="dh0_mag", dmem="dmem_mag", dkp="dkp_mag",
              dlogits=None, loss_rows=None, loss=None, masked_loss=None, demb="demb_mag")


TINY = 1e-30           # a magnitude below this is measured against this: fp32 holds products of weights under 1.2e-38 (one-hot
#                        attention) as denormals with fewer than 24 bits, which no relative bar can ask of them


def err(key, got, ref):
    """worst error of `got` against the float64 reference dict `ref` in the output's metric; where a contraction has no terms at
    all (magnitude 0) the value must be exactly 0"""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
    d = np.abs(g - r)
    if METRIC[key] is None:
        return float(d.max()) if d.size else 0.0
    m = np.asarray(ref[METRIC[key]], dtype=np.float64)
    if (d[m == 0] != 0).any():
        return float("inf")
    return float((d[m > 0] / np.maximum(m[m > 0], TINY)).max()) if (m > 0).any() else 0.0


def floor(key, ref):
    """GEMM_TOL of the magnitude: of the terms for a contraction (the metric is already relative), of the output's largest value
    for an absolute error"""
    if METRIC[key] is not None:
        return GEMM_TOL
    return GEMM_TOL * float(np.abs(np.asarray(ref[key], dtype=np.float64)).max())


def bar(key, ref64, ref32, margin=MARGIN):
    """max(floor, margin * n), n the error of the float32 evaluation of the reference formula: from the reference alone"""
    return max(floor(key, ref64), margin * err(key, ref32[key], ref64))
