"""-m gpu: the captioner's attention and loss kernels (tennis_amd/csrc/gnmt_kernels.hip) on their own, against NumPy float64.

Through the tn_dbg_gnmt_* hooks of include/tennis_hip_debug.h, which launch the production kernels with the production grid, block
and LDS: dec_attention_kernel<1> behind transpose_bth_kernel, trn_att_bwd_kernel, trn_att_outer_kernel, trn_ce_bwd_kernel +
masked_ce_kernel, trn_emb_grad_kernel.  Shapes, input recipes, references, metrics and bars are tests/tools/gnmt_kernel_refs.py's
(checked on the CPU by tests/test_cpu_gnmt_kernel_refs.py, which also shows that a kernel losing one source step, one decoder step
or one vocabulary column would miss these bars by a factor of 100 or more).  A bar is max(1e-6 of the magnitude, 16 x the error of
the float32 NumPy evaluation of the reference formula): it is computed from the reference alone.  Every output is pre-filled with
a sentinel inside a guarded buffer, so that a store outside the output shows.  The measured errors go to the session report."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tools import gnmt_kernel_refs as KR

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64            # floats of sentinel on either side of every output


def _lib():
    from tennis_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx():
    return _lib().default_context()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Out:
    """an output of `shape` (rows of pitch `ld` >= shape[-1]) inside a sentinel-filled buffer"""

    def __init__(self, *shape, ld=None):
        self.shape, self.ld = shape, ld or shape[-1]
        self.rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        self.buf = torch.full((2 * GUARD + self.rows * self.ld,), SENTINEL, dtype=torch.float32, device="cuda")

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def read(self, written_cols=None):
        """the written columns as an array of `shape`; everything else in the buffer must still be the sentinel"""
        a = self.buf.cpu().numpy()
        body = a[GUARD:-GUARD].reshape(self.rows, self.ld)
        n = written_cols or self.shape[-1]
        assert (a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all(), "bytes around the output were written"
        assert (body[:, n:] == SENTINEL).all(), "columns between the rows of a strided output were written"
        return body[:, :n].reshape(self.shape[:-1] + (n,)).copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(report, tag, key, got, ref64, ref32):
    assert np.isfinite(got).all(), (tag, key)
    e, b = KR.err(key, got, ref64), KR.bar(key, ref64, ref32)
    report[f"gnmt_kernels_{tag}_{key}"] = [e, b]
    print(f"{tag} {key}: err {e:.3e} bar {b:.3e}")
    return (tag, key, e, b) if not e <= b else None


def _assert_all(fails):
    fails = [f for f in fails if f]
    assert not fails, fails


# ---- references, computed once per case --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fwd_refs(name, cell):
    inp = KR.case_inputs(name, cell)
    return inp, KR.attention_fwd(inp), KR.attention_fwd(inp, np.float32)


@functools.lru_cache(maxsize=None)
def _bwd_refs(name, use_c0, use_c1):
    inp = KR.attention_bwd_inputs(name)
    return inp, KR.attention_bwd(inp, use_c0=use_c0, use_c1=use_c1), KR.attention_bwd(inp, np.float32, use_c0=use_c0, use_c1=use_c1)


# ---- attention forward ------------------------------------------------------------------------------------------------------------

def _run_fwd(ctx, inp, beam=1, split_cap=0, valid_len=None):
    """one tn_dbg_gnmt_attention_fwd call -> dict(h, c, w, ctx); hprev at pitch H + 4, x1 at pitch 3 H"""
    L = _lib()
    B, T, H = inp["mem"].shape
    R = B * beam
    lstm = inp["lstm"]
    hp = np.full((R, H + 4), 7.0, dtype=np.float32)
    hp[:, :H] = inp["hprev"]
    d = [_dev(inp["g0"]), _dev(hp), _dev(inp["cprev"]) if lstm else None, _dev(inp["keyproj"]), _dev(inp["mem"]),
         _dev(np.asarray(inp["valid_len"] if valid_len is None else valid_len, dtype=np.int32))]
    hn, cn, x1, cx, w = Out(R, H), Out(R, H), Out(R, 3 * H), Out(R, H), Out(R, T)
    L.check(ctx.lib.tn_dbg_gnmt_attention_fwd(ctx.handle, L.ptr(d[0]), L.ptr(d[1]), H + 4, L.ptr(d[2]), 1 if lstm else 0, L.ptr(d[3]),
                                              L.ptr(d[4]), L.ptr(d[5]), B, T, H, beam, split_cap, hn.ptr, cn.ptr if lstm else None,
                                              x1.ptr, 3 * H, cx.ptr, w.ptr), "tn_dbg_gnmt_attention_fwd")
    out = dict(h=hn.read(), ctx=cx.read(), w=w.read(), c=cn.read() if lstm else None)
    x = x1.read(written_cols=2 * H)
    assert np.array_equal(_bits(x[:, :H]), _bits(out["h"])) and np.array_equal(_bits(x[:, H:]), _bits(out["ctx"])), "x1 != [h, ctx]"
    if not lstm:
        assert (cn.buf == SENTINEL).all(), "the GRU form wrote a cell state"
    return out


def _check_fwd(report, tag, got, inp, ref64, ref32, beam=1):
    T = inp["mem"].shape[1]
    vl = np.repeat(KR.clamp_len(inp["valid_len"], T), beam)
    for r, v in enumerate(vl):
        assert not got["w"][r, v:].any(), (tag, "weights past valid_len", r)
    _assert_all(_check(report, tag, k, got[k], ref64, ref32) for k in ("h", "c", "w", "ctx") if ref64[k] is not None)


FWD_PARAMS = [(c[0], cell) for c in KR.ATT_CASES for cell in c[4]]


@pytest.mark.parametrize("name,cell", FWD_PARAMS, ids=[f"{n}-{c}" for n, c in FWD_PARAMS])
def test_attention_forward(ctx, report, name, cell):
    inp, ref64, ref32 = _fwd_refs(name, cell)
    got = _run_fwd(ctx, inp)
    again = _run_fwd(ctx, inp)
    for k in ("h", "w", "ctx"):
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, "not bit-identical on a repeated call")
    _check_fwd(report, f"fwd_{name}_{cell}", got, inp, ref64, ref32)


@pytest.mark.parametrize("name,cap", KR.SPLIT_CAP_CASES)
def test_attention_forward_capped_split(ctx, report, name, cap):
    """fewer partial sums per score and per context unit (what the host picks when 16 partial rows do not fit the LDS)"""
    inp, ref64, ref32 = _fwd_refs(name, "gru")
    _check_fwd(report, f"fwd_{name}_split{cap}", _run_fwd(ctx, inp, split_cap=cap), inp, ref64, ref32)


def test_attention_forward_beam_rows(ctx, report):
    """beam 5 x 12 clips: rows of the first eight clips are dealt to workgroups through the XCD mapping, four clips sit behind it"""
    c = KR.BEAM_CASE
    inp = KR.attention_inputs(c["T"], c["H"], tuple(int(v) for v in KR.beam_valid_len()), False, 1.5, c["beam"])
    got = _run_fwd(ctx, inp, beam=c["beam"])
    _check_fwd(report, "fwd_beam5x12", got, inp, KR.attention_fwd(inp), KR.attention_fwd(inp, np.float32), beam=c["beam"])


@pytest.mark.parametrize("name", ["T5_H8", "T129_H20"])
def test_attention_valid_len_is_clamped(ctx, name):
    """valid_len of T + 7 gives the bits of T; 0 and -3 give weights, context, ds and dh0 that are exactly zero"""
    inp, _, _ = _fwd_refs(name, "gru")
    B, T, H = inp["mem"].shape
    full = _run_fwd(ctx, inp, valid_len=[T] * B)
    over = _run_fwd(ctx, inp, valid_len=[T + 7] * B)
    for k in ("h", "w", "ctx"):
        assert np.array_equal(_bits(full[k]), _bits(over[k])), k
    none = _run_fwd(ctx, inp, valid_len=[0, -3, T][:B] + [0] * (B - 3))
    assert np.isfinite(none["w"]).all() and np.isfinite(none["ctx"]).all()
    assert not none["w"][:2].any() and not none["ctx"][:2].any()
    assert np.array_equal(_bits(none["w"][2]), _bits(full["w"][2])) and np.array_equal(_bits(none["h"]), _bits(full["h"]))
    binp = dict(KR.attention_bwd_inputs(name))
    bfull = _run_bwd(ctx, dict(binp, valid_len=np.array([T] * B, dtype=np.int32)))
    bover = _run_bwd(ctx, dict(binp, valid_len=np.array([T + 7] * B, dtype=np.int32)))
    for k in ("ds", "dctx", "dh0"):
        assert np.array_equal(_bits(bfull[k]), _bits(bover[k])), k
    bnone = _run_bwd(ctx, dict(binp, valid_len=np.array([0, -3, T], dtype=np.int32)))
    assert np.isfinite(bnone["ds"]).all() and np.isfinite(bnone["dh0"]).all()
    assert not bnone["ds"][:2].any() and not bnone["dh0"][:2].any()
    assert np.array_equal(_bits(bnone["ds"][2]), _bits(bfull["ds"][2])) and np.array_equal(_bits(bnone["dctx"]), _bits(bfull["dctx"]))


# ---- attention backward -----------------------------------------------------------------------------------------------------------

def _run_bwd(ctx, inp, use_c0=True, use_c1=True):
    L = _lib()
    B, T, H = inp["mem"].shape
    d = [_dev(inp["aw"]), _dev(inp["mem"]), _dev(inp["keyproj"]), _dev(inp["c0"]) if use_c0 else None, _dev(inp["c1"]) if use_c1 else None,
         _dev(np.asarray(inp["valid_len"], dtype=np.int32))]
    ds, dctx, dh0 = Out(B, T), Out(B, H), Out(B, H)
    L.check(ctx.lib.tn_dbg_gnmt_attention_bwd(ctx.handle, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), inp["c0"].shape[1], L.ptr(d[4]),
                                              inp["c1"].shape[1], L.ptr(d[5]), B, T, H, ds.ptr, dctx.ptr, dh0.ptr), "tn_dbg_gnmt_attention_bwd")
    return dict(ds=ds.read(), dctx=dctx.read(), dh0=dh0.read())


@pytest.mark.parametrize("name", [c[0] for c in KR.ATT_CASES])
def test_attention_backward(ctx, report, name):
    """both addends of d context at pitches H + 4 and 2 H + 8, then each alone"""
    fails = []
    for use_c0, use_c1 in ((True, True), (True, False), (False, True)):
        inp, ref64, ref32 = _bwd_refs(name, use_c0, use_c1)
        got = _run_bwd(ctx, inp, use_c0, use_c1)
        T = inp["mem"].shape[1]
        for b, v in enumerate(KR.clamp_len(inp["valid_len"], T)):
            assert not got["ds"][b, v:].any(), (name, "ds past valid_len", b)
        if use_c0 and use_c1:
            again = _run_bwd(ctx, inp)
            for k in ("ds", "dctx", "dh0"):
                assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, "not bit-identical on a repeated call")
        tag = f"bwd_{name}_c{int(use_c0)}{int(use_c1)}"
        fails += [_check(report, tag, k, got[k], ref64, ref32) for k in ("ds", "dctx", "dh0")]
    _assert_all(fails)


# ---- attention outer products -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps,T,H", KR.OUTER_CASES)
def test_attention_outer(ctx, report, steps, T, H):
    L = _lib()
    inp = KR.attention_outer_inputs(steps, T, H)
    ref64, ref32 = KR.attention_outer(inp), KR.attention_outer(inp, np.float32)
    B = inp["aw"].shape[1]
    d = [_dev(inp[k]) for k in ("aw", "ds", "dctx", "h0")]
    res = []
    for _ in range(2):
        dmem, dkp = Out(B, T, H), Out(B, T, H)
        L.check(ctx.lib.tn_dbg_gnmt_attention_outer(ctx.handle, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), inp["h0"].shape[2], steps, B, T,
                                                    H, dmem.ptr, dkp.ptr), "tn_dbg_gnmt_attention_outer")
        res.append(dict(dmem=dmem.read(), dkp=dkp.read()))
    assert all(np.array_equal(_bits(res[0][k]), _bits(res[1][k])) for k in ("dmem", "dkp")), "not bit-identical on a repeated call"
    _assert_all(_check(report, f"outer_L{steps}_T{T}_H{H}", k, res[0][k], ref64, ref32) for k in ("dmem", "dkp"))


# ---- cross-entropy ----------------------------------------------------------------------------------------------------------------

def _run_ce(ctx, inp):
    L = _lib()
    B, Ls, V = inp["logits"].shape
    d = [_dev(inp["logits"]), _dev(inp["labels"]), _dev(inp["valid_len"])]
    dlog, rows, loss, masked = Out(Ls, B, V), Out(Ls, B), Out(1), Out(B)
    L.check(ctx.lib.tn_dbg_gnmt_ce(ctx.handle, L.ptr(d[0]), L.ptr(d[1]), inp["labels"].shape[1], L.ptr(d[2]), B, Ls, V, dlog.ptr, rows.ptr,
                                   loss.ptr, masked.ptr), "tn_dbg_gnmt_ce")
    return dict(dlogits=dlog.read(), loss_rows=rows.read(), loss=loss.read()[0], masked_loss=masked.read())


@pytest.mark.parametrize("V,L", KR.CE_CASES)
def test_cross_entropy(ctx, report, V, L):
    inp = KR.ce_inputs(V, L)
    got = _run_ce(ctx, inp)
    ref64, ref32 = KR.ce(inp), KR.ce(inp, np.float32)
    # rows at or past valid_len (clip 1 has none valid) carry no gradient and no loss, exactly
    valid = np.arange(L)[:, None] < inp["valid_len"][None, :]
    assert not got["dlogits"][~valid].any() and not got["loss_rows"][~valid].any() and got["masked_loss"][1] == 0.0
    zero = _run_ce(ctx, KR.ce_inputs(V, L, all_masked=True))
    for k in ("dlogits", "loss_rows", "loss", "masked_loss"):
        assert np.isfinite(zero[k]).all() and not np.any(zero[k]), (k, "every valid_len 0 must give exact zeros")
    _assert_all(_check(report, f"ce_V{V}_L{L}", k, got[k], ref64, ref32) for k in ("dlogits", "loss_rows", "loss", "masked_loss"))


# ---- embedding gradient -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E,V", KR.EMB_CASES)
def test_embedding_gradient(ctx, report, E, V):
    L = _lib()
    inp = KR.emb_inputs(E, V)
    ref64 = KR.emb_grad(inp)
    ref32 = KR.emb_grad(inp, np.float32)
    d = [_dev(inp["dx0"]), _dev(inp["tgt"])]
    res = []
    for _ in range(2):
        demb = Out(V, E)
        L.check(ctx.lib.tn_dbg_gnmt_emb_grad(ctx.handle, L.ptr(d[0]), inp["dx0"].shape[2], L.ptr(d[1]), inp["tgt"].shape[1], inp["B"], inp["L"], E,
                                             V, demb.ptr), "tn_dbg_gnmt_emb_grad")
        res.append(demb.read())
    assert np.array_equal(_bits(res[0]), _bits(res[1])), "not bit-identical on a repeated call"
    used = set(np.maximum(inp["tgt"][:, :inp["L"]], 0).ravel().tolist())
    assert not res[0][[v for v in range(V) if v not in used]].any(), "the row of a token that never occurs must be exactly zero"
    _assert_all([_check(report, f"emb_E{E}_V{V}", "demb", res[0], ref64, ref32)])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_hooks_refuse_bad_arguments(ctx):
    """null pointer, H % 4 != 0, a pitch below its width, LDS beyond the step kernels' 152 KiB: TN_ERR_INVALID and a message, no launch"""
    L = _lib()
    lib, h = ctx.lib, ctx.handle
    f = torch.zeros(4096, dtype=torch.float32, device="cuda")
    i = torch.ones(64, dtype=torch.int32, device="cuda")
    o = torch.zeros(4096, dtype=torch.float32, device="cuda")          # every output of the accepted calls lands in here
    p, q, nul, po = L.ptr(f), L.ptr(i), None, L.ptr(o)
    B, T, H = 2, 5, 8

    def refused(rc, what):
        assert rc == -1, (what, rc)        # TN_ERR_INVALID
        with pytest.raises(RuntimeError, match="invalid argument"):
            L.check(rc, what)

    fwd = lambda **k: lib.tn_dbg_gnmt_attention_fwd(h, k.get("g0", p), p, k.get("ldh", H), k.get("cprev", nul), k.get("lstm", 0), p, p,
                                                    k.get("vl", q), B, k.get("T", T), k.get("H", H), 1, k.get("cap", 0), po, k.get("cn", nul), po,
                                                    k.get("ldx1", 3 * H), po, k.get("w", po))
    assert fwd() == 0
    for what, kw in (("null g0", dict(g0=nul)), ("null valid_len", dict(vl=nul)), ("null weights", dict(w=nul)), ("H % 4", dict(H=6)),
                     ("ldh < H", dict(ldh=H - 1)), ("ldx1 < 2H", dict(ldx1=2 * H - 1)), ("lstm without cprev", dict(lstm=1)),
                     ("split_cap 3", dict(cap=3)), ("LDS", dict(T=40000))):
        refused(fwd(**kw), "fwd " + what)
    bwd = lambda **k: lib.tn_dbg_gnmt_attention_bwd(h, k.get("aw", p), p, p, k.get("c0", p), k.get("lc0", H), k.get("c1", p), k.get("lc1", H),
                                                    q, B, k.get("T", T), k.get("H", H), po, po, k.get("dh0", po))
    assert bwd() == 0 and bwd(c1=nul, lc1=0) == 0
    for what, kw in (("null aw", dict(aw=nul)), ("both addends null", dict(c0=nul, c1=nul)), ("null dh0", dict(dh0=nul)), ("H % 4", dict(H=10)),
                     ("lc0 < H", dict(lc0=H - 4)), ("lc1 < H", dict(lc1=0)), ("LDS", dict(T=40000))):
        refused(bwd(**kw), "bwd " + what)
    outer = lambda **k: lib.tn_dbg_gnmt_attention_outer(h, p, k.get("ds", p), p, p, k.get("ldh", H), 2, B, T, k.get("H", H), po, k.get("dkp", po))
    for what, kw in (("null ds", dict(ds=nul)), ("null dkp", dict(dkp=nul)), ("H % 4", dict(H=7)), ("ldh < H", dict(ldh=4))):
        refused(outer(**kw), "outer " + what)
    ce = lambda **k: lib.tn_dbg_gnmt_ce(h, p, k.get("labels", q), k.get("ld", 3), q, B, 3, 7, po, po, k.get("loss", po), po)
    for what, kw in (("null labels", dict(labels=nul)), ("null loss", dict(loss=nul)), ("ld < L", dict(ld=2))):
        refused(ce(**kw), "ce " + what)
    emb = lambda **k: lib.tn_dbg_gnmt_emb_grad(h, k.get("dx0", p), k.get("K0", 9), q, k.get("ld", 3), B, 3, 6, 5, po)
    for what, kw in (("null dx0", dict(dx0=nul)), ("K0 <= E", dict(K0=6)), ("ld < L", dict(ld=2))):
        refused(emb(**kw), "emb " + what)
