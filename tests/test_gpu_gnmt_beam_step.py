"""-m gpu: the beam-search step kernel dec_beam_kernel<NBM> (tennis_amd/csrc/gnmt_kernels.hip) on its own, against NumPy float64.

Through tn_dbg_gnmt_beam_step (include/tennis_hip_debug.h): one launch with the instantiation, LDS, projection split and extra
workgroups tn_gnmt_beam_search computes for the shape.  Cases, input recipes, the reference, metrics and bars are
tests/tools/gnmt_step_refs.py's (checked on the CPU by tests/test_cpu_gnmt_step_refs.py against the oracle's sampler, with eight
mutants at least 10 bars away).  Every score the kernel selected is compared with float64's value for that same (parent, word)
against (|score prev_lp| + sum|wp h| + |bp| + |lse|) / lp; the states absolutely; bar = max(1e-6, 16 x the float32 NumPy
evaluation's error).  Selection, order and all bookkeeping must equal float64's: before comparing, each case asserts, on the
reference alone, that float64's gaps between consecutive winners and behind the last one exceed two bars (exact twins apart, in the
two tie cases, where the lower index must win).  The projection is not peaked (scale 1), so every column counts in the log-sum-exp.
Every buffer the kernel may write sits between sentinel guards.  The measured error / bar go to the session report."""
import ctypes as C

import numpy as np
import pytest
import torch

from tools import gnmt_step_refs as SR
from tools.guarded import Guarded, bits, dev

pytestmark = pytest.mark.gpu

PAD = 7.0
X1_ROW_PAD, X1_COL_PAD = 3, 4        # k-group-major x1 with R + 3 rows; row-major x1 at pitch 3 H + 4
I32 = np.int32


def _lib():
    from tennis_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx():
    return _lib().default_context()


def _run(ctx, inp, c, with_p0=True):
    """one tn_dbg_gnmt_beam_step call on the case's operands -> dict of everything the kernel wrote (keys as SR.beam_step's)"""
    L = _lib()
    beam, lstm, form = inp["beam"], inp["lstm"], inp["form"]
    R, H = inp["hprev"].shape
    B, V, step = R // beam, inp["wp"].shape[0], inp["step"]
    x1full = np.concatenate([inp["xin"], inp["xctx"], inp["hprev"]], axis=1)
    k4 = form == "tok_k4"
    if k4:
        rows = R + X1_ROW_PAD
        x1 = Guarded(3 * H // 4 * rows * 4, init=SR.k4(x1full, rows).reshape(-1))
        ldx1 = -rows
    else:
        ldx1 = 3 * H + X1_COL_PAD
        x1 = Guarded(R, 3 * H, ld=ldx1, init=x1full)
    g1 = dev(inp["g1"])
    c1 = Guarded(R, H, init=inp["c1"]) if lstm else None
    scores, alive, vlen = Guarded(R, init=inp["scores"]), Guarded(R, dtype=I32, init=inp["alive"]), Guarded(R, dtype=I32, init=inp["vlen"])
    bpp, bpw = Guarded(step, R, dtype=I32), Guarded(step, R, dtype=I32)
    flag = Guarded(1, dtype=I32, init=[0])
    hstate = Guarded(R, H) if inp["residual"] else None
    parent, tok = Guarded(R, dtype=I32), Guarded(R, dtype=I32) if form != "x0_rm" else None
    wp, bp = np.ascontiguousarray(inp["wp"]), np.ascontiguousarray(inp["bp"])
    P = lambda g: g.ptr if g is not None else None
    keep = []
    if form == "x0_rm":
        E = inp["emb"].shape[1]
        keep = [dev(inp["emb"]), dev(inp["ctxv"]), dev(inp["h0n"]), dev(inp["c0n"]) if lstm else None]
        x0, c0cur, p0 = Guarded(R, E + 2 * H), Guarded(R, H) if lstm else None, None
        tail = (None, None, None, 0, None, L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(keep[3]), x0.ptr, P(c0cur))
    else:
        E = SR.BEAM_E
        x0, c0cur = None, None
        p0 = Guarded(R, 4 * H) if with_p0 else None
        if with_p0:
            keep = [dev(inp["w1x"]), dev(inp["b1x"])]
            tail = (tok.ptr, L.ptr(keep[0]), L.ptr(keep[1]), inp["K1p"], p0.ptr, None, None, None, None, None, None)
        else:
            tail = (tok.ptr, None, None, 0, None, None, None, None, None, None, None)
    rc = ctx.lib.tn_dbg_gnmt_beam_step(ctx.handle, L.ptr(g1), x1.ptr, ldx1, 1 if lstm else 0, P(c1), wp.ctypes.data_as(C.c_void_p),
                                       bp.ctypes.data_as(C.c_void_p), B, H, E, V, beam, step, float(inp["lp"]), float(inp["prev_lp"]),
                                       int(inp["eos"]), c["split_cap"], scores.ptr, alive.ptr, vlen.ptr, bpp.ptr, bpw.ptr, flag.ptr,
                                       P(hstate), parent.ptr, *tail)
    L.check(rc, "tn_dbg_gnmt_beam_step")
    # ---- read back; nothing outside the documented outputs may have changed ----
    if k4:
        raw = x1.raw().reshape(3 * H // 4, R + X1_ROW_PAD, 4)
        assert (raw[:, R:, :] == PAD).all(), "rows of x1 past B * beam were written"
        x1new = SR.unk4(raw.reshape(-1), R, 3 * H)
    else:
        raw = x1.raw().reshape(R, ldx1)
        assert (raw[:, 3 * H:] == x1.sent).all(), "columns of x1 past 3 H were written"
        x1new = raw[:, :3 * H]
    assert np.array_equal(bits(x1new[:, :2 * H]), bits(x1full[:, :2 * H])), "x1[:, 0:2H] (the cell's input) was written"
    par_rows, word_rows = bpp.read(), bpw.read()
    assert (par_rows[:step - 1] == -777).all() and (word_rows[:step - 1] == -777).all(), "back-pointers of another step were written"
    got = dict(scores=scores.read(), alive=alive.read(), vlen=vlen.read(), par=par_rows[step - 1], word=word_rows[step - 1],
               flag=int(flag.read()[0]), parent_out=parent.read(), tok=tok.read() if tok is not None else None,
               hstate=hstate.read() if hstate is not None else None, h_gather=x1new[:, 2 * H:].copy(),
               c_gather=c1.read() if lstm else None, x0=x0.read() if x0 is not None else None,
               c0cur=c0cur.read() if c0cur is not None else None, p0=p0.read() if p0 is not None else None)
    del g1, keep
    return got


def _same_bits(a, b, skip=()):
    for k in a:
        if k in skip or a[k] is None:
            continue
        assert np.array_equal(bits(np.asarray(a[k])), bits(np.asarray(b[k]))), k


PARAMS = [(c["name"], cell) for c in SR.BEAM_CASES for cell in SR.BEAM_CELLS]


@pytest.mark.parametrize("name,cell", PARAMS, ids=[f"{n}-{c}" for n, c in PARAMS])
def test_beam_step_matches_float64(ctx, report, name, cell):
    c = SR.BEAM_BY_NAME[name]
    inp, r64, r32, _ = SR.beam_inputs(name, cell)
    # from the reference alone: the winners are separated, so selection and order are float64's or the kernel is wrong
    gap, zeros = SR.beam_gaps(r64, SR.beam_bars(r64, r32)["scores"], c["beam"])
    assert gap > SR.GAP_BARS and (zeros > 0) == (c["tie"] is not None), (gap, zeros)
    got = _run(ctx, inp, c)
    for k, v in got.items():
        assert v is None or np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    res = SR.beam_compare(got, inp, r64, r32)
    worst = {k: SR.ratio(*v) for k, v in res.items()}
    for k, (e, b) in res.items():
        report[f"gnmt_beam_step_{name}_{cell}_{k}"] = [e, b]
    print(name, cell, {k: f"{v:.3f}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, {k: (res[k], v) for k, v in worst.items() if v > 1.0}
    _same_bits(got, _run(ctx, inp, c))                                   # a repeated call gives the same bits
    if c["form"] != "x0_rm":                                             # the clips' outputs do not depend on the extra workgroups
        _same_bits(got, _run(ctx, inp, c, with_p0=False), skip=("p0",))
    if not inp["lstm"]:
        assert got["c_gather"] is None and got["c0cur"] is None


def test_hook_refuses_what_it_cannot_launch(ctx):
    L = _lib()
    f = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    i = torch.zeros(1 << 12, dtype=torch.int32, device="cuda")
    host = np.zeros(1 << 16, dtype=np.float32)
    hp = host.ctypes.data_as(C.c_void_p)
    p, q, n = L.ptr(f), L.ptr(i), None

    def call(g1=p, x1=p, ldx1=24, lstm=0, c1=n, wp=hp, B=1, H=8, E=4, V=30, beam=3, step=1, split_cap=0, tok=n, w1x=n, b1x=n, K1p=0, p0=n,
             emb=p, ctxv=p, h0n=p, x0=p):
        return ctx.lib.tn_dbg_gnmt_beam_step(ctx.handle, g1, x1, ldx1, lstm, c1, wp, hp, B, H, E, V, beam, step, 1.0, 1.0, 2, split_cap, p, q, q, q, q,
                                             q, n, q, tok, w1x, b1x, K1p, p0, emb, ctxv, h0n, n, x0, n)
    off = C.c_void_p(f.data_ptr() + 4)
    bad = [dict(g1=n), dict(wp=n), dict(H=6), dict(beam=0), dict(beam=17, V=40), dict(V=2), dict(ldx1=20), dict(ldx1=-2), dict(step=0),
           dict(split_cap=3), dict(lstm=1), dict(emb=n), dict(beam=16, H=256, V=4000, ldx1=768),
           dict(tok=q), dict(tok=q, emb=n, ctxv=n, h0n=n, x0=n, p0=p, w1x=n, b1x=p, K1p=32),
           dict(tok=q, emb=n, ctxv=n, h0n=n, x0=n, p0=p, w1x=p, b1x=p, K1p=12),
           dict(tok=q, emb=n, ctxv=n, h0n=n, x0=n, p0=p, w1x=off, b1x=p, K1p=32),
           dict(tok=q, emb=n, ctxv=n, h0n=n, x0=n, p0=p, w1x=p, b1x=p, K1p=32, ldx1=26)]
    for kw in bad:
        assert call(**kw) != 0, kw
    assert not f.any() and not i.any()
