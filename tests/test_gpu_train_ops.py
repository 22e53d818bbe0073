"""-m gpu: the small operator kernels that carry a training step from one GEMM to the next (csrc/finetune.hip ft_*, csrc/train.hip),
each alone against its float64 reference (oracle/train_ops_np.py, pinned on the CPU by tests/test_cpu_train_ops_ref.py), through the
tn_dbg_* hooks of include/tennis_hip_debug.h, which run the launchers the steps call.  Shapes and inputs: tests/tools/train_ops_cases.py.

Every case: outputs pre-filled with NaN, padding columns (ld > C) and a tail behind every output hold a sentinel that must survive,
padding columns of strided INPUTS hold NaN that must never be read, and the operator runs twice with bit-identical results.

Bars (u = 2^-24; docs/numerics.md, "The training steps' operator kernels, alone"); none is tuned to the code under test:
  * pure data movement - bit-exact;
  * integer-valued operands (every float32 sum exact) - the float64 reference rounded once, bit for bit;
  * a sum of n float32 terms in any order - |got - ref| <= (n + 1) u sum|terms| (first-order Higham), terms from the reference;
  * folded im2col3 (one fmaf, one fmaxf) - 2u |ref|, exactly 0 where the ReLU is closed;
  * optimisers and the running statistics - 8u sum|terms of the update|;
  * bn_fold, softmax_ce (rsqrtf / expf / logf) - 4x the worst error measured on MI355X over these cases, under a derived ceiling.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import train_ops_np as R
from tools import train_ops_cases as K

pytestmark = pytest.mark.gpu

U = K.U
SENT = np.float32(-123456.75)        # what padding columns and tails hold
TAIL = 96                            # floats behind every output
INT_FILL = -(2 ** 31) + 7

# Measured on MI355X over the cases of this file, in units of u, relative to the scales of docs/numerics.md:
#   bn_fold sc 1.77 (|ref|), sh 2.36 (|beta| + |mean sc|); softmax_ce loss 1.37, dlogits 2.24 (the label element after the u/2 |ref| of
#   its store; by the plain scale that element reaches 3631, see test_softmax_ce).
# The bars are 4x that, and never above the ceilings: 8u for the fold (which caps sh: 4 x 2.36 = 9.4), (C + 16) u for the loss quantities.
FOLD_SC_BAR, FOLD_SH_BAR, FOLD_CEIL = 7.1, 8.0, 8.0
CE_LOSS_BAR, CE_DLOGITS_BAR = 5.5, 9.0


def _lib():
    from tennis_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx():
    return _lib().default_context()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _strided(a, ld, fill=np.nan):
    """(rows, cols) -> device (rows, ld) with `fill` in the padding columns: NaN for an input (never to be read)"""
    rows, cols = a.shape
    h = np.full((rows, ld), fill, np.float32)
    h[:, :cols] = a
    return _dev(h)


class Out:
    """A (rows, cols) output of row stride ld inside a larger device tensor: NaN (int32: INT_FILL) where the operator must write
    (or `init` for an operator that updates in place), SENT in the padding columns and in the tail"""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, init=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.n = rows * self.ld
        self.buf = torch.empty(self.n + TAIL, dtype=dtype, device="cuda")
        body = self.buf[:self.n].view(rows, self.ld)
        body.fill_(float("nan") if dtype == torch.float32 else INT_FILL)
        if init is not None:
            body[:, :cols] = _dev(np.asarray(init).reshape(rows, cols))
        self.sent = float(SENT) if dtype == torch.float32 else int(SENT)
        body[:, cols:] = self.sent
        self.buf[self.n:] = self.sent

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def read(self, what=""):
        h = self.buf.cpu().numpy()
        assert (h[self.n:] == self.sent).all(), f"{what}: wrote behind its output"
        body = h[:self.n].reshape(self.rows, self.ld)
        assert (body[:, self.cols:] == self.sent).all(), f"{what}: wrote into the padding columns"
        return body[:, :self.cols].copy()


def _twice(run):
    a, b = run(), run()
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), f"output {i} differs between two runs"
    return a


def _ok(ctx, rc, what):
    _lib().check(rc, what)


def _bits(got, ref, what):
    """bit-exact against the float64 reference, whose values are float32 values"""
    ref32 = np.asarray(ref).astype(np.float32).reshape(got.shape)
    bad = got.view(np.uint32) != ref32.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _exact(got, ref, what):
    """integer-valued operands: the float64 reference is exact, and so must the float32 result be"""
    ref = np.asarray(ref).reshape(got.shape)
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64)), what
    bad = got.astype(np.float64) != ref
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _worst(report, key, v):
    report[key] = max(float(v), report.get(key, 0.0))


def _higham(report, key, got, ref, mag, n, what):
    """|got - ref| <= (n + 1) u sum|terms|; the worst ratio to the bound goes to the report"""
    ref, mag = np.asarray(ref).reshape(got.shape), np.asarray(mag).reshape(got.shape)
    assert np.isfinite(got).all(), what
    err, bound = np.abs(got.astype(np.float64) - ref), (n + 1) * U * mag
    _worst(report, f"train_ops_{key}_err_over_bound", (err / np.maximum(bound, 1e-300)).max() if err.any() else 0.0)
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), np.argwhere(bad)[:4].tolist())


# ---- im2col / col2im -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W", K.IM2COL7_SHAPES)
def test_im2col7(ctx, B, H, W):
    x = K.normal((B, H, W, 3), 1, B, H, W)
    xd = _dev(x)
    M = B * (H // 2) * (W // 2)

    def run():
        o = Out(M, 147)
        _ok(ctx, ctx.lib.tn_dbg_ft_im2col7(ctx.handle, _ptr(xd), B, H, W, o.ptr), "tn_dbg_ft_im2col7")
        return [o.read("im2col7")]
    _bits(_twice(run)[0], R.im2col7(x), (B, H, W))


def _im2col3(ctx, a, B, H, W, Cc, sc=None, sh=None):
    ad, scd, shd = _dev(a), (_dev(sc) if sc is not None else None), (_dev(sh) if sh is not None else None)

    def run():
        o = Out(B * H * W, 9 * Cc)
        _ok(ctx, ctx.lib.tn_dbg_ft_im2col3(ctx.handle, _ptr(ad), B, H, W, Cc, _ptr(scd), _ptr(shd), o.ptr), "tn_dbg_ft_im2col3")
        return [o.read("im2col3")]
    return _twice(run)[0]


def _col2im3(ctx, d, B, H, W, Cc):
    dd = _dev(d)

    def run():
        o = Out(B * H * W, Cc)
        _ok(ctx, ctx.lib.tn_dbg_ft_col2im3(ctx.handle, _ptr(dd), B, H, W, Cc, o.ptr), "tn_dbg_ft_col2im3")
        return [o.read("col2im3")]
    return _twice(run)[0]


@pytest.mark.parametrize("Cc", K.IM2COL3_C)
@pytest.mark.parametrize("B,H,W", K.IM2COL3_SHAPES)
def test_im2col3_plain_and_folded(ctx, report, B, H, W, Cc):
    a, sc, sh = K.fold_inputs(B, H, W, Cc)
    below, above, _ = K.fold_fractions(a, sc, sh)
    assert below >= 0.25 and above >= 0.25 and (sc < 0).any() and (sc == 0).any()
    _bits(_im2col3(ctx, a, B, H, W, Cc), R.im2col3(a), "plain")
    got = _im2col3(ctx, a, B, H, W, Cc, sc, sh)
    ref = R.im2col3(a, sc, sh)
    pre, width = K.fold_preactivation(a, sc, sh)
    amb = R.im2col((np.abs(pre) <= width).astype(np.float64), 3, 1, 1) > 0          # a sign that one rounding could flip
    wid = R.im2col(width, 3, 1, 1)
    report["train_ops_im2col3_fold_ambiguous"] = report.get("train_ops_im2col3_fold_ambiguous", 0) + int(amb.sum())
    assert amb.sum() < 1e-3 * amb.size
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    open_, closed = (ref != 0) & ~amb, (ref == 0) & ~amb
    assert closed.mean() >= 0.25
    assert (err[open_] <= 2 * U * np.abs(ref[open_])).all(), float((err[open_] / np.abs(ref[open_])).max() / U)
    assert not got[closed].any(), "a closed ReLU (or the padding) is not exactly 0"
    assert (got >= 0).all() and (err[amb] <= wid[amb]).all()
    _worst(report, "train_ops_im2col3_fold_rel_err_u", (err[open_] / np.abs(ref[open_])).max() / U if open_.any() else 0.0)


@pytest.mark.parametrize("Cc", K.IM2COL3_C)
@pytest.mark.parametrize("B,H,W", K.IM2COL3_SHAPES)
def test_col2im3_and_the_adjoint_identity(ctx, report, B, H, W, Cc):
    M = B * H * W
    d = K.normal((M, 9 * Cc), 30, B, H, W, Cc)
    _higham(report, "col2im3", _col2im3(ctx, d, B, H, W, Cc), R.col2im3(d, B, H, W, Cc), R.col2im3(np.abs(d), B, H, W, Cc), 9, "random")
    di = K.integers((M, 9 * Cc), -3, 3, 31, B, H, W, Cc)
    ai = K.integers((B, H, W, Cc), -3, 3, 32, B, H, W, Cc)
    da = _col2im3(ctx, di, B, H, W, Cc)
    _exact(da, R.col2im3(di, B, H, W, Cc), "integers")
    # <im2col3(a), d> = <a, col2im3(d)>, exactly, from the device outputs alone
    col = _im2col3(ctx, ai, B, H, W, Cc)
    assert (col.astype(np.float64) * di).sum() == (ai.reshape(M, Cc).astype(np.float64) * da).sum()


# ---- pools -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", K.POOL_C)
@pytest.mark.parametrize("B,H,W", K.POOL_SHAPES)
def test_maxpool_forward_and_backward(ctx, report, B, H, W, Cc):
    Ho, Wo = H // 2, W // 2
    Mo = B * Ho * Wo
    for ldy in (Cc, Cc + 5):
        for kind in K.POOL_KINDS:
            what = (kind, ldy)
            a = K.pool_input(kind, B, H, W, Cc)
            if kind == "ties":
                assert K.tied_window_fraction(a) >= 0.3, what
            ad = _dev(a)
            dys = [("int", K.integers((Mo, Cc), -3, 3, 33, B, H, W, Cc))]
            if kind in ("ties", "random"):
                dys.append(("random", K.normal((Mo, Cc), 34, B, H, W, Cc)))
            for dkind, dy in dys:
                dyd = _strided(dy, ldy)

                def run():
                    y, da = Out(Mo, Cc, ldy), Out(B * H * W, Cc)
                    _ok(ctx, ctx.lib.tn_dbg_ft_maxpool(ctx.handle, _ptr(ad), B, H, W, Cc, y.ptr, ldy, _ptr(dyd), da.ptr), "tn_dbg_ft_maxpool")
                    return [y.read("maxpool"), da.read("maxpool_bwd")]
                y, da = _twice(run)
                _bits(y, R.maxpool(a), what)
                if kind == "negative":
                    assert (y < 0).all(), "the padding won a window"
                dy4 = dy.reshape(B, Ho, Wo, Cc)
                ref = R.maxpool_bwd(a, dy4)
                if dkind == "int":
                    _exact(da, ref, what)               # the routing, bit for bit
                    assert np.array_equal(da.reshape(B, H * W, Cc).astype(np.float64).sum(axis=1), dy4.reshape(B, -1, Cc).astype(np.float64).sum(axis=1))
                else:
                    _higham(report, "maxpool_bwd", da, ref, R.maxpool_bwd(a, np.abs(dy4)), 4, what)


@pytest.mark.parametrize("Cc", K.POOL_C)
@pytest.mark.parametrize("B,H,W", K.POOL_SHAPES)
def test_avgpool2_forward_and_backward(ctx, report, B, H, W, Cc):
    Ho, Wo = H // 2, W // 2
    Mo = B * Ho * Wo
    for ldy in (Cc, Cc + 5):
        for kind in ("int", "random"):
            what = (kind, ldy)
            if kind == "int":
                z, dy = K.integers((B, H, W, Cc), -3, 3, 35, B, H, W, Cc), K.integers((Mo, Cc), -3, 3, 36, B, H, W, Cc)
            else:
                z, dy = K.normal((B, H, W, Cc), 37, B, H, W, Cc), K.normal((Mo, Cc), 38, B, H, W, Cc)
            zd, dyd = _dev(z), _strided(dy, ldy)

            def run():
                y, dz = Out(Mo, Cc, ldy), Out(B * H * W, Cc)
                _ok(ctx, ctx.lib.tn_dbg_ft_avgpool2(ctx.handle, _ptr(zd), B, H, W, Cc, y.ptr, ldy, _ptr(dyd), dz.ptr), "tn_dbg_ft_avgpool2")
                return [y.read("avgpool2"), dz.read("avgpool2_bwd")]
            y, dz = _twice(run)
            ry, rdz = R.avgpool2(z), R.avgpool2_bwd(dy.reshape(B, Ho, Wo, Cc))
            if kind == "int":
                _exact(y, ry, what)
                _exact(dz, rdz, what)
            else:
                _higham(report, "avgpool2", y, ry, R.avgpool2(np.abs(z)), 4, what)
                _higham(report, "avgpool2_bwd", dz, rdz, np.abs(rdz), 1, what)


@pytest.mark.parametrize("B,P,Cc", K.GAP_SHAPES)
def test_gap_forward_and_backward(ctx, report, B, P, Cc):
    for kind in ("int", "random"):
        if kind == "int":
            a, df = K.integers((B, P, Cc), -3, 3, 39, B, P, Cc), K.integers((B, Cc), -3, 3, 40, B, P, Cc)
        else:
            a, df = K.normal((B, P, Cc), 41, B, P, Cc), K.normal((B, Cc), 42, B, P, Cc)
        ad, dfd = _dev(a), _dev(df)

        def run():
            f, da = Out(B, Cc), Out(B * P, Cc)
            _ok(ctx, ctx.lib.tn_dbg_ft_gap(ctx.handle, _ptr(ad), B, P, Cc, f.ptr, _ptr(dfd), da.ptr), "tn_dbg_ft_gap")
            return [f.read("gap"), da.read("gap_bwd")]
        f, da = _twice(run)
        rf, rda = R.gap(a), R.gap_bwd(df, P)
        if kind == "int" and P & (P - 1) == 0:            # s / P is exact in float32
            _exact(f, rf, kind)
            _exact(da, rda, kind)
        else:
            _higham(report, "gap", f, rf, R.gap(np.abs(a)), P, kind)
            _higham(report, "gap_bwd", da, rda, np.abs(rda), 1, kind)


# ---- BatchNorm fold and running statistics ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", K.BN_C)
def test_bn_fold_and_running(ctx, report, Cc):
    for seed in range(4):                                 # every channel meets every variance
        mean, var, gamma, beta, rmean, rvar = K.bn_inputs(Cc, seed)
        md, vd, gd, bd = _dev(mean), _dev(var), _dev(gamma), _dev(beta)

        def run():
            sc, sh = Out(1, Cc), Out(1, Cc)
            _ok(ctx, ctx.lib.tn_dbg_ft_bn_fold(ctx.handle, _ptr(md), _ptr(vd), _ptr(gd), _ptr(bd), Cc, sc.ptr, sh.ptr), "tn_dbg_ft_bn_fold")
            rm, rv = Out(1, Cc, init=rmean), Out(1, Cc, init=rvar)
            _ok(ctx, ctx.lib.tn_dbg_ft_bn_running(ctx.handle, rm.ptr, rv.ptr, _ptr(md), _ptr(vd), Cc), "tn_dbg_ft_bn_running")
            return [sc.read("bn_fold sc")[0], sh.read("bn_fold sh")[0], rm.read("bn_running mean")[0], rv.read("bn_running var")[0]]
        sc, sh, rm, rv = _twice(run)
        rsc, rsh = R.bn_fold(mean, var, gamma, beta)
        assert np.isfinite(sc).all() and np.isfinite(sh).all()
        assert not sc[gamma == 0].any()
        esc = np.abs(sc - rsc) / np.maximum(np.abs(rsc), 1e-300)
        esh = np.abs(sh - rsh) / (np.abs(beta.astype(np.float64)) + np.abs(mean * rsc) + 1e-300)
        print(f"bn_fold C={Cc} seed={seed}: sc {esc.max() / U:.3f} u, sh {esh.max() / U:.3f} u")
        _worst(report, "train_ops_bn_fold_sc_err_u", esc.max() / U)
        _worst(report, "train_ops_bn_fold_sh_err_u", esh.max() / U)
        assert FOLD_SC_BAR <= FOLD_CEIL and FOLD_SH_BAR <= FOLD_CEIL
        assert esc.max() <= FOLD_SC_BAR * U and esh.max() <= FOLD_SH_BAR * U, (esc.max() / U, esh.max() / U)
        # running = 0.9 running + 0.1 batch: two products and a sum, the constants 0.9f and 1 - 0.9f (0.4 u and 4 u from 0.9 and 0.1)
        rrm, rrv = R.bn_running(rmean, rvar, mean, var)
        for got, ref, old, new, name in ((rm, rrm, rmean, mean, "mean"), (rv, rrv, rvar, var, "var")):
            terms = np.abs(R.BN_MOMENTUM * old.astype(np.float64)) + np.abs((1 - R.BN_MOMENTUM) * new.astype(np.float64))
            err = np.abs(got - ref)
            _worst(report, "train_ops_bn_running_err_u", (err / np.maximum(terms, 1e-300)).max() / U)
            assert (err <= 8 * U * terms).all(), (name, float((err / np.maximum(terms, 1e-300)).max() / U))


# ---- max over time ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("ties", "random"))
@pytest.mark.parametrize("B,T,F", K.POOLT_SHAPES)
def test_pool_max_arg_and_scatter(ctx, B, T, F, kind):
    x = K.poolt_input(kind, B, T, F)
    if kind == "ties" and T > 1:                          # (a column of one step cannot tie)
        assert K.tied_column_fraction(x) >= 0.3
    dp = K.normal((B, F), 43, B, T, F)
    xd, dpd = _dev(x), _dev(dp)

    def run():
        y, arg, ds = Out(B, F), Out(B, F, dtype=torch.int32), Out(B * T, F)
        _ok(ctx, ctx.lib.tn_dbg_pool_max_arg(ctx.handle, _ptr(xd), B, T, F, y.ptr, arg.ptr, _ptr(dpd), ds.ptr), "tn_dbg_pool_max_arg")
        return [y.read("pool_max_arg"), arg.read("pool_max_arg arg"), ds.read("scatter_pool_grad")]
    y, arg, ds = _twice(run)
    ry, rarg = R.pool_max_arg(x)
    _bits(y, ry, kind)
    assert np.array_equal(arg, rarg), kind
    _bits(ds, R.scatter_pool_grad(dp, rarg, T), kind)
    assert np.array_equal(ds.reshape(B, T, F).astype(np.float64).sum(axis=1), dp.astype(np.float64))      # sum over t of the scatter = dpooled


# ---- softmax cross-entropy --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Cc", K.CE_SHAPES)
def test_softmax_ce(ctx, report, B, Cc):
    """Scales: loss |max| + |log sum| + |p[label]| + 1; dlogits softmax_c (1 + |p_c| + |lse|) + u.  At the label the kernel stores
    softmax - 1, a float32 near -1: that store alone rounds by up to u/2 |ref|, which no float32 result can avoid and the scale above
    (proportional to softmax[label]) does not hold when the label is improbable, so that element is allowed u/2 |ref| on top and the
    error by the plain scale is reported beside it (docs/numerics.md)."""
    ceil = Cc + 16.0
    loss_bar, d_bar = min(CE_LOSS_BAR, ceil), min(CE_DLOGITS_BAR, ceil)
    for rot in range(len(K.CE_KINDS) if B < len(K.CE_KINDS) else 1):
        p, labels = K.ce_inputs(B, Cc, rot)
        assert labels.min() >= 0 and labels.max() < Cc and (B < Cc or len(set(labels.tolist())) == Cc)
        pd, ld = _dev(p), _dev(labels)

        def run():
            loss, d = Out(1, B), Out(B, Cc)
            _ok(ctx, ctx.lib.tn_dbg_softmax_ce(ctx.handle, _ptr(pd), _ptr(ld), labels.ctypes.data_as(C.c_void_p), B, Cc, loss.ptr, d.ptr),
                "tn_dbg_softmax_ce")
            return [loss.read("softmax_ce loss")[0], d.read("softmax_ce dlogits")]
        loss, d = _twice(run)
        rl, rd = R.softmax_ce(p, labels)
        m, ls = R.log_sum_exp(p)
        p64, rows = p.astype(np.float64), np.arange(B)
        soft = np.exp(p64 - (m + ls)[:, None])
        s_loss = np.abs(m) + np.abs(ls) + np.abs(p64[rows, labels]) + 1.0
        s_d = soft * (1.0 + np.abs(p64) + np.abs(m + ls)[:, None]) + U
        assert np.isfinite(loss).all() and np.isfinite(d).all()
        store = np.zeros_like(rd)
        store[rows, labels] = 0.5 * U * np.abs(rd[rows, labels])          # the rounding of softmax - 1 when it is stored
        err = np.abs(d - rd)
        el, ed, ed_plain = np.abs(loss - rl) / s_loss, np.maximum(err - store, 0.0) / s_d, (err / s_d)[rows, labels]
        print(f"softmax_ce B={B} C={Cc} rot={rot}: loss {el.max() / U:.3f} u (row {el.argmax()}), dlogits {ed.max() / U:.3f} u "
              f"(row {np.unravel_index(ed.argmax(), ed.shape)[0]}); label element by the plain scale {ed_plain.max() / U:.3f} u (row {ed_plain.argmax()})")
        _worst(report, "train_ops_softmax_ce_loss_err_u", el.max() / U)
        _worst(report, "train_ops_softmax_ce_dlogits_err_u", ed.max() / U)
        _worst(report, "train_ops_softmax_ce_dlogits_label_plain_scale_err_u", ed_plain.max() / U)
        assert el.max() <= loss_bar * U, (rot, el.max() / U)
        assert ed.max() <= d_bar * U, (rot, ed.max() / U)
        assert (loss >= 0).all()
        assert (np.abs(d.astype(np.float64).sum(axis=1)) <= (d_bar * U * s_d + store).sum(axis=1)).all()      # a row of dlogits sums to 0


# ---- dense backward, column sums --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Cc,Kd", K.DENSE_SHAPES)
def test_dense_bwd(ctx, report, B, Cc, Kd):
    for kind in ("int", "random"):
        if kind == "int":
            d, x, w = (K.integers(s, -3, 3, 44 + i, B, Cc, Kd) for i, s in enumerate(((B, Cc), (B, Kd), (Cc, Kd))))
        else:
            d, x, w = (K.normal(s, 47 + i, B, Cc, Kd) for i, s in enumerate(((B, Cc), (B, Kd), (Cc, Kd))))
        dd, xd, wd = _dev(d), _dev(x), _dev(w)

        def run():
            dw, db, dx = Out(Cc, Kd), Out(1, Cc), Out(B, Kd)
            _ok(ctx, ctx.lib.tn_dbg_dense_bwd(ctx.handle, _ptr(dd), _ptr(xd), _ptr(wd), B, Cc, Kd, dw.ptr, db.ptr, dx.ptr), "tn_dbg_dense_bwd")
            return [dw.read("dense_bwd dwd"), db.read("dense_bwd dbd")[0], dx.read("dense_bwd dpooled")]
        dw, db, dx = _twice(run)
        rdw, rdb, rdx = R.dense_bwd(d, x, w)
        if kind == "int":
            _exact(dw, rdw, "dwd"), _exact(db, rdb, "dbd"), _exact(dx, rdx, "dpooled")
        else:
            mdw, mdb, mdx = R.dense_bwd(np.abs(d), np.abs(x), np.abs(w))
            _higham(report, "dense_bwd", dw, rdw, mdw, B, "dwd")
            _higham(report, "dense_bwd", db, rdb, mdb, B, "dbd")
            _higham(report, "dense_bwd", dx, rdx, mdx, Cc, "dpooled")


def _colsum_case(ctx, report, rows, cols, lda):
    for kind in ("int", "random"):
        if kind == "int":
            A = K.integers((rows, cols), -3, 3, 50, rows, cols)
        else:
            A = K.normal((rows, cols), 51, rows, cols)
            A[:, 0] = 50.0 + 1e-2 * K.normal((rows,), 52, rows, cols)            # a large-mean column
        Ad = _strided(A, lda)

        def run():
            o = Out(1, cols)
            _ok(ctx, ctx.lib.tn_dbg_colsum(ctx.handle, _ptr(Ad), lda, rows, cols, o.ptr), "tn_dbg_colsum")
            return [o.read("colsum")[0]]
        got = _twice(run)[0]
        if kind == "int":
            _exact(got, R.colsum(A), (rows, cols, lda))
        else:
            _higham(report, "colsum", got, R.colsum(A), R.colsum(np.abs(A)), rows, (rows, cols, lda))


@pytest.mark.parametrize("rows", K.COLSUM_ROWS)
def test_colsum(ctx, report, rows):
    for cols in K.COLSUM_COLS:
        for lda in (cols, cols + 3):
            _colsum_case(ctx, report, rows, cols, lda)


def test_colsum_one_long_column(ctx, report):
    _colsum_case(ctx, report, *K.COLSUM_LONG)


# ---- optimisers -------------------------------------------------------------------------------------------------------------------

def _f32(v):
    return float(np.float32(v))


def _within(report, key, got, ref, terms, what):
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - ref)
    _worst(report, f"train_ops_{key}_err_u", (err / np.maximum(terms, 1e-300)).max() / U)
    bad = err > 8 * U * terms
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(terms, 1e-300)).max() / U), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("clip", (False, True))
@pytest.mark.parametrize("n", K.OPT_N)
def test_sgd_momentum(ctx, report, n, clip):
    lr, mo, wd, rs = _f32(0.01), _f32(0.9), _f32(1e-4), _f32(1.0 / 32)
    w0, g, m0, _ = K.opt_inputs(n)
    scale = _f32(K.CLIP_SCALE) if clip else 1.0
    gd = _dev(g)
    scd = _dev(np.array([K.CLIP_SCALE], np.float32)) if clip else None

    def run():
        w, m = Out(1, n, init=w0), Out(1, n, init=m0)
        res = []
        for _ in range(2):                                # two consecutive updates
            _ok(ctx, ctx.lib.tn_dbg_sgd_momentum(ctx.handle, w.ptr, _ptr(gd), m.ptr, n, lr, mo, wd, rs, _ptr(scd)), "tn_dbg_sgd_momentum")
            res += [w.read("sgd w")[0], m.read("sgd mom")[0]]
        return res
    w1, m1, w2, m2 = _twice(run)
    for (wa, ma), (wb, mb), k in (((w0, m0), (w1, m1), 1), ((w1, m1), (w2, m2), 2)):      # each update from the state the device had
        rw, rm = R.sgd_momentum(wa, g, ma, lr, mo, wd, rs, scale)
        wa, ga, ma = (np.abs(v.astype(np.float64)) for v in (wa, g, ma))
        tm = mo * ma + lr * rs * scale * ga + lr * wd * wa
        _within(report, "sgd", mb, rm, tm, ("mom", k))
        _within(report, "sgd", wb, rw, wa + tm, ("w", k))


@pytest.mark.parametrize("clip", (False, True))
@pytest.mark.parametrize("n", K.OPT_N)
def test_adam(ctx, report, n, clip):
    lr, b1, b2, eps = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(1e-8)
    w0, g, m0, v0 = K.opt_inputs(n)
    scale = _f32(K.CLIP_SCALE) if clip else 1.0
    gd = _dev(g)
    scd = _dev(np.array([K.CLIP_SCALE], np.float32)) if clip else None

    def run():
        w, m, v = Out(1, n, init=w0), Out(1, n, init=m0), Out(1, n, init=v0)
        res = []
        for step in K.ADAM_STEPS:
            _ok(ctx, ctx.lib.tn_dbg_adam(ctx.handle, w.ptr, _ptr(gd), m.ptr, v.ptr, n, lr, b1, b2, eps, step, _ptr(scd)), "tn_dbg_adam")
            res += [w.read("adam w")[0], m.read("adam m")[0], v.read("adam v")[0]]
        return res
    res = _twice(run)
    state = (w0, m0, v0)
    for i, step in enumerate(K.ADAM_STEPS):
        wa, ma, va = state
        wb, mb, vb = res[3 * i:3 * i + 3]
        lr_t = _f32(R.adam_rate(lr, b1, b2, step))        # the rate is a float32 kernel argument
        rw, rm, rv = R.adam(wa, g, ma, va, lr_t, b1, b2, eps, scale)
        ga = scale * np.abs(g.astype(np.float64))
        _within(report, "adam", mb, rm, b1 * np.abs(ma.astype(np.float64)) + (1 - b1) * ga, ("m", step))
        _within(report, "adam", vb, rv, b2 * np.abs(va.astype(np.float64)) + (1 - b2) * ga * ga, ("v", step))
        _within(report, "adam", wb, rw, np.abs(wa.astype(np.float64)) + np.abs(lr_t * rm / (np.sqrt(rv) + eps)), ("w", step))
        state = (wb, mb, vb)


# ---- frame staging, transpose -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,frame", K.STAGE_SHAPES)
def test_stage_frames(ctx, B, T, frame):
    for rot in range(4):
        x, valid = K.stage_inputs(B, T, frame, rot)
        xd, vd = _dev(x), _dev(valid)

        def run():
            y = Out(B * T, frame)
            _ok(ctx, ctx.lib.tn_dbg_stage_frames(ctx.handle, _ptr(xd), _ptr(vd), B, T, frame, y.ptr), "tn_dbg_stage_frames")
            return [y.read("stage_frames")]
        y = _twice(run)[0]
        _bits(y, R.stage_frames(x, valid), (rot, valid.tolist()))          # the NaN of a padded slot comes out as exactly +0


@pytest.mark.parametrize("rows,cols", K.TRANSPOSE_SHAPES)
def test_transpose(ctx, rows, cols):
    s = K.normal((rows, cols), 53, rows, cols)
    sd = _dev(s)

    def run():
        o = Out(cols, rows)
        _ok(ctx, ctx.lib.tn_dbg_transpose(ctx.handle, _ptr(sd), rows, cols, o.ptr), "tn_dbg_transpose")
        return [o.read("transpose")]
    _bits(_twice(run)[0], R.transpose(s), (rows, cols))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_every_hook_refuses_bad_arguments_and_works_afterwards(ctx):
    lib, h = ctx.lib, ctx.handle
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    src = torch.ones(4096, dtype=torch.float32, device="cuda")
    ints = torch.zeros(64, dtype=torch.int32, device="cuda")
    lab_ok, lab_hi, lab_lo = (np.array(v, np.int32) for v in ([0, 1], [0, 2], [-1, 1]))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    o1, o2, o3, o4 = nan(4096), nan(4096), nan(4096), torch.full((64,), INT_FILL, dtype=torch.int32, device="cuda")
    s, i, a, b, c, d = _ptr(src), _ptr(ints), _ptr(o1), _ptr(o2), _ptr(o3), _ptr(o4)
    off = lambda t: _ptr(t, 4)                             # 4 bytes past a 16-byte boundary
    # hook -> (the arguments of a good call after the context, [(position, bad value), ...])
    hooks = {
        "tn_dbg_ft_im2col7": ([s, 1, 2, 2, a], [(0, None), (4, None), (1, 0), (2, 0), (3, -2), (2, 3), (3, 1)]),
        "tn_dbg_ft_im2col3": ([s, 1, 2, 2, 4, s, s, a], [(0, None), (7, None), (5, None), (1, 0), (2, -1), (3, 0), (4, 0), (4, 6), (0, off(src)),
                                                        (7, off(o1)), (5, off(src)), (6, off(src))]),
        "tn_dbg_ft_col2im3": ([s, 1, 2, 2, 4, a], [(0, None), (5, None), (1, 0), (2, 0), (3, -1), (4, 0), (4, 2), (0, off(src)), (5, off(o1))]),
        "tn_dbg_ft_maxpool": ([s, 1, 2, 2, 3, a, 3, s, b], [(0, None), (7, None), (8, None), (1, 0), (2, 0), (3, 0), (4, 0), (6, 2), (2, 3), (3, 5)]),
        "tn_dbg_ft_avgpool2": ([s, 1, 2, 2, 3, a, 3, s, b], [(0, None), (5, None), (7, None), (8, None), (1, 0), (2, 0), (3, 0), (4, -3), (6, 2), (2, 1),
                                                           (3, 3)]),
        "tn_dbg_ft_gap": ([s, 2, 3, 4, a, s, b], [(0, None), (4, None), (5, None), (6, None), (1, 0), (2, 0), (3, -1)]),
        "tn_dbg_ft_bn_fold": ([s, s, s, s, 4, a, b], [(0, None), (1, None), (2, None), (3, None), (5, None), (6, None), (4, 0), (4, -4)]),
        "tn_dbg_ft_bn_running": ([a, b, s, s, 4], [(0, None), (1, None), (2, None), (3, None), (4, 0)]),
        "tn_dbg_pool_max_arg": ([s, 2, 3, 4, a, d, s, b], [(0, None), (4, None), (5, None), (6, None), (7, None), (1, 0), (2, 0), (3, -1)]),
        "tn_dbg_softmax_ce": ([s, i, hp(lab_ok), 2, 2, a, b], [(0, None), (1, None), (2, None), (5, None), (6, None), (3, 0), (4, 0), (2, hp(lab_hi)),
                                                             (2, hp(lab_lo))]),
        "tn_dbg_dense_bwd": ([s, s, s, 2, 3, 4, a, b, c], [(0, None), (1, None), (2, None), (6, None), (7, None), (8, None), (3, 0), (4, 0), (5, -1)]),
        "tn_dbg_colsum": ([s, 5, 3, 5, a], [(0, None), (4, None), (2, 0), (3, 0), (1, 4)]),
        "tn_dbg_sgd_momentum": ([a, s, b, 7, 0.01, 0.9, 1e-4, 1.0, None], [(0, None), (1, None), (2, None), (3, 0), (3, -7)]),
        "tn_dbg_adam": ([a, s, b, c, 7, 1e-3, 0.9, 0.999, 1e-8, 1, None], [(0, None), (1, None), (2, None), (3, None), (4, 0), (9, 0)]),
        "tn_dbg_stage_frames": ([s, i, 2, 3, 8, a], [(0, None), (1, None), (5, None), (2, 0), (3, 0), (4, 0), (4, 6), (4, -4)]),
        "tn_dbg_transpose": ([s, 3, 5, a], [(0, None), (3, None), (1, 0), (2, -5)]),
    }
    assert sorted(hooks) == sorted(n for n in _lib().declared_symbols() if n in hooks) and len(hooks) == 16
    outs = (o1, o2, o3, o4)
    snap = lambda: [t.view(torch.int32).clone() for t in outs]
    for name, (good, bads) in hooks.items():
        fn = getattr(lib, name)
        before = snap()
        assert fn(None, *good) == -1 and name in lib.tn_last_error().decode(), name          # no context
        for pos, val in bads:
            args = list(good)
            args[pos] = val
            rc = fn(h, *args)
            msg = lib.tn_last_error().decode()
            assert rc == -1, (name, pos, val, rc)          # TN_ERR_INVALID
            assert name in msg and len(msg) > len(name) + 10, (name, pos, msg)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(before, snap())), f"{name}: a refused call wrote to an output"
        for t in (o1, o2, o3):                             # the in-place hooks read their outputs
            t.fill_(1.0)
        assert fn(h, *good) == 0, (name, lib.tn_last_error().decode())
        torch.cuda.synchronize()
        assert torch.isfinite(o1).all()
        for t in (o1, o2, o3):
            t.fill_(float("nan"))
        o4.fill_(INT_FILL)
