"""The float64 references of the training steps' operator kernels (oracle/train_ops_np.py), pinned against float64 torch on the
CPU at the shapes and inputs the GPU tests use (tests/tools/train_ops_cases.py): F.unfold, the pools and the dense layer through
autograd, F.cross_entropy(reduction="none") through autograd, F.batch_norm, and two hand-written optimiser steps.

Ties.  The references send a tied maximum's gradient to the FIRST maximum in scan order, which is the kernels' documented rule.
torch does not promise a rule, so on tie-rich data the references are pinned against plain loops that state the rule, and torch is
compared only where a window's maximum is unique (test_maxpool_ties_*, test_pool_max_arg_ties_*); on this torch build the CPU
max_pool2d backward happens to follow the same rule, which test_maxpool_ties_follow_first_in_scan_order reports without relying on it.

The inputs' own properties (closed ReLUs, tied windows, no pre-activation within one rounding of zero) are asserted here too."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train_ops_np as R
from tools import train_ops_cases as K

T64 = torch.float64
TOL = 1e-12            # float64 against float64, sums of at most a few thousand terms of size <= 1e6


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    return t.requires_grad_(True) if grad else t


def _nchw(a, grad=False):
    return _t(np.transpose(np.asarray(a, dtype=np.float64), (0, 3, 1, 2)), grad)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def _close(got, ref, tol=TOL):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= tol * max(1.0, float(np.abs(ref).max())), err


def _unfold(a, k, stride, pad):
    """F.unfold's (B, C k k, L) with rows (c, ky, kx) -> (B L, k k C) with columns (ky, kx, c)"""
    B, H, W, C = a.shape
    u = F.unfold(_nchw(a), k, padding=pad, stride=stride)
    return u.reshape(B, C, k, k, -1).permute(0, 4, 2, 3, 1).reshape(-1, k * k * C).numpy()


@pytest.mark.parametrize("B,H,W", K.IM2COL7_SHAPES)
def test_im2col7_matches_unfold(B, H, W):
    x = K.normal((B, H, W, 3), 1, B, H, W)
    got = R.im2col7(x)
    assert got.shape == (B * (H // 2) * (W // 2), 147)
    assert np.array_equal(got, _unfold(x, 7, 2, 3))


@pytest.mark.parametrize("C", K.IM2COL3_C)
@pytest.mark.parametrize("B,H,W", K.IM2COL3_SHAPES)
def test_im2col3_and_its_adjoint_match_unfold(B, H, W, C):
    a, sc, sh = K.fold_inputs(B, H, W, C)
    assert np.array_equal(R.im2col3(a), _unfold(a, 3, 1, 1))
    folded = torch.relu(_t(a) * _t(sc) + _t(sh)).numpy()
    assert np.array_equal(R.im2col3(a, sc, sh), _unfold(folded, 3, 1, 1))
    # the adjoint: the gradient of <unfold(a), d> with respect to a
    d = K.integers((B * H * W, 9 * C), -3, 3, 2, B, H, W, C)
    at = _nchw(a, grad=True)
    u = F.unfold(at, 3, padding=1).reshape(B, C, 3, 3, -1).permute(0, 4, 2, 3, 1).reshape(-1, 9 * C)
    (u * _t(d)).sum().backward()
    assert np.array_equal(R.col2im3(d, B, H, W, C), _nhwc(at.grad))
    assert (R.im2col3(a) * d).sum() == pytest.approx((a.astype(np.float64) * R.col2im3(d, B, H, W, C)).sum(), rel=1e-12)


@pytest.mark.parametrize("C", K.IM2COL3_C)
@pytest.mark.parametrize("B,H,W", K.IM2COL3_SHAPES)
def test_fold_inputs_close_relus_and_stay_clear_of_zero(B, H, W, C):
    a, sc, sh = K.fold_inputs(B, H, W, C)
    below, above, ambiguous = K.fold_fractions(a, sc, sh)
    assert below >= 0.25 and above >= 0.25, (below, above)
    assert (sc < 0).any() and (sc == 0).any()
    assert ambiguous == 0               # no pre-activation that one rounding could move across zero: the reference alone gives none
    ref = R.im2col3(a, sc, sh)
    assert (ref == 0).mean() >= 0.25    # closed ReLUs (and padding) reach the matrix


def _maxpool_loops(a, dy):
    """the rule, stated with loops: -inf padding; the first maximum in (ky, kx) order takes the window's gradient"""
    B, H, W, C = a.shape
    Ho, Wo = H // 2, W // 2
    y, da = np.empty((B, Ho, Wo, C)), np.zeros((B, H, W, C))
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for c in range(C):
                    best, at = -np.inf, None
                    for ky in range(3):
                        for kx in range(3):
                            iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                            if 0 <= iy < H and 0 <= ix < W and a[b, iy, ix, c] > best:
                                best, at = a[b, iy, ix, c], (iy, ix)
                    y[b, oy, ox, c] = best
                    da[b, at[0], at[1], c] += dy[b, oy, ox, c]
    return y, da


def _maxpool_torch(a, dy):
    at = _nchw(a, grad=True)
    y = F.max_pool2d(at, 3, 2, 1)
    y.backward(_nchw(dy))
    return _nhwc(y), _nhwc(at.grad)


@pytest.mark.parametrize("kind", K.POOL_KINDS)
@pytest.mark.parametrize("B,H,W", K.POOL_SHAPES)
def test_maxpool_matches_torch_and_the_rule(B, H, W, kind):
    C = 3
    a = K.pool_input(kind, B, H, W, C)
    dy = K.integers((B, H // 2, W // 2, C), -3, 3, 4, B, H, W)
    y, da = R.maxpool(a), R.maxpool_bwd(a, dy)
    ty, tda = _maxpool_torch(a, dy)
    assert np.array_equal(y, ty)
    if kind == "negative":
        assert (y < 0).all()            # a zero from the padding would have won
    if kind == "random":                # unique maxima: torch's routing is defined
        assert np.array_equal(da, tda)
    if B * H * W <= 200:
        ly, lda = _maxpool_loops(a.astype(np.float64), dy.astype(np.float64))
        assert np.array_equal(y, ly) and np.array_equal(da, lda)
    assert np.array_equal(da.sum(axis=(1, 2)), dy.astype(np.float64).sum(axis=(1, 2)))


def test_maxpool_ties_follow_first_in_scan_order(capsys):
    a = K.pool_input("ties", 2, 4, 6, 3)
    assert K.tied_window_fraction(a) >= 0.3
    dy = K.integers((2, 2, 3, 3), 1, 3, 4, 0)
    da = R.maxpool_bwd(a, dy)
    _, lda = _maxpool_loops(a.astype(np.float64), dy.astype(np.float64))
    assert np.array_equal(da, lda)
    one = K.pool_input("ties", 1, 2, 2, 3)                # one window; pixels (0, 0) and (1, 1) tie at 3: the first takes it
    g1 = R.maxpool_bwd(one, np.full((1, 1, 1, 3), 5.0))
    assert (g1[0, 0, 0] == 5).all() and g1.sum() == 15
    _, tda = _maxpool_torch(a, dy)
    with capsys.disabled():
        print(f"\n  torch CPU max_pool2d backward routes tied windows {'as' if np.array_equal(da, tda) else 'NOT as'} first-in-scan-order")
    eq = K.pool_input("equal", 1, 4, 6, 1)
    g =R.maxpool_bwd(eq, np.ones((1, 2, 3, 1)))[0, :, :, 0]
    # all equal: window (oy, ox) starts at (2 oy - 1, 2 ox - 1) clipped to the frame, and its first pixel takes the gradient
    want = np.zeros((4, 6))
    for oy in range(2):
        for ox in range(3):
            want[max(2 * oy - 1, 0), max(2 * ox - 1, 0)] += 1
    assert np.array_equal(g, want)


@pytest.mark.parametrize("B,H,W", K.POOL_SHAPES)
def test_avgpool2_and_gap_match_torch(B, H, W):
    C = 3
    z = K.normal((B, H, W, C), 14, B, H, W)
    dy = K.normal((B, H // 2, W // 2, C), 15, B, H, W)
    zt = _nchw(z, grad=True)
    y = F.avg_pool2d(zt, 2, 2)
    y.backward(_nchw(dy))
    _close(R.avgpool2(z), _nhwc(y))
    _close(R.avgpool2_bwd(dy), _nhwc(zt.grad))


@pytest.mark.parametrize("B,P,C", K.GAP_SHAPES)
def test_gap_matches_torch(B, P, C):
    a = K.normal((B, P, C), 16, B, P, C)
    df = K.normal((B, C), 17, B, P, C)
    at = _t(a.reshape(B, P, 1, C).transpose(0, 3, 1, 2), grad=True)        # (B, C, P, 1)
    f = F.adaptive_avg_pool2d(at, 1).reshape(B, C)
    f.backward(_t(df))
    _close(R.gap(a), f.detach().numpy())
    _close(R.gap_bwd(df, P), at.grad.permute(0, 2, 3, 1).reshape(B, P, C).numpy())


@pytest.mark.parametrize("C", K.BN_C)
def test_bn_fold_and_running_match_batch_norm(C):
    mean, var, gamma, beta, rmean, rvar = K.bn_inputs(C)
    assert set(np.unique(var)) <= {np.float32(0), np.float32(1e-12), np.float32(1), np.float32(1e6)}
    assert (gamma < 0).any() and (C < 5 or (gamma == 0).any()) and np.abs(mean).max() == 50
    sc, sh = R.bn_fold(mean, var, gamma, beta)
    x = K.normal((6, C), 18, C).astype(np.float64) * 3 + mean
    y = F.batch_norm(_t(x), _t(mean), _t(var), _t(gamma), _t(beta), False, 0.0, R.BN_EPS).numpy()
    ref = x * sc + sh
    assert np.abs(ref - y).max() <= 1e-9 * max(1.0, np.abs(y).max())        # (x - mean) sc + beta against x sc + (beta - mean sc)
    # running statistics: torch's momentum is the weight of the batch (0.1), and it feeds the unbiased batch variance
    rm, rv = _t(rmean), _t(rvar)
    F.batch_norm(_t(x), rm, rv, None, None, True, 1.0 - R.BN_MOMENTUM, R.BN_EPS)
    got_m, got_v = R.bn_running(rmean, rvar, x.mean(axis=0), x.var(axis=0, ddof=1))
    _close(got_m, rm.numpy(), 1e-12)
    _close(got_v, rv.numpy(), 1e-12)


@pytest.mark.parametrize("kind", ("ties", "random"))
@pytest.mark.parametrize("B,T,F_", K.POOLT_SHAPES)
def test_pool_max_arg_and_scatter(B, T, F_, kind):
    x = K.poolt_input(kind, B, T, F_)
    dp = K.integers((B, F_), -3, 3, 19, B, T, F_)
    y, arg = R.pool_max_arg(x)
    ds = R.scatter_pool_grad(dp, arg, T)
    if kind == "ties" and T > 1:
        assert K.tied_column_fraction(x) >= 0.3
        assert (arg[:, ::2] == 0).all()                   # first and last step tie: the first takes it
    # the rule, with loops
    for b in range(B):
        for f in range(0, F_, max(1, F_ // 7)):
            col = x[b, :, f].tolist()
            assert y[b, f] == max(col) and arg[b, f] == col.index(max(col))
    xt = _t(x, grad=True)
    ty, targ = xt.max(dim=1)
    ty.backward(_t(dp))
    assert np.array_equal(y, ty.detach().numpy())
    if kind == "random":                                  # unique maxima: torch's routing is defined
        assert np.array_equal(arg, targ.numpy()) and np.array_equal(ds, xt.grad.numpy())
    assert np.array_equal(ds.sum(axis=1), dp.astype(np.float64))
    assert ((ds != 0).sum(axis=1) <= 1).all()


@pytest.mark.parametrize("B,C", K.CE_SHAPES)
def test_softmax_ce_matches_cross_entropy(B, C):
    for rot in range(len(K.CE_KINDS) if B < len(K.CE_KINDS) else 1):
        p, labels = K.ce_inputs(B, C, rot)
        if B >= C:
            assert set(labels.tolist()) == set(range(C))
        assert labels.min() >= 0 and labels.max() < C
        pt = _t(p, grad=True)
        lt = F.cross_entropy(pt, torch.from_numpy(labels.astype(np.int64)), reduction="none")
        lt.sum().backward()
        loss, d = R.softmax_ce(p, labels)
        # float64 on both sides; 1e4-sized logits leave about 1e4 * 2^-53 of absolute error in either
        assert np.abs(loss - lt.detach().numpy()).max() <= 1e-11
        assert np.abs(d - pt.grad.numpy()).max() <= 1e-11
        assert (loss >= 0).all() and np.abs(d.sum(axis=1)).max() <= 1e-12
    kinds = {K.CE_KINDS[(b + r) % 6] for r in range(6 if B < 6 else 1) for b in range(B)}
    assert kinds == set(K.CE_KINDS)
    if C >= 11:
        p, _ = K.ce_inputs(max(B, 6), C, 0)
        e = np.exp(p[4].astype(np.float64) - p[4].max())
        assert (e < 2.0 ** -149).any()                   # the spread row: some probabilities underflow float32


@pytest.mark.parametrize("B,C,Kd", K.DENSE_SHAPES)
def test_dense_bwd_and_colsum_match_autograd(B, C, Kd):
    d = K.normal((B, C), 20, B, C, Kd)
    x, w = K.normal((B, Kd), 21, B, C, Kd), K.normal((C, Kd), 22, B, C, Kd)
    xt, wt, bt = _t(x, grad=True), _t(w, grad=True), torch.zeros(C, dtype=T64, requires_grad=True)
    (F.linear(xt, wt, bt) * _t(d)).sum().backward()
    dw, db, dx = R.dense_bwd(d, x, w)
    _close(dw, wt.grad.numpy())
    _close(db, bt.grad.numpy())
    _close(dx, xt.grad.numpy())
    _close(R.colsum(d), bt.grad.numpy())


def test_optimisers_match_hand_written_steps():
    lr, mo, wd, rs = (float(np.float32(v)) for v in (0.01, 0.9, 1e-4, 1.0 / 32))
    b1, b2, eps = (float(np.float32(v)) for v in (0.9, 0.999, 1e-8))
    for n in (1, 257):
        w, g, m, v = K.opt_inputs(n)
        assert n < 4 or ((g == 0).any() and np.abs(g).max() == 1e6 and np.abs(g[g != 0]).min() <= 1e-12)
        for scale in (1.0, K.CLIP_SCALE):
            # MXNet sgd_mom_update, twice
            W_, M_ = _t(w), _t(m)
            rw, rm = w, m
            for _ in range(2):
                M_ = mo * M_ - lr * (rs * scale * _t(g) + wd * W_)
                W_ = W_ + M_
                rw, rm = R.sgd_momentum(rw, g, rm, lr, mo, wd, rs, scale)
            _close(rw, W_.numpy())
            _close(rm, M_.numpy())
            # MXNet adam_update at update counts 1 and 2: the rate carries the bias correction
            W_, M_, V_ = _t(w), _t(m), _t(v)
            rw, rm, rv = w, m, v
            for t in (1, 2):
                gt = scale * _t(g)
                M_ = b1 * M_ + (1 - b1) * gt
                V_ = b2 * V_ + (1 - b2) * gt * gt
                W_ = W_ - 1e-3 * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * M_ / (V_.sqrt() + eps)
                rw, rm, rv = R.adam(rw, g, rm, rv, R.adam_rate(1e-3, b1, b2, t), b1, b2, eps, scale)
            _close(rw, W_.numpy())
            _close(rm, M_.numpy())
            _close(rv, V_.numpy())
    assert R.adam_rate(1e-3, 0.9, 0.999, 10 ** 6) == pytest.approx(1e-3, rel=1e-12)       # both corrections are gone by then


@pytest.mark.parametrize("B,T,frame", K.STAGE_SHAPES[:3])
def test_stage_frames_and_transpose(B, T, frame):
    for rot in range(4):
        x, valid = K.stage_inputs(B, T, frame, rot)
        y = R.stage_frames(x, valid)
        assert np.isfinite(y).all()
        for b in range(B):
            n = min(int(valid[b]), T)
            assert np.array_equal(y[b, :n], x[b, :n].astype(np.float64)) and not y[b, n:].any()
    assert {int(v) for r in range(4) for v in K.stage_inputs(B, T, frame, r)[1]} == {0, 1, T, T + 2}
    s = K.normal((B * T, 5), 23, B, T)
    assert np.array_equal(R.transpose(s), _t(s).t().numpy())
