"""-m gpu: the fp32x3 matrix mode of the backbone training steps (TN_MATMUL_FP32X3, csrc/gemm_fp32x3.hip).

The two kernels through their hooks (tn_dbg_linear_fp32x3, tn_dbg_gemm_tn_fp32x3) against float64 with the project's fp32x3 kernel
bound, 5e-7 of sum_k |a||b| per output (tests/test_gpu_fp32x3_mode.py: the fp32 chain itself sits at 1.5 - 2.5e-7 of that sum; the
bound covers the operand transform's single fp32 rounding, 6e-8), the f32 hooks' error on the same operands recorded beside it;
then the three trainers with matmul="fp32x3" against the float64 autograd oracles with the parameters, inputs and bars of
tests/test_gpu_finetune.py, tests/test_gpu_cnnrnn_train.py and tests/test_gpu_gnmt_frames_train.py (helpers copied).  Every oracle
step is computed once and shared."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import densenet_train_torch as dt
from oracle import train_np as tn

pytestmark = pytest.mark.gpu

KERNEL_BOUND = 5e-7
U = 2.0 ** -24            # one fp32 rounding, relative
STOCK_BNS = ("densenet0_batchnorm0", "densenet0_stage1_batchnorm1", "densenet0_stage3_batchnorm47", "densenet0_batchnorm4")
TIGHT_GRADS = ("framemodel0_dense0_weight", "framemodel0_dense0_bias", "densenet0_stage4_conv31_weight", "densenet0_stage4_conv30_weight")
SENTINEL = -12345.678


def _L():
    from tennis_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx():
    return _L().default_context()


def _cap_threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else C.c_void_p(None)


# ---- 1. the NT kernel --------------------------------------------------------------------------------------------------------------

def _nt_operands(M, N, K, ldx, ldw, bn, seed, xoff=0):
    """X = +-relu(3 N(0,1) + 0.5) (bn: x ~ N(0,1) with |asc| ~ 3, |ash| ~ 0.5, both signs), W = 0.05 N(0,1); the strides' padding is
    filled with large values that a read past K would pick up.  -> flat x buffer (xoff floats of lead), w, asc, ash, float64 f(X), W"""
    rng = np.random.default_rng([M, N, K, seed])
    xbuf = np.full(xoff + M * ldx, 1e6, np.float32)
    x = xbuf[xoff:].reshape(M, ldx)
    w = np.full((N, ldw), 1e6, np.float32)
    w[:, :K] = (0.05 * rng.standard_normal((N, K))).astype(np.float32)
    if bn:
        x[:, :K] = rng.standard_normal((M, K)).astype(np.float32)
        asc = (rng.uniform(2.0, 4.0, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32)
        ash = (rng.uniform(0.25, 0.75, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32)
        f64 = np.maximum(x[:, :K].astype(np.float64) * asc.astype(np.float64) + ash.astype(np.float64), 0.0)
    else:
        asc = ash = None
        x[:, :K] = (np.maximum(3.0 * rng.standard_normal((M, K)) + 0.5, 0.0) * rng.choice([-1.0, 1.0], (M, K))).astype(np.float32)
        f64 = x[:, :K].astype(np.float64)
    return xbuf, w, asc, ash, f64, w[:, :K].astype(np.float64)


def _run_nt(ctx, hook, xbuf, xoff, ldx, asc, ash, w, M, N, K, ldy, yoff, accumulate, y0):
    """one hook call on a (M, ldy) buffer holding y0, the output at column offset yoff; -> the whole buffer afterwards"""
    L = _L()
    xd, wd, yd = _dev(xbuf), _dev(w), _dev(y0)
    ad, hd = (_dev(asc), _dev(ash)) if asc is not None else (None, None)
    L.check(getattr(ctx.lib, hook)(ctx.handle, _p(xd, xoff), ldx, _p(ad), _p(hd), _p(wd), w.shape[1], None, _p(yd, yoff), ldy, M, N, K,
                                   accumulate), hook)
    return yd.cpu().numpy()


# (M, N, K, ldx, ldy, bn, column offset of the output, float offset of X, accumulate)
NT_CASES = [(1, 1, 1, 1, 1, False, 0, 0, 0),
            (33, 33, 33, 35, 35, False, 0, 0, 0),
            (98, 128, 64, 256, 128, True, 0, 0, 0),
            (98, 32, 1152, 1152, 1024, False, 992, 0, 0),           # the 32 new channels at the end of a block's concat buffer
            (129, 40, 1000, 1024, 40, True, 0, 0, 0),
            (257, 1024, 128, 128, 1024, False, 0, 0, 0),
            (27, 1152, 32, 32, 1152, False, 0, 0, 0),
            (6912, 64, 147, 147, 64, False, 0, 1, 0),               # the stem: rows of 588 bytes, X one float off 16 bytes
            (131, 96, 200, 203, 101, True, 0, 0, 1)]                # accumulate


@pytest.mark.parametrize("case", NT_CASES, ids=["%dx%dx%d" % c[:3] for c in NT_CASES])
def test_nt_kernel_against_float64(ctx, report, case):
    M, N, K, ldx, ldy, bn, yoff, xoff, accumulate = case
    ldw = K if not bn else K + 3
    xbuf, w, asc, ash, f64, w64 = _nt_operands(M, N, K, ldx, ldw, bn, 1, xoff)
    ref, sab = f64 @ w64.T, np.abs(f64) @ np.abs(w64).T
    rng = np.random.default_rng(7)
    y0 = np.full((M, ldy), SENTINEL, np.float32)
    if accumulate:
        y0[:, yoff:yoff + N] = rng.standard_normal((M, N)).astype(np.float32)
        ref = ref + y0[:, yoff:yoff + N]
    # the product's bound; accumulate: plus the one rounding of y0 + v
    bound = KERNEL_BOUND * sab + (U * np.abs(ref) if accumulate else 0.0)
    got = _run_nt(ctx, "tn_dbg_linear_fp32x3", xbuf, xoff, ldx, asc, ash, w, M, N, K, ldy, yoff, accumulate, y0)
    keep = np.ones((M, ldy), bool)
    keep[:, yoff:yoff + N] = False
    assert np.array_equal(got.view(np.uint32)[keep], y0.view(np.uint32)[keep]), "written outside [0, M) x [0, N)"
    out = got[:, yoff:yoff + N].astype(np.float64)
    assert np.isfinite(out).all()
    ratio = float((np.abs(out - ref) / np.maximum(sab, 1e-300)).max())
    # the f32 kernel on the same operands, recorded
    L = _L()
    if bn:
        f32 = _run_nt(ctx, "tn_dbg_linear_bnrelu", xbuf, xoff, ldx, asc, ash, w, M, N, K, ldy, yoff, accumulate, y0)[:, yoff:yoff + N]
    else:
        xc, wc = _dev(xbuf[xoff:].reshape(M, ldx)[:, :K]), _dev(w[:, :K])
        yc = torch.empty((M, N), dtype=torch.float32, device="cuda")
        L.check(ctx.lib.tn_dbg_linear(ctx.handle, _p(xc), _p(wc), None, _p(yc), M, N, K), "tn_dbg_linear")
        ctx.sync()
        f32 = yc.cpu().numpy()
    ratio32 = float((np.abs(f32.astype(np.float64) - ref) / np.maximum(sab, 1e-300)).max())
    key = "matmul_nt_%dx%dx%d" % (M, N, K)
    report[key + "_fp32x3_err_over_sab"], report[key + "_f32_err_over_sab"] = ratio, ratio32
    report["matmul_fp32x3_kernel_err_over_sab_worst"] = max(ratio, report.get("matmul_fp32x3_kernel_err_over_sab_worst", 0.0))
    print("NT %s: fp32x3 %.3e  f32 %.3e of sum|a||b|" % (key, ratio, ratio32))
    assert (np.abs(out - ref) <= bound).all(), (key, ratio)


# ---- 2. the TN kernel --------------------------------------------------------------------------------------------------------------

def _tn_operands(M, N, K, lda, ldb, bn, seed):
    """A = 0.05 N(0,1) (the gradient side), B = +-relu(3 N(0,1) + 0.5) (bn: N(0,1) through relu(b bsc[n] + bsh[n]))"""
    rng = np.random.default_rng([M, N, K, seed])
    a = np.full((K, lda), 1e6, np.float32)
    b = np.full((K, ldb), 1e6, np.float32)
    a[:, :M] = (0.05 * rng.standard_normal((K, M))).astype(np.float32)
    if bn:
        b[:, :N] = rng.standard_normal((K, N)).astype(np.float32)
        bsc = (rng.uniform(2.0, 4.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
        bsh = (rng.uniform(0.25, 0.75, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
        g64 = np.maximum(b[:, :N].astype(np.float64) * bsc.astype(np.float64) + bsh.astype(np.float64), 0.0)
    else:
        bsc = bsh = None
        b[:, :N] = (np.maximum(3.0 * rng.standard_normal((K, N)) + 0.5, 0.0) * rng.choice([-1.0, 1.0], (K, N))).astype(np.float32)
        g64 = b[:, :N].astype(np.float64)
    return a, b, bsc, bsh, a[:, :M].astype(np.float64), g64


def _run_tn(ctx, hook, ad, bd, scd, shd, M, N, K, ldc, ws_floats):
    L = _L()
    out = torch.full((M, ldc), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.empty(ws_floats, dtype=torch.float32, device="cuda") if ws_floats else None
    L.check(getattr(ctx.lib, hook)(ctx.handle, _p(ad), ad.shape[1], _p(bd), bd.shape[1], _p(scd), _p(shd), _p(out), ldc, M, N, K, _p(ws),
                                   ws_floats), hook)
    return out.cpu().numpy()


WS_STEP = 16 << 20
# (M, N, rows, lda, ldb, bn, workspaces)
TN_CASES = [(1, 1, 4097, 1, 1, False, (WS_STEP,)),
            (33, 35, 1, 33, 35, False, (WS_STEP,)),
            (32, 1152, 98, 32, 1152, False, (WS_STEP,)),
            (128, 992, 98, 128, 1024, True, (WS_STEP,)),
            (64, 147, 6912, 64, 147, False, (WS_STEP,)),
            (512, 1024, 588, 512, 1024, False, (WS_STEP,)),
            (32, 1152, 25088, 32, 1152, False, (WS_STEP, 32 * 1152 + 5, 0))]     # split 29 ways, too small for any split, none


@pytest.mark.parametrize("case", TN_CASES, ids=["%dx%dx%d" % c[:3] for c in TN_CASES])
def test_tn_kernel_against_float64(ctx, report, case):
    M, N, K, lda, ldb, bn, workspaces = case
    a, b, bsc, bsh, a64, g64 = _tn_operands(M, N, K, lda, ldb, bn, 2)
    ref, sab = a64.T @ g64, np.abs(a64).T @ np.abs(g64)
    ad, bd = _dev(a), _dev(b)
    scd, shd = (_dev(bsc), _dev(bsh)) if bn else (None, None)
    ldc = N + 3
    key = "matmul_tn_%dx%dx%d" % (M, N, K)
    for ws in workspaces:
        got = _run_tn(ctx, "tn_dbg_gemm_tn_fp32x3", ad, bd, scd, shd, M, N, K, ldc, ws)
        assert (got[:, N:] == np.float32(SENTINEL)).all(), "columns past N written"
        out = got[:, :N].astype(np.float64)
        assert np.isfinite(out).all()
        ratio = float((np.abs(out - ref) / np.maximum(sab, 1e-300)).max())
        report["%s_ws%d_fp32x3_err_over_sab" % (key, ws)] = ratio
        report["matmul_fp32x3_kernel_err_over_sab_worst"] = max(ratio, report.get("matmul_fp32x3_kernel_err_over_sab_worst", 0.0))
        print("TN %s ws %d: fp32x3 %.3e of sum|a||b|" % (key, ws, ratio))
        assert (np.abs(out - ref) <= KERNEL_BOUND * sab).all(), (key, ws, ratio)
        if ws == WS_STEP:                          # the same workspace again: the same bits
            again = _run_tn(ctx, "tn_dbg_gemm_tn_fp32x3", ad, bd, scd, shd, M, N, K, ldc, ws)
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "a repeated call gave other bits"
    f32 = _run_tn(ctx, "tn_dbg_gemm_tn", ad, bd, scd, shd, M, N, K, ldc, WS_STEP)[:, :N].astype(np.float64)
    report[key + "_f32_err_over_sab"] = float((np.abs(f32 - ref) / np.maximum(sab, 1e-300)).max())


# ---- 3. exactness: integer operands of one bf16 term each -------------------------------------------------------------------------------

@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("M,N,K", [(37, 70, 13), (130, 33, 63), (5, 129, 41)])
def test_integer_operands_are_exact(ctx, M, N, K, bn):
    """|values| <= 256 are single bf16 terms and every sum stays below 2^24: the result is the integer sum, bit for bit.  A dropped,
    doubled or misplaced k-slot, a swapped plane or a padded slot that is not 0 (bn: ash > 0, so relu(0 sc + sh) > 0) shows."""
    rng = np.random.default_rng([M, N, K, int(bn)])
    ia = rng.integers(-60, 61, (M, K))                       # the transformed side, before the transform
    iw = rng.integers(-256, 257, (N, K))
    sc = rng.choice([-2, -1, 1, 2], K)
    sh = rng.integers(1, 9, K)
    fa = np.maximum(ia * sc + sh, 0) if bn else ia           # |fa| <= 128
    # NT: Y = f(X) W^T, strides with a sentinel behind K
    ldx, ldw = K + 5, K + 2
    x = np.full((M, ldx), 999.0, np.float32); x[:, :K] = ia
    w = np.full((N, ldw), 999.0, np.float32); w[:, :K] = iw
    y0 = np.full((M, N + 1), SENTINEL, np.float32)
    got = _run_nt(ctx, "tn_dbg_linear_fp32x3", x.reshape(-1), 0, ldx, sc.astype(np.float32) if bn else None,
                  sh.astype(np.float32) if bn else None, w, M, N, K, N + 1, 0, 0, y0)
    assert np.array_equal(got[:, :N].astype(np.int64), fa @ iw.T) and (got[:, N] == np.float32(SENTINEL)).all()
    # TN: C = A^T g(B) over K rows: A (K, M) the plain side, B (K, N) the transformed one (per column n)
    ib = rng.integers(-60, 61, (K, N))
    ja = rng.integers(-256, 257, (K, M))
    scn, shn = rng.choice([-2, -1, 1, 2], N), rng.integers(1, 9, N)
    gb = np.maximum(ib * scn + shn, 0) if bn else ib
    a = np.full((K, M + 3), 999.0, np.float32); a[:, :M] = ja
    b = np.full((K, N + 1), 999.0, np.float32); b[:, :N] = ib
    scd, shd = (_dev(scn.astype(np.float32)), _dev(shn.astype(np.float32))) if bn else (None, None)
    got = _run_tn(ctx, "tn_dbg_gemm_tn_fp32x3", _dev(a), _dev(b), scd, shd, M, N, K, N + 2, WS_STEP)
    assert np.array_equal(got[:, :N].astype(np.int64), ja.T @ gb) and (got[:, N:] == np.float32(SENTINEL)).all()


# ---- 4. exponent range ---------------------------------------------------------------------------------------------------------------

def test_exponent_range(ctx, report):
    """(98, 128, 64) with column k of f(X) scaled by 2^e_k and of W by 2^-e_k, e_k uniform in [-30, 30] (exact scalings: asc and ash
    both carry 2^e_k): every product is what it was, so is the bound - bf16 has fp32's exponent range, nothing is scaled inside"""
    M, N, K, ldx = 98, 128, 64, 256
    xbuf, w, asc, ash, f64, w64 = _nt_operands(M, N, K, ldx, K, True, 4)
    e = np.random.default_rng(4).integers(-30, 31, K)
    up, down = np.ldexp(1.0, e), np.ldexp(1.0, -e)
    asc2, ash2 = (asc * up).astype(np.float32), (ash * up).astype(np.float32)
    w2 = (w * down[None, :]).astype(np.float32)
    ref, sab = f64 @ w64.T, np.abs(f64) @ np.abs(w64).T
    y0 = np.full((M, N), SENTINEL, np.float32)
    out = _run_nt(ctx, "tn_dbg_linear_fp32x3", xbuf, 0, ldx, asc2, ash2, w2, M, N, K, N, 0, 0, y0).astype(np.float64)
    ratio = float((np.abs(out - ref) / sab).max())
    report["matmul_nt_exponent_range_err_over_sab"] = ratio
    assert (np.abs(out - ref) <= KERNEL_BOUND * sab).all(), ratio


# ---- 5.-7. the fine-tuning step ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _setup(B, size=224, seed=5, shift=0.0):
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(0)
    p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
    if shift:
        p = {k: (v + shift).astype(np.float32) if k.endswith("_beta") else v for k, v in p.items()}
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(B, size, seed))
    y = np.random.default_rng(seed).integers(0, 11, B).astype(np.int32)
    return p, x, y


@functools.lru_cache(maxsize=None)
def _oracle(B, size=224, seed=5, shift=0.0):
    """the float64 autograd step, and how many ReLU inputs of it are not positive (0 = every ReLU open)"""
    _cap_threads()
    p, x, y = _setup(B, size, seed, shift)
    closed = [0]
    relu = dt.F.relu

    def counting_relu(t, *a, **k):
        closed[0] += int((t <= 0).sum())
        return relu(t, *a, **k)

    dt.F.relu = counting_relu
    try:
        out = dt.loss_and_grads(p, x, y)
    finally:
        dt.F.relu = relu
    return out + (closed[0],)


def _compare(tr, rg):
    """per parameter: max-abs error relative to the largest reference entry (floored at 1e-3 of the largest gradient entry of the whole
    model) and cosine similarity of the non-negligible ones (tests/test_gpu_finetune.py)"""
    floor = 1e-3 * max(np.abs(g).max() for g in rg.values())
    worst, worst_k, min_cos = 0.0, None, 1.0
    for k, g in rg.items():
        got = tr.get(k, gradient=True).astype(np.float64)
        err = np.abs(got - g).max() / max(floor, np.abs(g).max())
        if np.abs(g).max() > floor:
            min_cos = min(min_cos, float((got * g).sum() / max(1e-30, np.linalg.norm(got) * np.linalg.norm(g))))
        if err > worst:
            worst, worst_k = err, k
    return worst, worst_k, min_cos


def _open_relu_step(report, tag, B, size, shift, all_open=False):
    from tennis_amd.engine import FrameModelTrainer
    p, x, y = _setup(B, size, 5, shift)
    rl, rlog, rg, rstats, closed = _oracle(B, size, 5, shift)
    if all_open:              # checked on the CPU before anything runs on the device
        assert closed == 0, f"{closed} ReLU inputs of the float64 oracle are not positive at shift {shift}: raise the shift"
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = {}
    for mode in ("f32", "fp32x3"):
        tr = FrameModelTrainer(p, size, 11, batch=B, matmul=mode)
        assert tr.matmul == mode
        loss, logits = tr.forward_backward(xd, yd)
        el = float(np.abs(logits.cpu().numpy() - rlog).max() / max(1.0, np.abs(rlog).max()))
        worst, worst_k, min_cos = _compare(tr, rg)
        res[mode] = (el, worst, worst_k, min_cos, tr.matmul_stats())
        report[f"finetune_matmul{tag}_{mode}_open_relu_logits_rel_err"] = el
        report[f"finetune_matmul{tag}_{mode}_open_relu_grad_rel_err_worst"] = float(worst)
        report[f"finetune_matmul{tag}_{mode}_open_relu_grad_min_cosine"] = float(min_cos)
        print(f"open ReLU {size}x{B} {mode}: logits {el:.3e} worst grad {worst:.3e} ({worst_k}) min cosine {min_cos:.9f}")
        del tr
    assert res["f32"][4] == (359, 0) and res["fp32x3"][4] == (0, 359), (res["f32"][4], res["fp32x3"][4])
    el, worst, worst_k, min_cos, _ = res["fp32x3"]
    assert el < 1e-3
    assert worst < 2e-3 and min_cos > 0.999999, (worst_k, worst, min_cos)


def test_step_open_relus_224(report):
    """224 x 224, 2 frames, every beta + 4: all 364 gradients of the fp32x3 step against float64 autograd with the f32 step's bars
    (logits 1e-3 relative, worst gradient error < 2e-3, cosine > 0.999999); 120 + 239 launches, all in the mode's counter"""
    _open_relu_step(report, "", 2, 224, 4.0)


def test_step_tails_96(report):
    """96 x 96, 3 frames: maps of 24 / 12 / 6 / 3, so 27 rows in block 4 and row counts off every tile (6912, 1728, 432, 108, 27).
    The float64 oracle is first checked, on the CPU, to have no ReLU input <= 0 in any BatchNorm channel.  With every beta + 4 it
    has 1876 of them at this size (+ 6: 16), so the shift is raised to + 8 as the 512 x 512 test does, where it has none; the
    bars stay those of the 224 x 224 test."""
    _open_relu_step(report, "_96x3", 3, 96, 8.0, all_open=True)


def test_step_stock_224(report):
    """the stock-parameter step at 224 x 224 x 2 in fp32x3 with the bars of tests/test_gpu_finetune.py::_stock_checks; the f32
    trainer's figures on the same batch recorded beside them"""
    from tennis_amd.engine import FrameModelTrainer
    B, size = 2, 224
    p, x, y = _setup(B, size)
    rl, rlog, rg, rstats, _ = _oracle(B, size)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    f32 = FrameModelTrainer(p, size, 11, batch=B)
    assert f32.matmul == "f32"
    f32.forward_backward(xd, yd)
    w32, _, c32 = _compare(f32, rg)
    report["finetune_matmul_f32_stock_grad_rel_err_worst"], report["finetune_matmul_f32_stock_grad_min_cosine"] = float(w32), float(c32)
    del f32
    tr = FrameModelTrainer(p, size, 11, batch=B, matmul="fp32x3")
    loss, logits = tr.forward_backward(xd, yd)
    el = float(np.abs(logits.cpu().numpy() - rlog).max())
    report["finetune_matmul_fp32x3_stock_logits_maxabs_err"] = el
    assert el < 1e-4 and np.abs(loss.cpu().numpy() - rl).max() < 1e-4, (el, loss.cpu().numpy(), rl)
    for bn in STOCK_BNS:
        c = rstats[bn][0].shape[0]
        em = np.abs(tr.get(bn + "_batch_mean", shape=(c,)) - rstats[bn][0]).max() / max(1.0, np.abs(rstats[bn][0]).max())
        ev = np.abs(tr.get(bn + "_batch_var", shape=(c,)) - rstats[bn][1]).max() / max(1.0, np.abs(rstats[bn][1]).max())
        assert em < 1e-4 and ev < 1e-4, (bn, em, ev)
    for k in TIGHT_GRADS:
        g = rg[k]
        assert np.abs(tr.get(k, gradient=True) - g).max() < 1e-4 * np.abs(g).max(), k
    worst, worst_k, min_cos = _compare(tr, rg)
    report["finetune_matmul_fp32x3_stock_grad_rel_err_worst"] = float(worst)
    report["finetune_matmul_fp32x3_stock_grad_min_cosine"] = float(min_cos)
    print(f"stock 224x2: fp32x3 worst {worst:.3e} cosine {min_cos:.6f}; f32 worst {w32:.3e} cosine {c32:.6f}")
    assert min_cos > 0.995 and worst < 0.3, (worst_k, worst, min_cos)
    bn = "densenet0_stage2_batchnorm3"
    exp = 0.9 * p[bn + "_running_mean"] + 0.1 * rstats[bn][0]
    assert np.abs(tr.get(bn + "_running_mean") - exp).max() < 1e-4
    assert tr.matmul_stats() == (0, 359)


def test_repeatability_and_switching():
    from tennis_amd.engine import FrameModelTrainer
    B = 2
    p, x, y = _setup(B, 224, 9)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    tr = FrameModelTrainer(p, 224, 11, batch=B, matmul="fp32x3")
    tr.forward_backward(xd, yd)
    g1 = tr.grads.clone()
    tr.forward_backward(xd, yd)
    assert bool(torch.isfinite(g1).all())
    assert torch.equal(g1.view(torch.int32), tr.grads.view(torch.int32)), "two identical fp32x3 steps gave different gradients"
    # fp32x3 -> f32 on the same handle: the gradients of a trainer that never left f32, bit for bit
    tr.set_matmul("f32")
    assert tr.matmul == "f32"
    tr.forward_backward(xd, yd)
    never = FrameModelTrainer(p, 224, 11, batch=B)
    never.forward_backward(xd, yd)
    assert torch.equal(tr.grads.view(torch.int32), never.grads.view(torch.int32)), "the f32 step after a switch is not the f32 step"
    assert not torch.equal(tr.grads.view(torch.int32), g1.view(torch.int32))          # and the two modes are two computations
    assert tr.matmul_stats() == (359, 718) and never.matmul_stats() == (359, 0)
    with pytest.raises(ValueError):
        tr.set_matmul("bf16")


def test_sgd_steps_in_fp32x3_reduce_the_loss():
    """three steps of train.py's recipe in fp32x3 on one batch; the first update is oracle/train_np.py::sgd_momentum applied to the
    library's own gradients (1e-6, the f32 test's bar)"""
    from tennis_amd.engine import FrameModelTrainer
    B = 4
    p, x, y = _setup(B, 224, 9)
    tr = FrameModelTrainer(p, 224, 11, batch=B, matmul="fp32x3")
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    loss, _ = tr.forward_backward(xd, yd)
    first = float(loss.mean())
    names = ["framemodel0_dense0_weight", "densenet0_stage2_conv5_weight", "densenet0_conv0_weight", "densenet0_stage4_batchnorm7_gamma"]
    g0 = {k: tr.get(k, gradient=True) for k in names}
    tr.step(B, 0.01, 0.9, 1e-4)
    p1, _ = tn.sgd_momentum({k: p[k].astype(np.float64) for k in names}, g0, {}, 0.01, 0.9, 1e-4, 1.0 / B)
    for k in names:
        assert np.abs(tr.get(k) - p1[k]).max() < 1e-6 * max(1.0, np.abs(p1[k]).max()), k
    for _ in range(2):
        tr.forward_backward(xd, yd)
        tr.step(B, 0.01, 0.9, 1e-4)
    loss, _ = tr.forward_backward(xd, yd)
    assert float(loss.mean()) < first and bool(torch.isfinite(tr.grads).all())


# ---- 8. the CNN-RNN step and the captioner on frames ----------------------------------------------------------------------------------

def _cnnrnn_setup(B, T, shift=0.0, seed=5):
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(0)
    if shift:
        p = {k: (v + shift).astype(np.float32) if k.endswith("_beta") else v for k, v in p.items()}
    p.update(W.make_rnn_weights(2, "gru", 1024, 128, "cnnrnn0_gru0_"))
    p.update(W.make_dense_weights(1, 11, 256, "cnnrnn0_dense0_"))
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(B * T, 224, seed))
    y = np.random.default_rng(seed).integers(0, 11, B).astype(np.int32)
    return p, x, y


def _cnnrnn_run(tr, x, y, B, T):
    xd = torch.from_numpy(x).cuda().reshape(B, T, *x.shape[1:])
    loss, logits = tr.forward_backward(xd, torch.from_numpy(y).cuda())
    return loss.cpu().numpy(), logits.cpu().numpy()


def test_cnnrnn_step_open_relus(report):
    """tests/test_gpu_cnnrnn_train.py::test_step_exact_with_open_relus[gru] (batch 2 x steps 3 at 224 x 224, beta + 4) in fp32x3"""
    from tools import cnnrnn_train_torch as ct
    from tennis_amd.engine import CNNRNNTrainer
    _cap_threads()
    B, T = 2, 3
    p, x, y = _cnnrnn_setup(B, T, 4.0)
    tr = CNNRNNTrainer(p, 224, 11, batch=B, steps=T, type="gru", matmul="fp32x3")
    loss, logits = _cnnrnn_run(tr, x, y, B, T)
    rl, rlog, rg, _ = ct.loss_and_grads(p, x, y, T, "gru")
    assert np.abs(logits - rlog).max() < 1e-3 * max(1.0, np.abs(rlog).max())
    worst, worst_k, min_cos = _compare(tr, rg)
    report["cnnrnn_matmul_fp32x3_open_relu_grad_rel_err_worst"] = float(worst)
    report["cnnrnn_matmul_fp32x3_open_relu_grad_min_cosine"] = float(min_cos)
    assert worst < 2e-3 and min_cos > 0.999999, (worst_k, worst, min_cos)
    assert tr.matmul == "fp32x3" and tr.matmul_stats() == (0, 359)


def test_cnnrnn_frozen_step_counts_the_forward(report):
    """--freeze_backbone in fp32x3: 120 launches (the forward alone), the head's gradients against the oracle with detached features
    at the f32 test's 1e-4"""
    from tools import cnnrnn_train_torch as ct
    from tennis_amd.engine import CNNRNNTrainer
    _cap_threads()
    B, T = 2, 3
    p, x, y = _cnnrnn_setup(B, T)
    tr = CNNRNNTrainer(p, 224, 11, batch=B, steps=T, type="gru", freeze_backbone=True, matmul="fp32x3")
    loss, logits = _cnnrnn_run(tr, x, y, B, T)
    assert tr.matmul_stats() == (0, 120)
    rl, rlog, rg, _ = ct.loss_and_grads(p, x, y, T, frozen=True)
    assert np.abs(logits - rlog).max() < 1e-4 and np.abs(loss - rl).max() < 1e-4
    for k, g in rg.items():
        assert np.abs(tr.get(k, gradient=True) - g).max() < 1e-4 * np.abs(g).max(), k


def test_gnmt_frames_step_open_relus(report):
    """tests/test_gpu_gnmt_frames_train.py::test_step_exact_with_open_relus[gru-8] (batch 2 x steps 3, one padded slot) in fp32x3"""
    from tools import gnmt_frames_train_torch as ft
    from tennis_amd import weights as W
    from tennis_amd.engine import GNMTFramesTrainer
    _cap_threads()
    E, V, Lt, H, B, T, seed = 6, 14, 6, 8, 2, 3, 5
    p = W.make_densenet121_weights(0)
    p = {k: (v + 4.0).astype(np.float32) if k.endswith("_beta") else v for k, v in p.items()}
    p.update(W.make_gnmt_weights(seed, "gru", 1024, H, E, V))
    p["gnmt_tgt_embed_weight"] = np.random.default_rng(seed).normal(0, 0.5, (V, E)).astype(np.float32)
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(B * T, 224, seed)).reshape(B, T, 3, 224, 224)
    rng = np.random.default_rng(seed)
    tgt = rng.integers(4, V, (B, Lt)).astype(np.int32)
    tgt[:, 0] = 2
    tvl = rng.integers(3, Lt + 1, B).astype(np.int32)
    tvl[0] = Lt
    for b in range(B):
        tgt[b, tvl[b] - 1] = 3
        tgt[b, tvl[b]:] = 1
    svl = np.array((3, 2), np.int32)
    tr = GNMTFramesTrainer(p, H, E, V, size=224, max_batch=2, max_src_len=3, max_tgt_len=Lt, cell_type="gru", matmul="fp32x3")
    loss, logits = tr.forward_backward(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(svl).cuda(),
                                       torch.from_numpy(tgt).cuda(), torch.from_numpy(tvl).cuda(), return_logits=True)
    logits = logits.cpu().numpy()
    rl, rlog, rg, _, _ = ft.loss_and_grads(p, x, svl, tgt, tvl, H, cell="gru")
    assert float(np.abs(logits - rlog).max()) < 1e-3 * max(1.0, np.abs(rlog).max())
    worst, worst_k, min_cos = _compare(tr, rg)
    report["gnmt_frames_matmul_fp32x3_open_relu_grad_rel_err_worst"] = float(worst)
    report["gnmt_frames_matmul_fp32x3_open_relu_grad_min_cosine"] = float(min_cos)
    assert worst < 2e-3 and min_cos > 0.999999, (worst_k, worst, min_cos)
    assert tr.matmul == "fp32x3" and tr.matmul_stats() == (0, 359)


# ---- 9. the driver and the ABI's refusals --------------------------------------------------------------------------------------------

def test_train_driver_runs_in_fp32x3(tmp_path, capsys):
    from tennis_amd import train as tr
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    assert tr.main(["--root", root, "--frames_per_video", "8", "--data_shape", "224", "--model_id", "0009", "--window", "2", "--temp_pool",
                    "gru", "--epochs", "1", "--batch_size", "2", "--max_batches", "1", "--exp_root", exp, "--matmul", "fp32x3"]) == 0
    out = capsys.readouterr().out
    assert "Backbone matmul: fp32x3" in out
    assert (tmp_path / "exp" / "0009" / "0000.params").exists()


def test_abi_refusals():
    from tennis_amd.engine import FrameModelTrainer
    L = _L()
    p, _, _ = _setup(2)
    tr = FrameModelTrainer(p, 224, 11, batch=2)
    lib = tr.lib
    assert lib.tn_finetune_set_matmul(tr.handle, 7) != 0
    assert b"TN_MATMUL" in lib.tn_last_error()
    assert tr.matmul_stats() == (0, 0) and tr.matmul == "f32"
    a, b = C.c_int64(), C.c_int64()
    assert lib.tn_finetune_set_matmul(None, 1) != 0 and b"null handle" in lib.tn_last_error()
    assert lib.tn_finetune_matmul_stats(None, C.byref(a), C.byref(b)) != 0
    assert lib.tn_cnnrnn_trainer_set_matmul(None, 1) != 0 and lib.tn_cnnrnn_trainer_matmul_stats(None, C.byref(a), C.byref(b)) != 0
    assert lib.tn_gnmt_frames_trainer_set_matmul(None, 1) != 0
    assert lib.tn_gnmt_frames_trainer_matmul_stats(None, C.byref(a), C.byref(b)) != 0
    ctx = L.default_context()
    t = torch.zeros((16, 8), device="cuda")
    s = torch.ones(8, device="cuda")
    assert lib.tn_dbg_linear_fp32x3(ctx.handle, _p(t), 7, None, None, _p(t), 8, None, _p(t), 8, 8, 8, 8, 0) != 0        # ldx < K
    assert lib.tn_dbg_linear_fp32x3(ctx.handle, _p(t), 8, _p(s), None, _p(t), 8, None, _p(t), 8, 8, 8, 8, 0) != 0      # asc without ash
    assert lib.tn_dbg_gemm_tn_fp32x3(ctx.handle, _p(t), 7, _p(t), 8, None, None, _p(t), 8, 8, 8, 16, None, 0) != 0    # lda < M
    assert lib.tn_dbg_gemm_tn_fp32x3(ctx.handle, _p(t), 8, _p(t), 8, _p(s), None, _p(t), 8, 8, 8, 16, None, 0) != 0
