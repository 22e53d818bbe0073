"""-m gpu: the training-only kernels of the fine-tuning step (tn_finetune_*) on their own, against NumPy float64.

Through the test hooks of include/tennis_hip_debug.h, which call the launchers the step calls:
  * tn_dbg_gemm_tn (train.hip gemm_tn_dispatch: gemm_tn_f32_kernel, its BN + ReLU operand form, split-K and splitk_reduce_kernel) at
    the weight-gradient shapes of a 512x512 x 64 step and at ragged shapes, with and without the split-K workspace;
  * tn_dbg_linear_bnrelu (linear.hip launch_linear_f32_bnrelu: the forward 1x1 convolutions with BN + ReLU on the X operand);
  * tn_dbg_linear at the stem's row count of a 512x512 x 64 step and past 65,536 row tiles;
  * tn_dbg_bn_train (finetune.hip: the training-mode BatchNorm statistics, BN + ReLU and its backward) on adversarial columns.
Errors are measured against magnitude-scaled bars (|A|^T |B| for a product, the column's scale for a BatchNorm); the worst ones go to
the session report (the `report` fixture of tests/conftest.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5          # gluon nn.BatchNorm(epsilon=1e-5), finetune.hip kEps
CHUNK = 1 << 16     # rows per float64 chunk of a reference


def _lib():
    from tennis_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx():
    return _lib().default_context()


def _worst(report, key, v):
    report[key] = max(float(v), report.get(key, 0.0))


def _dev_rand(rows, cols, seed, mean=0.0, std=1.0):
    """(rows, cols) float32 normal on the GPU (a big operand is never generated on the host)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn((rows, cols), generator=g, device="cuda", dtype=torch.float32).mul_(std).add_(mean)


# ---- gemm_tn: C (M, N) = A^T B over K rows ---------------------------------------------------------------------------------------

def _gemm_tn_ref(A, B, M, N, bsc=None, bsh=None):
    """float64 A[:, :M]^T op(B[:, :N]) and |A|^T |op(B)|, walked in row chunks (A, B device tensors of K rows)"""
    ref, mag = np.zeros((M, N)), np.zeros((M, N))
    for r0 in range(0, A.shape[0], CHUNK):
        a = A[r0:r0 + CHUNK, :M].cpu().numpy().astype(np.float64)
        b = B[r0:r0 + CHUNK, :N].cpu().numpy().astype(np.float64)
        if bsc is not None:
            b = np.maximum(b * bsc.astype(np.float64) + bsh.astype(np.float64), 0.0)
        ref += a.T @ b
        mag += np.abs(a).T @ np.abs(b)
    return ref, mag


def _gemm_tn(ctx, A, B, M, N, K, ws_floats, bsc=None, bsh=None, ldc=None, a_off=0, b_off=0):
    """one tn_dbg_gemm_tn call; A / B (K, ld) device tensors, operand pointers optionally moved on by a_off / b_off floats"""
    import ctypes as C
    L = _lib()
    ldc = ldc or N
    out = torch.full((M, ldc), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(max(1, ws_floats), dtype=torch.float32, device="cuda") if ws_floats else None
    sc = torch.from_numpy(bsc).cuda() if bsc is not None else None
    sh = torch.from_numpy(bsh).cuda() if bsh is not None else None
    pa, pb = C.c_void_p(A.data_ptr() + 4 * a_off), C.c_void_p(B.data_ptr() + 4 * b_off)
    L.check(ctx.lib.tn_dbg_gemm_tn(ctx.handle, pa, A.shape[1], pb, B.shape[1], L.ptr(sc), L.ptr(sh), L.ptr(out), ldc, M, N, K,
                                   L.ptr(ws), ws_floats), "tn_dbg_gemm_tn")
    return out[:, :N].cpu().numpy()


def _check_gemm(report, key, got, ref, mag, tol):
    assert np.isfinite(got).all(), key
    rel = np.abs(got.astype(np.float64) - ref) / np.maximum(mag, 1e-30)
    _worst(report, "gemm_tn_rel_err_worst", rel.max())
    report[f"gemm_tn_{key}"] = float(rel.max())
    assert rel.max() < tol, (key, float(rel.max()), np.unravel_index(rel.argmax(), rel.shape))


# The per-element error relative to |A|^T |B|: an fp32 MFMA chain over each split-K slice, the slices added in order.  Random-sign
# products keep the partial sums small against |A|^T |B|, so the bar sits far below the K u worst case of a recursive sum.
# Measured on MI355X: 3.2e-7 worst (unsplit, K = 65,536), split forms 1e-8 to 1e-7; linear_bnrelu 3.5e-7, the long stem 3.7e-7.
GEMM_TOL = 1e-6
WS_STEP = 16 << 20           # the step's workspace (finetune.hip: ws_floats = 16 Mi floats)

# (name, M, N, K): the weight gradients of a 512x512 x 64 step: a dense 3x3 (32, 1152) over 64*128*128 rows, block 1's 1x1
# (128, K) at K = 64 and 256, the stem (64, 147) over 64*256*256 rows, transitions 1 and 3
STEP_SHAPES = [("conv3x3_b1", 32, 1152, 64 * 128 * 128), ("conv1x1_k64", 128, 64, 64 * 128 * 128),
               ("conv1x1_k256", 128, 256, 64 * 128 * 128), ("stem", 64, 147, 64 * 256 * 256),
               ("trans1", 128, 256, 64 * 128 * 128), ("trans3", 512, 1024, 64 * 32 * 32)]


@pytest.mark.parametrize("name,M,N,K", STEP_SHAPES, ids=[s[0] for s in STEP_SHAPES])
def test_gemm_tn_weight_gradient_shapes(ctx, report, name, M, N, K):
    A = _dev_rand(K, M, 11 + M)
    B = _dev_rand(K, N, 17 + N, mean=0.25)
    ref, mag = _gemm_tn_ref(A, B, M, N)
    split = _gemm_tn(ctx, A, B, M, N, K, WS_STEP)
    again = _gemm_tn(ctx, A, B, M, N, K, WS_STEP)
    assert np.array_equal(split.view(np.uint32), again.view(np.uint32)), "split-K result not bit-identical on a repeated call"
    _check_gemm(report, f"{name}_split", split, ref, mag, GEMM_TOL)
    if K <= (1 << 20):                                   # the unsplit form: one chain of K MFMAs per output tile
        _check_gemm(report, f"{name}_unsplit", _gemm_tn(ctx, A, B, M, N, K, 0), ref, mag, GEMM_TOL)


@pytest.mark.parametrize("K", [1, 15, 16, 2047, 2048, 2049, 4100, 70001])
@pytest.mark.parametrize("M,N", [(70, 100), (32, 1152), (5, 3), (128, 193)])
def test_gemm_tn_ragged(ctx, report, M, N, K):
    """M, N off the 64 grid; K round the 2048 split gate and the 16-row k-tile; 4100 and 70001 leave a short last slice"""
    A = _dev_rand(K, M, K + M)
    B = _dev_rand(K, N, K + N + 1)
    ref, mag = _gemm_tn_ref(A, B, M, N)
    a = _gemm_tn(ctx, A, B, M, N, K, WS_STEP)
    b = _gemm_tn(ctx, A, B, M, N, K, WS_STEP)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _check_gemm(report, f"ragged_{M}x{N}x{K}_split", a, ref, mag, GEMM_TOL)
    _check_gemm(report, f"ragged_{M}x{N}x{K}_unsplit", _gemm_tn(ctx, A, B, M, N, K, 0), ref, mag, GEMM_TOL)


@pytest.mark.parametrize("ws_mult", [1, 2, 3, 7])
def test_gemm_tn_small_workspace(ctx, report, ws_mult):
    """a workspace of ws_mult (M, N) partials cuts S back from its natural 512 / tiles (here 128); 1 means no split at all"""
    M, N, K = 70, 100, 300007
    A = _dev_rand(K, M, 3)
    B = _dev_rand(K, N, 4)
    ref, mag = _gemm_tn_ref(A, B, M, N)
    got = _gemm_tn(ctx, A, B, M, N, K, ws_mult * M * N)
    _check_gemm(report, f"small_ws_{ws_mult}", got, ref, mag, GEMM_TOL)


@pytest.mark.parametrize("lda_pad,ldb_pad,a_off,b_off", [(1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 1, 0), (0, 0, 0, 2), (5, 7, 3, 1)])
def test_gemm_tn_scalar_path(ctx, report, lda_pad, ldb_pad, a_off, b_off):
    """lda / ldb not multiples of 4, or an operand pointer off 16 bytes: the scalar (vec = false) staging path; ldc > N"""
    M, N, K = 128, 192, 50000
    A = _dev_rand(K + 1, M + lda_pad + a_off, 5)
    B = _dev_rand(K + 1, N + ldb_pad + b_off, 6)
    lda, ldb = A.shape[1], B.shape[1]           # what the kernel sees: K rows of the full stride from the offset on
    a_host = A.cpu().numpy().reshape(-1)[a_off:a_off + K * lda].reshape(K, lda)[:, :M]
    b_host = B.cpu().numpy().reshape(-1)[b_off:b_off + K * ldb].reshape(K, ldb)[:, :N]
    ref, mag = _gemm_tn_ref(torch.from_numpy(np.ascontiguousarray(a_host)), torch.from_numpy(np.ascontiguousarray(b_host)), M, N)
    for ws in (WS_STEP, 0):
        got = _gemm_tn(ctx, A, B, M, N, K, ws, ldc=N + 3, a_off=a_off, b_off=b_off)
        _check_gemm(report, f"scalar_{lda_pad}_{ldb_pad}_{a_off}_{b_off}_{'split' if ws else 'unsplit'}", got, ref, mag, GEMM_TOL)


@pytest.mark.parametrize("M,N,K", [(128, 256, 1 << 20), (128, 100, 4099), (32, 64, 77)])
def test_gemm_tn_bnrelu_operand(ctx, report, M, N, K):
    """B -> relu(B bsc + bsh) while staged, with negative, zero and tiny scales (the backward of a BN + ReLU'd 1x1 input)"""
    rng = np.random.default_rng(M + N + K)
    bsc = (rng.uniform(0.2, 2.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    bsh = rng.normal(0.0, 1.0, N).astype(np.float32)
    bsc[0], bsh[0] = 0.0, 0.75                  # scale 0: the constant relu(shift)
    bsc[1], bsh[1] = 0.0, -0.5                  # ... which is 0
    bsc[2], bsh[2] = -1.5, 0.0                  # negative scale
    bsc[3], bsh[3] = 1e-30, 0.0                 # a denormal product
    A = _dev_rand(K, M, 7)
    B = _dev_rand(K, N, 8, mean=0.3, std=1.5)
    ref, mag = _gemm_tn_ref(A, B, M, N, bsc, bsh)
    for ws in (WS_STEP, 0):
        got = _gemm_tn(ctx, A, B, M, N, K, ws, bsc=bsc, bsh=bsh)
        assert (got[:, 1] == 0.0).all()
        _check_gemm(report, f"bnrelu_{M}x{N}x{K}_{'split' if ws else 'unsplit'}", got, ref, mag, GEMM_TOL)


def test_gemm_tn_hook_refuses_bad_arguments(ctx):
    L = _lib()
    A = torch.zeros((16, 8), device="cuda")
    out = torch.zeros((8, 8), device="cuda")
    s = torch.ones(8, device="cuda")
    assert ctx.lib.tn_dbg_gemm_tn(ctx.handle, L.ptr(A), 7, L.ptr(A), 8, None, None, L.ptr(out), 8, 8, 8, 16, None, 0) != 0   # lda < M
    assert ctx.lib.tn_dbg_gemm_tn(ctx.handle, L.ptr(A), 8, L.ptr(A), 8, L.ptr(s), None, L.ptr(out), 8, 8, 8, 16, None, 0) != 0


# ---- linear_f32_bnrelu: Y (+)= relu(X asc + ash) W^T (+ bias) --------------------------------------------------------------------

def _linear_bnrelu_ref(x, asc, ash, w, bias):
    a = np.maximum(x.astype(np.float64) * asc.astype(np.float64) + ash.astype(np.float64), 0.0)
    w64 = w.astype(np.float64)
    ref = a @ w64.T + (bias.astype(np.float64) if bias is not None else 0.0)
    mag = np.abs(a) @ np.abs(w64).T + (np.abs(bias.astype(np.float64)) if bias is not None else 0.0)
    return ref, mag


LINEAR_TOL = 1e-6     # K <= 1024: one MFMA chain per output


# (M, N, K, ldx, bias, accumulate): >= 512 64x64 tiles (linear_f32_kernel<2, true>) and fewer (linear_f32_skinny_kernel<true>);
# K % 4 != 0 and ldx > K (the scalar staging path), accumulate (the backward's dX += ... form)
LINEAR_CASES = [(33000, 64, 256, 256, False, 0), (33001, 128, 131, 131, True, 0), (40000, 32, 1152, 1160, False, 1),
                (1000, 100, 64, 64, True, 0), (777, 128, 147, 150, False, 1), (5, 3, 1, 1, True, 0),
                (16384, 128, 1024, 1024, False, 0), (2049, 512, 1022, 1030, True, 1)]


@pytest.mark.parametrize("M,N,K,ldx,use_bias,accumulate", LINEAR_CASES)
def test_linear_bnrelu(ctx, report, M, N, K, ldx, use_bias, accumulate):
    L = _lib()
    rng = np.random.default_rng([M, N, K, accumulate])
    x = rng.normal(0.2, 1.3, (M, ldx)).astype(np.float32)
    asc = (rng.uniform(0.2, 2.0, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32)
    ash = rng.normal(0.0, 1.0, K).astype(np.float32)
    asc[0] = 0.0
    if K > 2:
        asc[1], ash[1] = 0.0, -1.0
    ldw = K + 3
    w = rng.normal(0.0, 1.0 / np.sqrt(K), (N, ldw)).astype(np.float32)
    bias = rng.normal(0.0, 1.0, N).astype(np.float32) if use_bias else None
    ldy = N + 5
    y0 = rng.normal(0.0, 1.0, (M, ldy)).astype(np.float32)
    xd, ad, hd, wd, yd = (torch.from_numpy(v).cuda() for v in (x, asc, ash, w, y0))
    bd = torch.from_numpy(bias).cuda() if use_bias else None
    L.check(ctx.lib.tn_dbg_linear_bnrelu(ctx.handle, L.ptr(xd), ldx, L.ptr(ad), L.ptr(hd), L.ptr(wd), ldw, L.ptr(bd), L.ptr(yd), ldy,
                                         M, N, K, accumulate), "tn_dbg_linear_bnrelu")
    got = yd.cpu().numpy()
    ref, mag = _linear_bnrelu_ref(x[:, :K], asc, ash, w[:, :K], bias)
    if accumulate:
        ref, mag = ref + y0[:, :N], mag + np.abs(y0[:, :N])
    assert np.array_equal(got[:, N:], y0[:, N:]), "columns past N written"
    rel = np.abs(got[:, :N] - ref) / np.maximum(mag, 1e-30)
    _worst(report, "linear_bnrelu_rel_err_worst", rel.max())
    report[f"linear_bnrelu_{M}x{N}x{K}_acc{accumulate}"] = float(rel.max())
    assert rel.max() < LINEAR_TOL, (float(rel.max()), np.unravel_index(rel.argmax(), rel.shape))


# ---- the stem GEMM's grid: 64 * 256 * 256 rows are 65,536 row tiles -------------------------------------------------------------

@pytest.mark.parametrize("M", [64 * 256 * 256, 64 * 256 * 256 + 3 * 64 + 17, 65 * 256 * 256])
def test_linear_past_the_grid_y_limit(ctx, report, M):
    """tn_dbg_linear (launch_linear_f32) at N = 64, K = 147: M row tiles of 64 reach 65,536 (a 512x512 x 64 step's stem) and pass it
    (a batch of 65).  Every row must be written; the first, last and boundary-straddling row blocks are checked against float64."""
    L = _lib()
    N, K = 64, 147
    X = _dev_rand(M, K, 21)
    rng = np.random.default_rng(M)
    w = rng.normal(0.0, 1.0 / np.sqrt(K), (N, K)).astype(np.float32)
    b = rng.normal(0.0, 1.0, N).astype(np.float32)
    wd, bd = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    Y = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    L.check(ctx.lib.tn_dbg_linear(ctx.handle, L.ptr(X), L.ptr(wd), L.ptr(bd), L.ptr(Y), M, N, K), "tn_dbg_linear")
    ctx.sync()
    written = torch.isfinite(Y).all(dim=1)
    missing = int((~written).sum())
    report[f"linear_grid_M{M}_rows_unwritten"] = missing
    assert missing == 0, (M, missing, int((~written).nonzero()[0]))
    worst = 0.0
    edges = [0, 32767 * 64, 65535 * 64 - 128, 65536 * 64 - 128, M - 4096]
    for r0 in sorted({min(max(0, e), M - 1) for e in edges}):
        x = X[r0:r0 + 4096].cpu().numpy().astype(np.float64)
        ref = x @ w.T.astype(np.float64) + b
        mag = np.abs(x) @ np.abs(w.T.astype(np.float64)) + np.abs(b)
        got = Y[r0:r0 + 4096].cpu().numpy()
        worst = max(worst, float((np.abs(got - ref) / mag).max()))
    report[f"linear_grid_M{M}_rel_err"] = worst
    assert worst < LINEAR_TOL, worst


# ---- training-mode BatchNorm ------------------------------------------------------------------------------------------------------

KINDS = ("normal", "outlier_row0", "large_mean", "constant", "border", "negative")


def _bn_matrix(M, C, ld, seed):
    """(M, ld) float32 whose column c is of kind KINDS[c % 6]; the pad columns are garbage the kernels must not read"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, ld), dtype=np.float32) * np.float32(1e3)
    r = np.arange(M)
    side = 16                                    # a 16x16 frame per 256 rows: its border pixels, corner first (row 0)
    py, px = (r % 256) // side, r % side
    border = (py == 0) | (py == side - 1) | (px == 0) | (px == side - 1)
    for c in range(C):
        kind = KINDS[c % 6]
        if kind == "normal":
            v = rng.normal(0.3, 1.2, M)
        elif kind == "outlier_row0":             # x0 = mu + 30 sigma: the shifted one-pass sums' worst shift
            v = rng.normal(-0.7, 0.5, M)
            v[0] = -0.7 + 30 * 0.5
        elif kind == "large_mean":
            v = rng.normal(50.0, 1e-2, M)
        elif kind == "constant":
            v = np.full(M, 0.7)
        elif kind == "border":                   # a zero-padded convolution of a flat frame: constant but for the border
            v = np.where(border, 0.4, 1.25) + (py == 0) * 0.1
        else:
            v = rng.normal(-2.0, 0.5, M)
        x[:, c] = v
    return x


def _bn_ref(x, C):
    """float64 mean, biased variance and mean |x| of columns [0, C), in row chunks"""
    M = x.shape[0]
    s1 = np.zeros(C)
    for r0 in range(0, M, CHUNK):
        s1 += x[r0:r0 + CHUNK, :C].astype(np.float64).sum(0)
    mean = s1 / M
    s2, sa = np.zeros(C), np.zeros(C)
    for r0 in range(0, M, CHUNK):
        d = x[r0:r0 + CHUNK, :C].astype(np.float64) - mean
        s2 += (d * d).sum(0)
        sa += np.abs(x[r0:r0 + CHUNK, :C].astype(np.float64)).sum(0)
    var = s2 / M
    return mean, var, sa / M


def _bn_bars(x, dy, got, mean, var, absmean, gamma, beta, C, accumulate, dx0):
    """per-element worst errors of y, dgamma / dbeta and dx relative to their scales, in float64, row chunk by row chunk.  A ReLU
    input within 1e-5 of 0 (relative to its terms) may take either branch in float32 (in a column of mean 50 and sigma 1e-2 the
    float32 mean alone moves it by 2e-4 sigma): its element is let through in y, and what its branch can move dgamma, dbeta and dx
    by is allowed on top of their bars."""
    M = x.shape[0]
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    isd = 1.0 / np.sqrt(var + EPS)
    err_y = 0.0
    db, dg, sb, sg = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
    amb_b, amb_g = np.zeros(C), np.zeros(C)
    for r0 in range(0, M, CHUNK):
        xc = x[r0:r0 + CHUNK, :C].astype(np.float64)
        xh = (xc - mean) * isd
        pre = g64 * xh + b64
        scale = np.abs(g64) * (np.abs(xc) + absmean) * isd + np.abs(b64)
        amb = np.abs(pre) <= 1e-5 * scale
        e = np.abs(got["y"][r0:r0 + CHUNK].astype(np.float64) - np.maximum(pre, 0.0)) / scale
        e[amb] = 0.0
        err_y = max(err_y, float(e.max()) if e.size else 0.0)
        if dy is not None:
            d = dy[r0:r0 + CHUNK].astype(np.float64)
            gg = np.where(pre > 0, d, 0.0)
            db += gg.sum(0); dg += (gg * xh).sum(0)
            sb += np.abs(gg).sum(0); sg += np.abs(gg * xh).sum(0)
            amb_b += (np.abs(d) * amb).sum(0); amb_g += (np.abs(d * xh) * amb).sum(0)
    out = {"y": err_y}
    if dy is None:
        return out
    # what an ambiguous element can move a result by is allowed in full, the rest is measured against the result's scale
    out["dbeta"] = float((np.maximum(np.abs(got["dbeta"] - db) - amb_b, 0.0) / (sb + 1e-30)).max())
    out["dgamma"] = float((np.maximum(np.abs(got["dgamma"] - dg) - amb_g, 0.0) / (sg + 1e-30)).max())
    err_dx = 0.0
    gis = g64 * isd
    for r0 in range(0, M, CHUNK):
        xc = x[r0:r0 + CHUNK, :C].astype(np.float64)
        xh = (xc - mean) * isd
        pre = g64 * xh + b64
        amb = np.abs(pre) <= 1e-5 * (np.abs(g64) * (np.abs(xc) + absmean) * isd + np.abs(b64))
        d = dy[r0:r0 + CHUNK].astype(np.float64)
        gg = np.where(pre > 0, d, 0.0)
        v = gis * (gg - db / M - xh * dg / M)
        allow = np.abs(gis) * (np.abs(d) * amb + amb_b / M + np.abs(xh) * amb_g / M)
        scale = np.abs(gis) * (np.abs(gg) + sb / M + np.abs(xh) * sg / M)
        got_dx = got["dx"][r0:r0 + CHUNK].astype(np.float64)
        if accumulate:
            v = v + dx0[r0:r0 + CHUNK]
            scale = scale + np.abs(dx0[r0:r0 + CHUNK])
        # a variance off by dv moves 1/sqrt(var + eps) by dv / (2 (var + eps)): the bar includes what the var bar allows
        scale = scale + np.abs(v) * VAR_TOL
        e = np.maximum(np.abs(got_dx - v) - allow, 0.0) / np.maximum(scale, 1e-30)
        err_dx = max(err_dx, float(e.max()) if e.size else 0.0)
    out["dx"] = err_dx
    return out


# Measured on MI355X (worst over every case): mean 5.9e-7, var 3.4e-6, y 2.5e-7, dbeta 3.4e-8, dgamma 1.2e-7, dx 1.6e-6.  Before the
# shift of the one-pass variance moved off row 0: var 1.2e-3 (the outlier column), mean 1.6e-5, y 5.7e-4.
MEAN_TOL = 1e-6      # |mean - ref| / mean |x|
VAR_TOL = 1e-5       # |var - ref| / max(var, eps)
Y_TOL = 1e-6         # |y - ref| / (|gamma| (|x| + mean|x|) / sqrt(var + eps) + |beta|)
GRAD_TOL = 5e-6      # dbeta, dgamma: / sum |terms|;  dx: / the sum of its terms' magnitudes

BN_ROWS = [1, 2047, 2048, 2049, 5003, 1 << 20, 1 << 22]
BN_CHANNELS = [32, 64, 128, 1024]


# (the 4 Mi-row map at 32 and 64 channels and the 1 Mi-row one up to 128 cover the long reductions)
BN_CASES = [(M, C) for M in BN_ROWS for C in BN_CHANNELS if M * C <= (1 << 28)]


@pytest.mark.parametrize("M,C", BN_CASES)
def test_bn_train_against_fp64(ctx, report, M, C):
    L = _lib()
    rng = np.random.default_rng([M, C])
    ld = C + 4 + M % 3                                            # ld > C (not always a multiple of 4)
    x = _bn_matrix(M, C, ld, M + C)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.normal(0.0, 0.5, C).astype(np.float32)
    gamma[7 % C] = -0.8                                           # a negative and a zero scale
    if C > 13:
        gamma[13] = 0.0
    dy = rng.standard_normal((M, C), dtype=np.float32)
    accumulate = int(M % 2)
    ldd = C + 3
    dx0 = rng.standard_normal((M, ldd), dtype=np.float32)
    xd, gd, bd, dyd = (torch.from_numpy(v).cuda() for v in (x, gamma, beta, dy))
    outs = []
    for _ in range(2):
        mean = torch.full((C,), float("nan"), device="cuda")
        var, dg, db = mean.clone(), mean.clone(), mean.clone()
        y = torch.full((M, C), float("nan"), device="cuda")
        dx = torch.from_numpy(dx0).cuda()
        L.check(ctx.lib.tn_dbg_bn_train(ctx.handle, L.ptr(xd), ld, M, C, L.ptr(gd), L.ptr(bd), L.ptr(mean), L.ptr(var), L.ptr(y),
                                        L.ptr(dyd), L.ptr(dg), L.ptr(db), L.ptr(dx), ldd, accumulate), "tn_dbg_bn_train")
        outs.append({"mean": mean.cpu().numpy(), "var": var.cpu().numpy(), "y": y.cpu().numpy(), "dgamma": dg.cpu().numpy(),
                     "dbeta": db.cpu().numpy(), "dx": dx.cpu().numpy()})
        del y, dx
    for k in outs[0]:
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)), f"{k} not bit-identical on a repeated call"
    got = outs[0]
    got["dx"], dx_pad = got["dx"][:, :C], got["dx"][:, C:]
    assert np.array_equal(dx_pad, dx0[:, C:]), "dx columns past C written"
    mean, var, absmean = _bn_ref(x, C)
    e_mean = np.abs(got["mean"] - mean) / np.maximum(absmean, 1e-30)
    e_var = np.abs(got["var"] - var) / np.maximum(var, EPS)
    const = [c for c in range(C) if KINDS[c % 6] == "constant"]
    assert (got["var"][const] == 0.0).all() and (got["mean"][const] == np.float32(0.7)).all(), got["var"][const]
    assert (got["var"] >= 0).all() and np.isfinite(got["var"]).all()
    errs = _bn_bars(x, dy, got, mean, var, absmean, gamma, beta, C, accumulate, dx0[:, :C].astype(np.float64))
    errs["mean"], errs["var"] = float(e_mean.max()), float(e_var.max())
    for k, v in errs.items():
        _worst(report, f"bn_train_{k}_rel_err_worst", v)
        report[f"bn_train_{M}x{C}_{k}"] = v
    worst_kind = {KINDS[c % 6]: float(e_var[c]) for c in np.argsort(e_var)[-3:]}
    assert errs["mean"] < MEAN_TOL and errs["var"] < VAR_TOL, (errs, worst_kind)
    assert errs["y"] < Y_TOL, errs
    assert errs["dbeta"] < GRAD_TOL and errs["dgamma"] < GRAD_TOL and errs["dx"] < GRAD_TOL, errs


def test_bn_train_forward_only_and_refusals(ctx):
    """without dy only the forward runs; dy without its outputs, or ld < C, is refused"""
    L = _lib()
    M, C = 3000, 64
    x = torch.randn((M, C), device="cuda")
    g, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    mean, var = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    y = torch.empty((M, C), device="cuda")
    L.check(ctx.lib.tn_dbg_bn_train(ctx.handle, L.ptr(x), C, M, C, L.ptr(g), L.ptr(b), L.ptr(mean), L.ptr(var), L.ptr(y), None, None,
                                    None, None, 0, 0), "tn_dbg_bn_train")
    x64 = x.double().cpu()
    assert torch.allclose(mean.double().cpu(), x64.mean(0), atol=1e-6)
    assert torch.allclose(y.double().cpu(), torch.relu((x64 - x64.mean(0)) / torch.sqrt(x64.var(0, unbiased=False) + EPS)), atol=1e-5)
    assert ctx.lib.tn_dbg_bn_train(ctx.handle, L.ptr(x), C, M, C, L.ptr(g), L.ptr(b), L.ptr(mean), L.ptr(var), L.ptr(y), L.ptr(x),
                                   None, None, None, C, 0) != 0
    assert ctx.lib.tn_dbg_bn_train(ctx.handle, L.ptr(x), C - 1, M, C, L.ptr(g), L.ptr(b), L.ptr(mean), L.ptr(var), L.ptr(y), None,
                                   None, None, None, 0, 0) != 0
