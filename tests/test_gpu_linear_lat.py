"""-m gpu: the latency GEMM (tennis_amd/csrc/linear.h lat_tile_f32<WK4, XK4>) on its own, against NumPy float64.

Through tn_dbg_linear_lat (include/tennis_hip_debug.h), which calls launch_linear_f32_lat2 / launch_linear_f32_lat_wk4 with the
production grid and reports which kernel ran.  Shapes, references and bars are tests/tools/gnmt_step_refs.py's (checked on the CPU
by tests/test_cpu_gnmt_step_refs.py, which also shows that a tile losing four k, a chunk, a wave's quarter, the bias, a row or a
column misses these bars by a factor of 10 or more).  Error per element against sum|x w| + |b|; bar = max(1e-6, 16 x the float32
NumPy evaluation's error), from the reference alone.  Operands sit at pitches above their widths (ldw = K + 16, ldx = K + 8,
k-group-major X with M + 5 rows, ldy = N + 7) and the output inside a guarded buffer.  The measured errors go to the session report."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tools import gnmt_step_refs as SR
from tools.guarded import Guarded, bits, dev

pytestmark = pytest.mark.gpu

PAD = 7.0              # what the pad columns / pad rows of the operands hold: a kernel reading past K or past M shows


def _lib():
    from tennis_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx():
    return _lib().default_context()


def _pitched(a, ld, off=0):
    """device copy of a (rows, cols) at pitch ld, `off` floats into a 16-byte aligned allocation -> (tensor, pointer)"""
    rows, cols = a.shape
    host = np.full(off + rows * ld + 4, PAD, dtype=np.float32)
    host[off:off + rows * ld].reshape(rows, ld)[:, :cols] = a
    t = torch.from_numpy(host).cuda()
    return t, C.c_void_p(t.data_ptr() + 4 * off)


def _run(ctx, form, inp, nsplit=None, K2=0, bias=True, xoff=0):
    """one tn_dbg_linear_lat call -> (y (M,N), route)"""
    L = _lib()
    X, W, b = inp["X"], inp["W"], inp["b"]
    M, K = X.shape
    N = W.shape[0]
    wt, wp = _pitched(W, K + SR.LAT_LDW_PAD)
    if form == "wk4xk4":
        rows = M + SR.LAT_XROWS_PAD
        xt = dev(SR.k4(X, rows).reshape(-1))
        xp, ldx = C.c_void_p(xt.data_ptr()), -rows
    else:
        ldx = K + SR.LAT_LDX_PAD
        xt, xp = _pitched(X, ldx, xoff)
    bt = dev(b) if bias else None
    y = Guarded(M, N, ld=N + SR.LAT_LDY_PAD)
    route = C.c_int(-1)
    rc = ctx.lib.tn_dbg_linear_lat(ctx.handle, 0 if form == "rm" else 1, xp, ldx, wp, K + SR.LAT_LDW_PAD, L.ptr(bt), y.ptr, N + SR.LAT_LDY_PAD,
                                   M, N, K, N if nsplit is None else nsplit, K2, C.byref(route))
    L.check(rc, "tn_dbg_linear_lat")
    del wt, xt
    return y.read(), route.value


@functools.lru_cache(maxsize=None)
def _refs(M, N, K, nsplit=None, K2=None, bias=True):
    inp = SR.lat_inputs(M, N, K)
    return inp, SR.lat_gemm(inp, nsplit=nsplit, K2=K2, bias=bias), SR.lat_gemm(inp, np.float32, nsplit=nsplit, K2=K2, bias=bias)


def _check(report, tag, got, r64, r32):
    e, b = SR.rel_err(got, r64["y"], r64["y_mag"]), SR.rel_bar(r64["y"], r32["y"], r64["y_mag"])
    report[f"linear_lat_{tag}"] = [e, b]
    print(f"{tag}: err {e:.3e} bar {b:.3e}")
    assert e <= b, (tag, e, b)


SHAPE_IDS = [f"K{K}_M{M}_N{N}" for K, M, N in SR.LAT_SHAPES]


@pytest.mark.parametrize("form", SR.LAT_FORMS)
@pytest.mark.parametrize("K,M,N", SR.LAT_SHAPES, ids=SHAPE_IDS)
def test_lat_gemm_matches_float64(ctx, report, form, K, M, N):
    inp, r64, r32 = _refs(M, N, K)
    got, route = _run(ctx, form, inp)
    assert route == (0 if form == "rm" else 1), route
    again, _ = _run(ctx, form, inp)
    assert np.array_equal(bits(got), bits(again)), "not bit-identical on a repeated call"
    _check(report, f"{form}_K{K}_M{M}_N{N}", got, r64, r32)


@pytest.mark.parametrize("K,M,N", SR.LAT_SHAPES, ids=SHAPE_IDS)
def test_lat_gemm_forms_agree_bitwise(ctx, K, M, N):
    """row-major, the two-range launcher with both ranges reaching K, k-group-major W, k-group-major W and X: the same partial
    tiles added in the same order"""
    inp = SR.lat_inputs(M, N, K)
    base, _ = _run(ctx, "rm", inp)
    two, route = _run(ctx, "rm", inp, nsplit=16 if N > 16 else N, K2=K)
    assert route == 0 and np.array_equal(bits(base), bits(two)), "two-range form"
    for form in ("wk4", "wk4xk4"):
        other, _ = _run(ctx, form, inp)
        assert np.array_equal(bits(base), bits(other)), form


@pytest.mark.parametrize("form", SR.LAT_FORMS)
def test_lat_gemm_small_integers_are_exact(ctx, form):
    for K, M, N in SR.LAT_SHAPES:
        inp = SR.lat_inputs(M, N, K, small_int=True)
        got, _ = _run(ctx, form, inp)
        assert np.array_equal(got.astype(np.float64), SR.lat_gemm(inp)["y"]), (form, K, M, N)


@pytest.mark.parametrize("M,N,K,nsplit,K2", SR.LAT2_CASES)
def test_lat_gemm_two_ranges(ctx, report, M, N, K, nsplit, K2):
    """the columns from nsplit on contract only k < K2 (launch_linear_f32_lat2 with nsplit < N: no production caller left); they
    equal, bit for bit, a launch of their own over K2"""
    inp, r64, r32 = _refs(M, N, K, nsplit, K2)
    got, route = _run(ctx, "rm", inp, nsplit=nsplit, K2=K2)
    assert route == 0
    _check(report, f"two_range_K{K}_K2{K2}", got, r64, r32)
    tail = dict(X=np.ascontiguousarray(inp["X"][:, :K2]), W=np.ascontiguousarray(inp["W"][nsplit:, :K2]), b=inp["b"][nsplit:])
    alone, route = _run(ctx, "rm", tail)
    assert route == 0 and np.array_equal(bits(got[:, nsplit:]), bits(alone))
    small = SR.lat_inputs(M, N, K, small_int=True)
    assert np.array_equal(_run(ctx, "rm", small, nsplit=nsplit, K2=K2)[0].astype(np.float64), SR.lat_gemm(small, nsplit=nsplit, K2=K2)["y"])


@pytest.mark.parametrize("tag,M,N,K,xoff,want", SR.LAT_ROUTE_CASES, ids=[c[0] for c in SR.LAT_ROUTE_CASES])
def test_lat_gemm_dispatch_boundaries(ctx, report, tag, M, N, K, xoff, want):
    """K = 124 | 128, X one float off a 16-byte boundary, 4096 | 4160 tiles: the latency kernel on one side, launch_linear_f32 on the
    other, both within the bar"""
    inp, r64, r32 = _refs(M, N, K)
    got, route = _run(ctx, "rm", inp, xoff=xoff)
    assert route == want, (tag, route)
    _check(report, f"route_{tag}", got, r64, r32)


def test_lat_gemm_without_bias(ctx, report):
    K, M, N = SR.LAT_SHAPES[2]
    inp, r64, r32 = _refs(M, N, K, bias=False)
    for form in SR.LAT_FORMS:
        _check(report, f"{form}_nobias_K{K}_M{M}_N{N}", _run(ctx, form, inp, bias=False)[0], r64, r32)


def test_hook_refuses_what_it_cannot_launch(ctx):
    L = _lib()
    t = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p, n = L.ptr(t), L.ptr(None)
    call = lambda *a: ctx.lib.tn_dbg_linear_lat(ctx.handle, *a, None)
    #             form X  ldx  W  ldw bias Y ldy  M   N   K  nsplit K2
    bad = [(0, n, 128, p, 128, n, p, 16, 3, 16, 128, 16, 0),           # null X
           (0, p, 124, p, 128, n, p, 16, 3, 16, 128, 16, 0),           # ldx below K
           (0, p, 128, p, 124, n, p, 16, 3, 16, 128, 16, 0),           # ldw below K
           (0, p, 128, p, 128, n, p, 15, 3, 16, 128, 16, 0),           # ldy below N
           (0, p, 128, p, 128, n, p, 32, 3, 32, 128, 8, 64),           # nsplit not a multiple of 16
           (0, p, 128, p, 128, n, p, 32, 3, 32, 128, 16, 130),         # K2 above K
           (0, p, -8, p, 128, n, p, 16, 3, 16, 128, 16, 0),            # the row-major launcher takes no k-group-major X
           (1, p, -2, p, 128, n, p, 16, 3, 16, 128, 16, 0),            # k-group-major rows below M
           (1, p, 132, p, 130, n, p, 16, 3, 16, 130, 16, 0),           # K % 4 != 0
           (1, p, 130, p, 128, n, p, 16, 3, 16, 128, 16, 0),           # ldx % 4 != 0
           (1, C.c_void_p(t.data_ptr() + 4), 128, p, 128, n, p, 16, 3, 16, 128, 16, 0),   # X off a 16-byte boundary
           (1, p, 128, p, 128, n, p, 32, 3, 32, 128, 16, 64),          # no column split in the k-group-major form
           (2, p, 128, p, 128, n, p, 16, 3, 16, 128, 16, 0)]           # no such form
    for args in bad:
        assert call(*args) != 0, args
    assert not t.any()
