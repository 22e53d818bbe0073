"""-m gpu: the paired launch geometry of the 28x28 strip kernels (csrc/dense_strip_pair_w28.hip: two frames per workgroup, each wave
walks half a frame, 14 rows) against the one-frame launch (dense_strip_kernel<28, KS>: four waves, seven rows each) on the same input.

Both run the layer body of dense_strip_body.h with the same LDS map, slot schedules and window registers: per output the same
arithmetic in the same order, so the bar is BIT identity over the whole concat buffer, no tolerance (the one-frame kernels are held
to float64 by tests/test_gpu_strip_instantiations.py).  What the paired form could get wrong is its geometry: the frame a wave works
on, its row range, and the seam between the two halves of a frame - both waves recompute bottleneck rows 13 and 14 themselves - so
rows 13 and 14 are looked at first, the two frames of a workgroup hold different data, and the inputs carry |x| in [20, 60] on both
sides of that seam and of the frame borders (tools/tile_ref.py::noisy_x: the row-tile seam of the 28x28 tile kernel is the same
line).  Parameters: tile_ref's noisy ones (clamp constants of all three kinds) with one BatchNorm scale in eight negative.

Per layer: K = 128 (even K / 32), K = 160 (odd: the trailing half super-step) and K = 320 (the widest body: 256 VGPRs), at B = 2
(one workgroup) and B = 4 (two); the chain: K0 = 128, six layers in one launch against six one-frame launches in order, B = 2.
An odd B is refused with an error and nothing is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from tools import tile_ref as TR

pytestmark = pytest.mark.gpu

W, LDC = 28, 512
SENTINEL = np.float16(300.0)       # behind the output channels: never read, never written
STALE = np.float16(-77.0)          # where outputs go: has to be overwritten


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _negate_one_scale_in_eight(p):
    s2 = p["s2"].copy()
    s2[3::8] *= -1.0
    return dict(p, s2=s2)


def _pack(ctx, p):
    """one layer's device operands: (lo, hi, w1s, w3s) tensors"""
    from tennis_amd import _lib
    k = p["w1"].shape[1]
    w1s = np.empty((k + 16) * 128, np.uint16)
    w3s = np.empty(36864, np.uint16)
    w1, s2, t2, w3 = (np.ascontiguousarray(p[n], np.float32) for n in ("w1", "s2", "t2", "w3"))
    _lib.check(ctx.lib.tn_dbg_pack_strip(_vp(w1), k, _vp(s2), _vp(t2), _vp(w1s), _vp(w3), _vp(w3s)), "pack_strip")
    return (torch.from_numpy(np.ascontiguousarray(p["lo"], np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(p["hi"], np.float32)).cuda(),
            torch.from_numpy(w1s.view(np.int16)).cuda(), torch.from_numpy(w3s.view(np.int16)).cuda())


def _buffer(x, nout):
    """(B,28,28,K) fp16 -> the (B,28,28,512) concat buffer: input | STALE where the outputs go | SENTINEL"""
    k = x.shape[-1]
    buf = np.full(x.shape[:3] + (LDC,), SENTINEL, np.float16)
    buf[..., :k] = x
    buf[..., k:k + nout] = STALE
    return torch.from_numpy(buf).cuda()


def _one_frame(ctx, ops, buf, k, b):
    from tennis_amd import _lib
    lo, hi, w1s, w3s = ops
    _lib.check(ctx.lib.tn_dbg_dense_strip_dev(ctx.handle, _lib.ptr(buf), LDC, k, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(w1s), _lib.ptr(w3s),
                                              b, W, W, None), "dense_strip")


def _paired_rc(ctx, ops, buf, k, b):
    from tennis_amd import _lib
    lo, hi, w1s, w3s = ops
    return ctx.lib.tn_dbg_dense_strip_pair_dev(ctx.handle, _lib.ptr(buf), LDC, k, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(w1s), _lib.ptr(w3s),
                                               b, W, W, None)


def _launches(ctx):
    n = C.c_int64(-1)
    assert ctx.lib.tn_dbg_strip_pair_launches(C.byref(n)) == 0
    return n.value


def _bits(t):
    return t.view(torch.int16)


def _assert_identical(got, want, k, nout, start):
    """rows 13 and 14 of every frame first (the seam of the paired form), then the whole buffer; and the launch did its work"""
    for row in (13, 14):
        same = _bits(got[:, row]) == _bits(want[:, row])
        assert bool(same.all()), "row %d: %d values differ, first (frame, column, channel) %s" % (
            row, int((~same).sum()), (~same).nonzero()[:4].tolist())
    same = _bits(got) == _bits(want)
    assert bool(same.all()), "%d values differ, first (frame, row, column, channel) %s" % (int((~same).sum()), (~same).nonzero()[:4].tolist())
    out = got[..., k:k + nout].float()
    assert bool(torch.isfinite(out).all())
    assert float((_bits(got[..., k:k + nout]) != _bits(start[..., k:k + nout])).float().mean()) > 0.99       # overwritten
    keep = torch.ones(LDC, dtype=torch.bool, device="cuda")
    keep[k:k + nout] = False
    assert torch.equal(_bits(got[..., keep]), _bits(start[..., keep]))                                         # nothing else touched
    for f in range(1, got.shape[0]):                                                                           # every frame its own data
        assert not torch.equal(_bits(got[f, ..., k:k + nout]), _bits(got[0, ..., k:k + nout]))


@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("k", [128, 160, 320])
def test_paired_layer_is_bit_identical_to_the_one_frame_launch(ctx, k, b):
    inp = TR.noisy(W, k, b, 40)
    ops = _pack(ctx, _negate_one_scale_in_eight(inp))
    start = _buffer(inp["x"], 32)
    assert not torch.equal(start[0], start[1])
    want, got = start.clone(), start.clone()
    _one_frame(ctx, ops, want, k, b)
    n0 = _launches(ctx)
    from tennis_amd import _lib
    _lib.check(_paired_rc(ctx, ops, got, k, b), "dense_strip_pair")
    torch.cuda.synchronize()
    assert _launches(ctx) == n0 + 1
    _assert_identical(got, want, k, 32, start)


def test_paired_chain_is_bit_identical_to_six_one_frame_launches(ctx):
    from tennis_amd import _lib
    k0, nl, b = 128, 6, 2
    x, layers = TR.chain_noisy(W, k0, nl, b, 41)
    ops = [_pack(ctx, _negate_one_scale_in_eight(p)) for p in layers]
    start = _buffer(x, 32 * nl)
    want, got = start.clone(), start.clone()
    for l in range(nl):
        _one_frame(ctx, ops[l], want, k0 + 32 * l, b)
    arr = [(C.c_void_p * nl)(*[o[i].data_ptr() for o in ops]) for i in range(4)]
    n0 = _launches(ctx)
    _lib.check(ctx.lib.tn_dbg_dense_strip_pair_chain_dev(ctx.handle, _lib.ptr(got), LDC, k0, nl, arr[0], arr[1], arr[2], arr[3], b, W, W),
               "dense_strip_pair_chain")
    torch.cuda.synchronize()
    assert _launches(ctx) == n0 + 1
    _assert_identical(got, want, k0, 32 * nl, start)


def test_an_odd_batch_is_refused_without_a_launch(ctx):
    from tennis_amd import _lib
    k = 128
    inp = TR.noisy(W, k, 3, 42)
    ops = _pack(ctx, inp)
    start = _buffer(inp["x"], 32)
    buf = start.clone()
    n0 = _launches(ctx)
    rc = _paired_rc(ctx, ops, buf, k, 3)
    assert rc != 0
    with pytest.raises(RuntimeError) as ei:
        _lib.check(rc, "dense_strip_pair")
    assert "odd batch" in str(ei.value)
    arr = [(C.c_void_p * 6)(*[ops[i].data_ptr()] * 6) for i in range(4)]
    rc = ctx.lib.tn_dbg_dense_strip_pair_chain_dev(ctx.handle, _lib.ptr(buf), LDC, 128, 6, arr[0], arr[1], arr[2], arr[3], 3, W, W)
    assert rc != 0 and "odd batch" in ctx.lib.tn_last_error().decode()
    # other maps and other channel counts are not the paired kernels' either
    assert ctx.lib.tn_dbg_dense_strip_pair_dev(ctx.handle, _lib.ptr(buf), LDC, 64, _lib.ptr(ops[0]), _lib.ptr(ops[1]), _lib.ptr(ops[2]),
                                               _lib.ptr(ops[3]), 2, W, W, None) != 0
    assert ctx.lib.tn_dbg_dense_strip_pair_dev(ctx.handle, _lib.ptr(buf), LDC, k, _lib.ptr(ops[0]), _lib.ptr(ops[1]), _lib.ptr(ops[2]),
                                               _lib.ptr(ops[3]), 2, 56, 56, None) != 0
    torch.cuda.synchronize()
    assert _launches(ctx) == n0
    assert torch.equal(_bits(buf), _bits(start))                # nothing was launched
