"""-m gpu: every instantiation of the strip-streaming fused dense layer (dense_strip_kernel<W, KS>, csrc/dense_strip_impl.h) on its own,
through tn_dbg_pack_strip and tn_dbg_dense_strip_dev, against the float64 reference and the derived bound of
tests/tools/strip_ref.py (what the bound can and cannot see: tests/test_cpu_strip_ref.py).

All 35 (W, K) that dense_strip_supported accepts - each K / 32 has a compile-time schedule, ring depth and LDS map of its own, odd
K / 32 a half super-step with another channel mapping, and each keeps its bottleneck window in literal accumulator registers:
  * `noisy` inputs (large magnitudes planted on both sides of every frame border, strip seam, chunk seam and in the partly empty
    last strip pair) inside the componentwise bound, max |y_dev - y| / E <= 1, everything outside the 32 output channels untouched;
  * `integer` inputs reproduced bit for bit;
  * more workgroups than CUs: a frame's bits do not depend on its place in the batch, nor on the launch;
  * what dense_strip_supported or the channel geometry rules out is refused with a message that names it.

Measured worst ratios: docs/numerics.md "The strip kernel, every instantiation"."""
import ctypes as C

import numpy as np
import pytest
import torch

from tools import strip_ref as SR

pytestmark = pytest.mark.gpu

IDS = ["%d-%d" % c for c in SR.SUPPORTED]
SENTINEL = np.float16(300.0)       # behind the output channels: never read, never written
STALE = np.float16(-77.0)          # in the output channels: has to be overwritten


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _pack(ctx, inp):
    """-> the device operands of a case: (lo, hi, w1s, w3s) tensors"""
    from tennis_amd import _lib
    k = inp["x"].shape[-1]
    w1s = np.empty((k + 16) * 128, np.uint16)
    w3s = np.empty(36864, np.uint16)
    w1, s2, t2, w3 = (np.ascontiguousarray(inp[n], np.float32) for n in ("w1", "s2", "t2", "w3"))
    _lib.check(ctx.lib.tn_dbg_pack_strip(_vp(w1), k, _vp(s2), _vp(t2), _vp(w1s), _vp(w3), _vp(w3s)), "pack_strip")
    return (torch.from_numpy(np.ascontiguousarray(inp["lo"], np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(inp["hi"], np.float32)).cuda(),
            torch.from_numpy(w1s.view(np.int16)).cuda(), torch.from_numpy(w3s.view(np.int16)).cuda())


def _buffer(x, ldc):
    """(B,W,W,K) fp16 -> the (B,W,W,ldc) concat buffer: input | STALE where the output goes | SENTINEL"""
    k = x.shape[-1]
    buf = np.full(x.shape[:3] + (ldc,), SENTINEL, np.float16)
    buf[..., :k] = x
    buf[..., k:k + 32] = STALE
    return buf


def _launch(ctx, ops, buf_d, ldc, k, b, w):
    from tennis_amd import _lib
    lo, hi, w1s, w3s = ops
    _lib.check(ctx.lib.tn_dbg_dense_strip_dev(ctx.handle, _lib.ptr(buf_d), ldc, k, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(w1s), _lib.ptr(w3s),
                                              b, w, w, None), "dense_strip")
    torch.cuda.synchronize()


def _run(ctx, inp, ldc):
    """one launch on a fresh buffer -> (the buffer as it went in, as it came out), numpy fp16"""
    b, w, _, k = inp["x"].shape
    buf = _buffer(inp["x"], ldc)
    d = torch.from_numpy(buf).cuda()
    _launch(ctx, _pack(ctx, inp), d, ldc, k, b, w)
    return buf, d.cpu().numpy()


def _untouched(buf, out, k):
    keep = np.ones(buf.shape[-1], bool)
    keep[k:k + 32] = False
    return np.array_equal(out[..., keep].view(np.uint16), buf[..., keep].view(np.uint16))


@pytest.mark.parametrize("w,k", SR.SUPPORTED, ids=IDS)
def test_every_instantiation_against_float64(ctx, report, w, k):
    """`noisy` inputs, B = 2 (W <= 56) or 1, the smallest legal row pitch for odd K / 32 and one line more otherwise."""
    b = 2 if w <= 56 else 1
    ldc = SR.case_ldc(k)
    inp = SR.noisy(w, k, b, 0)
    y, bound = SR.reference(inp)
    buf, out = _run(ctx, inp, ldc)
    got = out[..., k:k + 32].astype(np.float64)
    q = np.abs(got - y) / bound
    r = float(q.max())
    report[f"dense_strip_f64_ratio_W{w}_K{k}"] = r
    print("dense_strip<%d, %d>: max |err| / E = %.3f at %s, max |err| = %.3g, |y| max %.3g" % (w, k // 32, r, np.unravel_index(q.argmax(), q.shape),
                                                                                          np.abs(got - y).max(), np.abs(y).max()))
    assert np.isfinite(got).all()
    assert r <= 1.0, (r, np.argwhere(q > 1.0)[:8].tolist())
    assert _untouched(buf, out, k)


@pytest.mark.parametrize("w,k", SR.SUPPORTED, ids=IDS)
def test_every_instantiation_integer_exact(ctx, w, k):
    """`integer` inputs: every product, sum and rounding is exact, so the device's halves are the integers' halves."""
    b = 2 if w <= 56 else 1
    inp = SR.integer(w, k, b, 0)
    y, _ = SR.reference(inp)
    buf, out = _run(ctx, inp, SR.case_ldc(k))
    want = y.astype(np.float16)
    got = out[..., k:k + 32]
    same = got.view(np.uint16) == want.view(np.uint16)
    if not same.all():
        bad = np.argwhere(~same)
        print("dense_strip<%d, %d>: %d of %d outputs differ; first (frame, row, column, channel): %s" % (w, k // 32, len(bad), same.size, bad[:8].tolist()))
        for f, r_, c_, o in bad[:8]:
            print("  (%d, %d, %d, %d): device %g, exact %g" % (f, r_, c_, o, float(got[f, r_, c_, o]), float(want[f, r_, c_, o])))
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert _untouched(buf, out, k)


@pytest.mark.parametrize("w,k,b", [(28, 160, 300), (64, 128, 90)], ids=["28-160-B300", "64-128-B90"])
def test_more_workgroups_than_cus_and_batch_position(ctx, w, k, b):
    """300 / 270 workgroups on 256 CUs: the same frame first and last in the batch gives the same bits, the bits of a launch of that
    frame alone, and a second launch on a fresh copy of the batch reproduces the first."""
    ldc = SR.case_ldc(k)
    inp = SR.noisy(w, k, 1, 1)
    ops = _pack(ctx, inp)
    frame = torch.from_numpy(_buffer(inp["x"], ldc)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(w * 1000 + k)
    batch = (torch.randn((b, w, w, ldc), generator=g, device="cuda", dtype=torch.float32) * 1.5).to(torch.float16)
    batch[0] = frame[0]
    batch[b - 1] = frame[0]
    first, second, alone = batch.clone(), batch.clone(), frame.clone()
    _launch(ctx, ops, first, ldc, k, b, w)
    _launch(ctx, ops, second, ldc, k, b, w)
    _launch(ctx, ops, alone, ldc, k, 1, w)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(first[0]), bits(first[b - 1]))
    assert torch.equal(bits(first[0]), bits(alone[0]))
    assert torch.equal(bits(first), bits(second))
    keep = torch.ones(ldc, dtype=torch.bool, device="cuda")
    keep[k:k + 32] = False
    assert torch.equal(bits(first[..., keep]), bits(batch[..., keep]))
    # and the frame is the right one, not merely the same one three times
    y, bound = SR.reference(inp)
    assert SR.ratio(alone[0, :, :, k:k + 32].cpu().numpy()[None], y, bound) <= 1.0
    # every workgroup stored its frame: (nearly) no output half is the random number that was there before
    written = (bits(first[..., k:k + 32]) != bits(batch[..., k:k + 32])).float().mean(dim=(1, 2, 3))
    assert torch.isfinite(first[..., k:k + 32].float()).all() and float(written.min()) > 0.99, float(written.min())


REFUSED = [  # (W, K, ldc, what the message has to name)
    (128, 320, 384, ("128 x 128", "K = 320")),       # the instantiation that spills one register
    (56, 32, 64, ("56 x 56", "K = 32")),
    (28, 352, 384, ("28 x 28", "K = 352")),
    (56, 80, 128, ("56 x 56", "K = 80")),
    (14, 128, 192, ("14 x 14", "K = 128")),
    (28, 128, 128, ("K = 128", "ldc = 128")),        # ldc < K + 32
    (56, 96, 160, ("K = 96", "ldc = 160")),          # ldc % 64 != 0
]


def test_unsupported_geometries_are_refused(ctx):
    from tennis_amd import _lib
    dummy = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    f32 = torch.zeros(512, dtype=torch.float32, device="cuda")
    for w, k, ldc, names in REFUSED:
        rc = ctx.lib.tn_dbg_dense_strip_dev(ctx.handle, _lib.ptr(dummy), ldc, k, _lib.ptr(f32), _lib.ptr(f32), _lib.ptr(dummy), _lib.ptr(dummy), 1, w, w, None)
        assert rc != 0, (w, k, ldc)
        with pytest.raises(RuntimeError) as ei:
            _lib.check(rc, "dense_strip")
        msg = str(ei.value)
        assert "dense_strip" in msg and all(n in msg for n in names), (w, k, ldc, msg)
    torch.cuda.synchronize()
    assert not dummy.any()                                     # nothing was launched
    # a good call afterwards still works
    inp = SR.integer(28, 64, 1, 2)
    y, _ = SR.reference(inp)
    _, out = _run(ctx, inp, SR.case_ldc(64))
    assert np.array_equal(out[..., 64:96].view(np.uint16), y.astype(np.float16).view(np.uint16))
