"""-m gpu: the head (BatchNorm + ReLU + 7x7 average) folded into its two producers, each kernel on its own.

  * trans_ws_kernel<NK, 64, 512, true> (csrc/trans_ws.hip) through tn_dbg_conv1x1_head: a 14 x 14 -> 7 x 7 transition whose workgroup
    writes the frame's features 0 ... 511 instead of the fp32 copy of its result;
  * dense_block7_kernel<6, true> (csrc/dense_block7.hip) through tn_dbg_block7_run_head: every layer writes the features of the 32
    channels it appends.

Either is held to the launch it replaces: the same kernel writing the fp32 copy (y32 / side), then head_kernel<true> on that copy
(tn_dbg_head).  The fused kernels apply head_kernel's operations to the same fp32 values in head_kernel's order - per channel one
chain over the pixels 0 ... 48, then the 1 / 49 - so the features are the same BITS, and so is the fp16 buffer.  Feature columns a
kernel does not own keep their sentinel, and a NaN-filled side buffer handed to the fused launch comes back untouched.  The features
also meet the bound tests/test_gpu_stem_head.py::test_head_against_float64 holds head_kernel to, against a float64 head of the
unfused fp32 map.

Data: the noisy generators of tests/tools (layerwise_ref.noisy, block_ref.noisy: Gaussian data with large values planted at the seams,
different in every frame), the head's scale negative in about one channel in eight."""
import ctypes as C

import numpy as np
import pytest
import torch

from tools import block_ref as BR
from tools import layerwise_ref as LR

pytestmark = pytest.mark.gpu

LDC = 1024          # row pitch of the last block's buffer, and of the feature rows
FEAT_SENTINEL = np.float32(-3.0)


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _head_consts(seed):
    rng = np.random.default_rng([seed, 10])
    s = (rng.uniform(0.5, 1.5, LDC) * np.where(rng.random(LDC) < 0.125, -1.0, 1.0)).astype(np.float32)
    t = rng.normal(0, 0.3, LDC).astype(np.float32)
    assert 0.05 < (s < 0).mean() < 0.25
    return s, t


def _head64(x64, scale, shift):
    """float64 head of a (B, 49, C) map -> (features (B, C), mean |terms| (B, C))"""
    terms = np.maximum(x64 * scale.astype(np.float64) + shift.astype(np.float64), 0.0)
    return terms.mean(axis=1), np.abs(terms).mean(axis=1)


def _meets_float64_bound(got, x32, scale, shift, what):
    ref, mag = _head64(x32.astype(np.float64), scale, shift)
    ulp32 = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 23)
    bound = 64 * 2.0 ** -24 * mag + ulp32
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: max err / bound %.3f (max err %.3g)" % (what, (err / bound).max(), err.max()))
    return bool(np.all(err <= bound))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    v = np.uint16 if a.dtype == np.float16 else np.uint32
    return a.shape == b.shape and np.array_equal(a.view(v), b.view(v))


def _head_dev(ctx, x32d, b, c, sd, td):
    """head_kernel<true> on a device (B, 7, 7, c) fp32 map (the fp16 pointer poisoned) -> (B, c) numpy"""
    from tennis_amd import _lib
    poison = torch.full((b, 7, 7, c), float("nan"), dtype=torch.float16, device="cuda")
    fd = torch.full((b, c), float(FEAT_SENTINEL), dtype=torch.float32, device="cuda")
    _lib.check(ctx.lib.tn_dbg_head(ctx.handle, _lib.ptr(poison), _lib.ptr(x32d), b, 7, 7, c, _lib.ptr(sd), _lib.ptr(td), _lib.ptr(fd), 1, 1), "tn_dbg_head")
    return fd.cpu().numpy()


# ---- the last transition ----------------------------------------------------------------------------------------------------------------
def _trans_inputs(k, b, h=14, n=512):
    c = LR._case("ws", ("trans_ws_kernel", (16 if k == 1024 else 0, 64, 512)), "noisy", N=n, K=k, B=b, H=h, W=h)
    return c, LR.noisy(c)


def _trans_operands(ctx, c, inp):
    w16 = LR.weight_rows(inp)
    frag = np.empty(w16.size, np.float16)
    assert ctx.lib.tn_dbg_pack_trans_frags(_vp(np.ascontiguousarray(w16)), c["N"], c["K"], _vp(frag)) == 0
    return (torch.from_numpy(LR.x_buffer(c, inp)).cuda(), _dev(inp["s"]), _dev(inp["t"]), torch.from_numpy(w16).cuda(), torch.from_numpy(frag).cuda())


def _ybuf(c):
    y = np.full((c["M"], LDC), LR.SENTINEL, np.float16)
    y[:, :c["N"]] = LR.STALE
    return y


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("k", [128, 1024])
def test_transition_features_are_the_unfused_bits(ctx, k, b):
    from tennis_amd import _lib
    lib, n = ctx.lib, 512
    c, inp = _trans_inputs(k, b)
    assert c["M"] == b * 49
    xd, s, t, wd, frag = _trans_operands(ctx, c, inp)
    hs, ht = _head_consts(k + b)
    hsd, htd = _dev(hs), _dev(ht)
    # unfused: the fp32 copy (pitch n), then the head kernel on it
    yd0 = torch.from_numpy(_ybuf(c)).cuda()
    y32d = torch.full((c["M"], n), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.tn_dbg_conv1x1_ex(ctx.handle, _lib.ptr(xd), LR.ldx_of(c), k, _lib.ptr(s), _lib.ptr(t), _lib.ptr(wd), n, _lib.ptr(yd0), LDC, 0, c["M"], 1,
                                     14, 14, 0, None, 0, _lib.ptr(y32d), n, _lib.ptr(frag)), "tn_dbg_conv1x1_ex")
    torch.cuda.synchronize()
    want = _head_dev(ctx, y32d, b, n, hsd, htd)
    # fused: features straight from the kernel; the side buffer it is handed stays what it was
    yd1 = torch.from_numpy(_ybuf(c)).cuda()
    side = torch.full((c["M"], n), float("nan"), dtype=torch.float32, device="cuda")
    fd = torch.full((b, LDC), float(FEAT_SENTINEL), dtype=torch.float32, device="cuda")
    _lib.check(lib.tn_dbg_conv1x1_head(ctx.handle, _lib.ptr(xd), LR.ldx_of(c), k, _lib.ptr(s), _lib.ptr(t), _lib.ptr(wd), n, _lib.ptr(yd1), LDC, 0, c["M"], 1,
                                       14, 14, _lib.ptr(side), n, _lib.ptr(frag), _lib.ptr(fd), _lib.ptr(hsd), _lib.ptr(htd), LDC), "tn_dbg_conv1x1_head")
    torch.cuda.synchronize()
    got = fd.cpu().numpy()
    assert np.isfinite(got).all()
    assert _same(got[:, :n], want)
    assert np.all(got[:, n:] == FEAT_SENTINEL)
    y0, y1 = yd0.cpu().numpy(), yd1.cpu().numpy()
    assert _same(y1, y0)
    assert np.all(y1[:, n:] == LR.SENTINEL) and (y1[:, :n] == LR.STALE).mean() < 0.01          # (overwritten; a result may be -77 itself)
    assert bool(torch.isnan(side).all())
    x32 = y32d.cpu().numpy().reshape(b, 49, n)
    assert np.isfinite(x32).all() and len({x32[f].tobytes() for f in range(b)}) == b
    assert _meets_float64_bound(got[:, :n], x32, hs[:n], ht[:n], "transition K = %d, B = %d" % (k, b))


@pytest.mark.parametrize("h,n,word", [(28, 512, "one 49-pixel tile"), (14, 256, "N = 512")], ids=["two_tiles_per_frame", "N256"])
def test_transition_refusals_launch_nothing(ctx, h, n, word):
    from tennis_amd import _lib
    lib, k, b = ctx.lib, 128, 2
    c, inp = _trans_inputs(k, b, h, n)
    xd, s, t, wd, frag = _trans_operands(ctx, c, inp)
    hs, ht = _head_consts(0)
    hsd, htd = _dev(hs), _dev(ht)
    yd = torch.from_numpy(_ybuf(c)).cuda()
    fd = torch.full((b, LDC), float(FEAT_SENTINEL), dtype=torch.float32, device="cuda")
    rc = lib.tn_dbg_conv1x1_head(ctx.handle, _lib.ptr(xd), LR.ldx_of(c), k, _lib.ptr(s), _lib.ptr(t), _lib.ptr(wd), n, _lib.ptr(yd), LDC, 0, c["M"], 1,
                                 h, h, None, 0, _lib.ptr(frag), _lib.ptr(fd), _lib.ptr(hsd), _lib.ptr(htd), LDC)
    assert rc != 0
    msg = lib.tn_last_error().decode()
    assert "head epilogue" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((fd == float(FEAT_SENTINEL)).all())
    assert _same(yd.cpu().numpy(), _ybuf(c))


# ---- the 7x7 block ------------------------------------------------------------------------------------------------------------------------
class Block7:
    def __init__(self, ctx, k0, layers):
        from tennis_amd import _lib
        self.lib, self.handle = ctx.lib, C.c_void_p()
        cat = lambda name: np.ascontiguousarray(np.concatenate([np.asarray(p[name], np.float32).ravel() for p in layers]))
        ops = [cat(nm) for nm in ("w1", "lo", "hi", "s2", "t2", "w3")]
        _lib.check(ctx.lib.tn_dbg_block7_create(ctx.handle, k0, len(layers), *[_vp(o) for o in ops], C.byref(self.handle)), "tn_dbg_block7_create")

    def run(self, d, b, side=None, feat=None, hs=None, ht=None):
        from tennis_amd import _lib
        _lib.check(self.lib.tn_dbg_block7_run_head(self.handle, _lib.ptr(d), LDC, b, _lib.ptr(side), _lib.ptr(feat), _lib.ptr(hs), _lib.ptr(ht), LDC, None),
                   "tn_dbg_block7_run_head")
        torch.cuda.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.tn_dbg_block7_destroy(self.handle)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("k0,nl", [(448, 1), (448, 2), (512, 16)])
def test_block_features_are_the_unfused_bits(ctx, k0, nl, b):
    x, layers = BR.noisy(7, k0, nl, b, 0)
    buf = BR.buffer(x, LDC, 32 * nl)
    own = slice(k0, k0 + 32 * nl)
    hs, ht = _head_consts(k0 + nl + b)
    hsd, htd = _dev(hs), _dev(ht)
    with Block7(ctx, k0, layers) as blk:
        # unfused: the fp32 side copy of the appended channels (zero elsewhere), then the head kernel over all 1024 channels
        d0 = torch.from_numpy(buf).cuda()
        side0 = torch.zeros((b, 49, LDC), dtype=torch.float32, device="cuda")
        blk.run(d0, b, side=side0)
        want = _head_dev(ctx, side0, b, LDC, hsd, htd)
        # fused
        d1 = torch.from_numpy(buf).cuda()
        side1 = torch.full((b, 49, LDC), float("nan"), dtype=torch.float32, device="cuda")
        fd = torch.full((b, LDC), float(FEAT_SENTINEL), dtype=torch.float32, device="cuda")
        blk.run(d1, b, side=side1, feat=fd, hs=hsd, ht=htd)
    got = fd.cpu().numpy()
    assert np.isfinite(got).all()
    assert _same(got[:, own], want[:, own])
    keep = np.ones(LDC, bool)
    keep[own] = False
    assert np.all(got[:, keep] == FEAT_SENTINEL)
    o0, o1 = d0.cpu().numpy(), d1.cpu().numpy()
    assert _same(o1, o0)
    assert _same(o1[..., keep], buf[..., keep]) and (o1[..., own] == BR.STALE).mean() < 0.01      # (overwritten; a result may be -77 itself)
    assert bool(torch.isnan(side1).all())
    x32 = side0.cpu().numpy()[..., own]
    assert np.isfinite(x32).all() and len({x32[f].tobytes() for f in range(b)}) == b
    assert _meets_float64_bound(got[:, own], x32, hs[own], ht[own], "block K0 = %d, nl = %d, B = %d" % (k0, nl, b))


def test_block_refuses_head_fields_that_do_not_fit(ctx):
    x, layers = BR.noisy(7, 448, 1, 1, 0)
    from tennis_amd import _lib
    hs, ht = _head_consts(1)
    hsd, htd = _dev(hs), _dev(ht)
    with Block7(ctx, 448, layers) as blk:
        d = torch.from_numpy(BR.buffer(x, LDC, 32)).cuda()
        fd = torch.full((1, LDC), float(FEAT_SENTINEL), dtype=torch.float32, device="cuda")
        for args in ((_lib.ptr(fd), None, _lib.ptr(htd), LDC), (_lib.ptr(fd), _lib.ptr(hsd), _lib.ptr(htd), 448)):
            rc = ctx.lib.tn_dbg_block7_run_head(blk.handle, _lib.ptr(d), LDC, 1, None, *args, None)
            assert rc != 0 and "head epilogue" in ctx.lib.tn_last_error().decode()
        torch.cuda.synchronize()
        assert bool((fd == float(FEAT_SENTINEL)).all())
        assert _same(d.cpu().numpy(), BR.buffer(x, LDC, 32))
