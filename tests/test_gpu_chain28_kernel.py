"""-m gpu: the chained tile kernel over the two row tiles of a 28x28 frame, dense_layer_kernel<28, 14, 512, 32, 2, true>
(csrc/dense_layer_big.hip, `MT`), on its own through tn_dbg_dense_chain_dev.

One workgroup is one frame and walks frame -> layer -> row tile.  What the chained form can get wrong that a per-layer launch cannot is
the seam between the two tiles: layer l + 1, tile 0 reads output row 14 of layer l, which tile 1 of layer l stored from the same
workgroup, and tile 1 of layer l reads as its halo the channels [0, K) of row 13, whose channels [K, K + 32) tile 0 has just stored.  So:

  * the chained launch against `nl` per-layer launches of dense_layer_kernel<28, 14, 512, 32, 2, false> on a copy: the whole concat
    buffer bit for bit, rows 13 / 14 asserted on their own first so that a seam fault names itself;
  * the chained launch against the float64 reference of tests/tools/tile_ref.py at the bar of tests/test_gpu_tile_instantiations.py
    (max |y_dev - y| / E <= 1 with the derived componentwise bound E), every layer from the device's own final buffer - the concat
    only appends, so buf[..., :K0 + 32 l] is exactly what layer l read;
  * nothing outside the chain's output channels is touched.

Shapes: ldc = 512 (the block's own pitch: 128-byte lines hold 64 channels, so K % 64 == 32 puts a layer's output into the line its
input ends in); B = 2 and 3 (an odd grid); K0 = 352, nl = 5 (the network's chain), K0 = 64, nl = 2 (the first layer sits at the
2 BK <= K edge of the k-tiles requested ahead), K0 = 480, nl = 1.  Parameters in tile_ref's `noisy` distribution (clamp constants of
all three kinds, |x| in [20, 60] planted on rows 0, 13, 14, 27, the border columns and the wave / fragment seams) with one BatchNorm
scale in eight negative."""
import ctypes as C

import numpy as np
import pytest
import torch

from tools import tile_ref as TR

pytestmark = pytest.mark.gpu

H, LDC = 28, 512
SHAPES = [(352, 5), (64, 2), (480, 1)]
CASES = [pytest.param(k0, n, b, id="K%d-n%d-B%d" % (k0, n, b)) for k0, n in SHAPES for b in (2, 3)]
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _pack(ctx, p):
    """one layer's parameters -> its device operands in the forms the kernel reads (the 1x1 weights with 64 halves of slack, as the
    encoder's weight pool gives them)"""
    w1 = np.concatenate([p["w1"].astype(np.float16).ravel(), np.zeros(64, np.float16)])
    wp = np.empty(2 * 72 * 64 * 8, np.uint16)
    ctx.lib.tn_dbg_pack_conv3x3(np.ascontiguousarray(p["w3"], np.float32).ctypes.data_as(C.c_void_p), wp.ctypes.data_as(C.c_void_p))
    return dict(lo=_dev(p["lo"], np.float32), hi=_dev(p["hi"], np.float32), w1=torch.from_numpy(w1).cuda(), s2=_dev(p["s2"], np.float32),
                t2=_dev(p["t2"], np.float32), wp=torch.from_numpy(wp.view(np.int16)).cuda())


def _inputs(k0, n, b):
    x, layers = TR.chain_noisy(H, k0, n, b, 28)
    rng = np.random.default_rng([28, k0, n, b])
    for p in layers:
        neg = rng.random(128) < 0.125
        assert neg.any()
        p["s2"] = np.where(neg, -p["s2"], p["s2"]).astype(np.float32)
        kinds = (p["lo"] == -TR.F16_MAX).any() and (p["hi"] == TR.F16_MAX).any() and ((p["lo"] == 0) & (p["hi"] == 0)).any()
        assert kinds                                # all three kinds of clamp constants, in every layer of every case
    return x, layers


def _run(ctx, k0, n, b):
    """both launches of a case, once: (the buffer as it went in, the chained launch's, the per-layer launches', the layers)"""
    from tennis_amd import _lib
    key = (k0, n, b)
    if key not in _cache:
        x, layers = _inputs(k0, n, b)
        ops = [_pack(ctx, p) for p in layers]
        buf = TR.buffer(x, LDC, 32 * n)
        chained = torch.from_numpy(buf).cuda()
        per_layer = chained.clone()
        arr = {name: (C.c_void_p * n)(*[_lib.ptr(o[name]) for o in ops]) for name in ("lo", "hi", "w1", "s2", "t2", "wp")}
        _lib.check(ctx.lib.tn_dbg_dense_chain_dev(ctx.handle, _lib.ptr(chained), LDC, k0, n, arr["lo"], arr["hi"], arr["w1"], arr["s2"], arr["t2"],
                                                  arr["wp"], b, H, H, 0), "dense_chain")
        for l, o in enumerate(ops):
            _lib.check(ctx.lib.tn_dbg_dense_layer_dev(ctx.handle, _lib.ptr(per_layer), LDC, k0 + 32 * l, _lib.ptr(o["lo"]), _lib.ptr(o["hi"]),
                                                      _lib.ptr(o["w1"]), _lib.ptr(o["s2"]), _lib.ptr(o["t2"]), _lib.ptr(o["wp"]), b, H, H, None, 0),
                       "dense_layer")
        torch.cuda.synchronize()
        got, want = chained.cpu().numpy(), per_layer.cpu().numpy()
        for a in (buf, got, want):
            a.setflags(write=False)
        _cache[key] = (buf, got, want, layers)
    return _cache[key]


def _differ(got, want):
    d = got.view(np.uint16) != want.view(np.uint16)
    return int(d.sum()), np.argwhere(d)[:8].tolist()


@pytest.mark.parametrize("k0,n,b", CASES)
def test_chained_launch_has_the_bits_of_per_layer_launches(ctx, k0, n, b):
    buf, got, want, _ = _run(ctx, k0, n, b)
    assert np.isfinite(got[..., :k0 + 32 * n].astype(np.float32)).all()
    # the tile seam first: row 13 is tile 0's last output row and tile 1's halo, row 14 tile 1's first and tile 0's halo
    for row in (13, 14):
        nd, where = _differ(got[:, row], want[:, row])
        assert nd == 0, "row %d (tile seam): %d halves differ, first (frame, column, channel): %s" % (row, nd, where)
    nd, where = _differ(got, want)
    assert nd == 0, "%d halves differ, first (frame, row, column, channel): %s" % (nd, where)
    # input channels and the sentinel behind the output are what they were; every output half was stored
    keep = np.ones(LDC, bool)
    keep[k0:k0 + 32 * n] = False
    assert np.array_equal(got[..., keep].view(np.uint16), buf[..., keep].view(np.uint16))
    assert (got[..., ~keep] != TR.STALE).mean() > 0.99


@pytest.mark.parametrize("k0,n,b", CASES)
def test_chained_launch_against_float64(ctx, report, k0, n, b):
    _, got, _, layers = _run(ctx, k0, n, b)
    worst = 0.0
    for l, p in enumerate(layers):
        k = k0 + 32 * l
        y, bound = TR.reference(dict(x=got[..., :k], **p))
        q = np.abs(got[..., k:k + 32].astype(np.float64) - y) / bound
        print("K0 = %d, n = %d, B = %d, layer %d (K = %d): max |err| / E = %.3f at %s; rows 13 / 14: %.3f / %.3f" % (
            k0, n, b, l, k, q.max(), np.unravel_index(q.argmax(), q.shape), q[:, 13].max(), q[:, 14].max()))
        worst = max(worst, float(q.max()))
        assert q[:, 13:15].max() <= 1.0, (l, k, "tile seam", float(q[:, 13:15].max()))
        assert q.max() <= 1.0, (l, k, float(q.max()), np.argwhere(q > 1.0)[:8].tolist())
    report["dense_tile_chain28_f64_ratio_K%d_n%d_B%d" % (k0, n, b)] = worst


def test_what_the_launcher_refuses_of_a_28x28_chain(ctx):
    """a chain of two layers starts at K >= 64 (two k-tiles of 32 channels are requested ahead of a layer's stores); the last layer has to
    fit the table space (K <= 512) and the row pitch; nothing is launched"""
    from tennis_amd import _lib
    dummy = torch.zeros(1 << 20, dtype=torch.float16, device="cuda")
    f32 = torch.zeros(2048, dtype=torch.float32, device="cuda")
    for k0, n, ldc, names in ((32, 2, 512, ("starts at K >= 64", "2 k-tiles of 32", "28 x 28")), (480, 3, 1024, ("28 x 28", "K = 480", "512")),
                              (448, 2, 480, ("28 x 28", "ldc = 480", "nchain = 2"))):
        arr = [(C.c_void_p * n)(*[_lib.ptr(t)] * n) for t in (f32, f32, dummy, f32, f32, dummy)]
        rc = ctx.lib.tn_dbg_dense_chain_dev(ctx.handle, _lib.ptr(dummy), ldc, k0, n, *arr, 1, H, H, 0)
        assert rc != 0, (k0, n, ldc)
        with pytest.raises(RuntimeError) as ei:
            _lib.check(rc, "dense_chain")
        assert all(s in str(ei.value) for s in names), str(ei.value)
    torch.cuda.synchronize()
    assert not dummy.any()
