"""-m gpu: every instantiation of the fused TILE kernel (dense_layer_kernel<W, ROUT, BM, BK, PP, CHAIN, EX>, csrc/dense_layer_big.hip) on its
own, through tn_dbg_dense_layer_dev and - chained launches - tn_dbg_dense_chain_dev, against the float64 reference and the derived bound of
tests/tools/tile_ref.py (what the bound can and cannot see: tests/test_cpu_tile_ref.py).

All 30 instantiations launch_dense_layer_big can reach (tile_ref.INSTANTIATIONS, held equal to the dispatch by the CPU test):
  * single layers at every K with 1, 2, 3 or 4 k-tiles, a mid-range K % 64 == 0 and K % 64 == 32, KMAX - 32 and KMAX: `noisy` inputs (large
    magnitudes planted wherever the kernel changes owner) inside the componentwise bound, max |y_dev - y| / E <= 1, `integer` inputs bit
    for bit, everything outside the 32 output channels untouched; B = 3 (W <= 32) or 1, and B = 8 for the XCD remap;
  * the persistent walk (more tiles than workgroups, a tile count that is no multiple of the grid, with and without the XCD remap): a frame's
    bits do not depend on its place in the batch, nor on the launch;
  * chains: `chain_integer` bit for bit over the whole chain; `noisy`: every layer checked from the device's own final buffer (the concat only
    appends, so buf[..., :K0 + 32 l] is exactly what layer l read); the chain's bits equal those of per-layer launches;
  * what the launcher rules out is refused with a message that names the geometry - among it the chains that start at so small a K0 that
    the k-tiles the chained kernel requests ahead for the second layer would reach into the first layer's own, not yet stored output
    (csrc/dense_layer_big.hip::chain_primed_ktiles).

The 1x1 weights carry 64 halves of slack, as the encoder's weight pool gives them: at BK = 64 the last k-tile of a K % 64 == 32 layer is
requested whole (its second half is never multiplied).

Measured worst ratios: docs/numerics.md "The tile kernel, every instantiation"."""
import ctypes as C

import numpy as np
import pytest
import torch

from tools import tile_ref as TR

pytestmark = pytest.mark.gpu

SINGLE = [r for r in TR.INSTANTIATIONS if not r["chained"]]
CHAINED = [r for r in TR.INSTANTIATIONS if r["chained"]]
PERSISTENT = [r for r in SINGLE if r["targs"][4] in (0, 2)]
SINGLE_CASES = [pytest.param(r, k, 3 if r["h"] <= 32 else 1, id="%s-K%d" % (r["id"], k)) for r in SINGLE for k in r["ks"]] + \
               [pytest.param(r, 96, 8, id="%s-K96-B8" % r["id"]) for r in SINGLE]
CHAIN_CASES = [pytest.param(r, k0, n, b, id="%s-K%d-n%d-B%d" % (r["id"], k0, n, b)) for r in CHAINED for k0, n in r["ks"] for b in (3, 8)]


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _pack(ctx, p, h):
    """one layer's parameters -> its device operands (lo, hi, w1, s2, t2, w3p) in the forms the kernel reads"""
    k = p["w1"].shape[1]
    exact = TR.is_exact(p)
    if exact:
        kp = TR.kp_of(h, k)
        w1 = np.zeros((128, 2 * kp), np.float16)
        w1[:, :k] = p["w1"]
        w1[:, kp:kp + k] = p["w1_lo"]
    else:
        w1 = p["w1"].astype(np.float16)
    w1 = np.concatenate([w1.ravel(), np.zeros(64, np.float16)])
    imgs = []
    for part in ([p["w3"], p["w3_lo"]] if exact else [p["w3"]]):
        wp = np.empty(2 * 72 * 64 * 8, np.uint16)           # both MFMA operand layouts
        ctx.lib.tn_dbg_pack_conv3x3(_vp(np.ascontiguousarray(part, np.float32)), _vp(wp))
        imgs.append(wp)
    return dict(lo=_dev(p["lo"], np.float32), hi=_dev(p["hi"], np.float32), w1=torch.from_numpy(w1).cuda(), s2=_dev(p["s2"], np.float32),
                t2=_dev(p["t2"], np.float32), wp=torch.from_numpy(np.concatenate(imgs).view(np.int16)).cuda())


def _rc_layer(ctx, o, buf_d, ldc, k, b, h, variant, exact):
    from tennis_amd import _lib
    rc = ctx.lib.tn_dbg_dense_layer_dev(ctx.handle, _lib.ptr(buf_d), ldc, k, _lib.ptr(o["lo"]), _lib.ptr(o["hi"]), _lib.ptr(o["w1"]), _lib.ptr(o["s2"]),
                                        _lib.ptr(o["t2"]), _lib.ptr(o["wp"]), b, h, h, None, variant | (TR.EXACT if exact else 0))
    return rc


def _launch(ctx, o, buf_d, ldc, k, b, h, variant, exact):
    from tennis_amd import _lib
    _lib.check(_rc_layer(ctx, o, buf_d, ldc, k, b, h, variant, exact), "dense_layer")
    torch.cuda.synchronize()


def _rc_chain(ctx, ops, buf_d, ldc, k0, b, h, variant, exact):
    from tennis_amd import _lib
    n = len(ops)
    arr = {name: (C.c_void_p * n)(*[_lib.ptr(o[name]) for o in ops]) for name in ("lo", "hi", "w1", "s2", "t2", "wp")}
    return ctx.lib.tn_dbg_dense_chain_dev(ctx.handle, _lib.ptr(buf_d), ldc, k0, n, arr["lo"], arr["hi"], arr["w1"], arr["s2"], arr["t2"], arr["wp"], b, h, h,
                                          variant | (TR.EXACT if exact else 0))


def _untouched(buf, out, k, nout=32):
    keep = np.ones(buf.shape[-1], bool)
    keep[k:k + nout] = False
    return np.array_equal(out[..., keep].view(np.uint16), buf[..., keep].view(np.uint16))


def _run(ctx, inp, ldc, variant):
    """one launch on a fresh buffer -> (the buffer as it went in, as it came out), numpy fp16"""
    b, h, _, k = inp["x"].shape
    buf = TR.buffer(inp["x"], ldc)
    d = torch.from_numpy(buf).cuda()
    _launch(ctx, _pack(ctx, inp, h), d, ldc, k, b, h, variant, TR.is_exact(inp))
    return buf, d.cpu().numpy()


def _same_bits(got, want, what):
    same = got.view(np.uint16) == want.view(np.uint16)
    if not same.all():
        bad = np.argwhere(~same)
        print("%s: %d of %d outputs differ; first (frame, row, column, channel): %s" % (what, len(bad), same.size, bad[:8].tolist()))
        for i in bad[:8]:
            print("  %s: device %g, exact %g" % (tuple(i), float(got[tuple(i)]), float(want[tuple(i)])))
    return bool(same.all())


@pytest.mark.parametrize("inst,k,b", SINGLE_CASES)
def test_every_single_layer_instantiation_against_float64(ctx, report, inst, k, b):
    """`noisy` inputs; the smallest legal row pitch (K + 32) for odd K / 32 and one line more otherwise."""
    h = inst["h"]
    inp = TR.noisy(h, k, b, 0, inst["exact"])
    y, bound = TR.reference(inp)
    buf, out = _run(ctx, inp, TR.case_ldc(k), inst["variant"])
    got = out[..., k:k + 32].astype(np.float64)
    q = np.abs(got - y) / bound
    r = float(q.max())
    report["dense_tile_f64_ratio_%s_K%d_B%d" % (inst["id"], k, b)] = r
    report["dense_tile_f64_ratio_%s" % inst["id"]] = max(r, report.get("dense_tile_f64_ratio_%s" % inst["id"], 0.0))
    print("dense_layer_kernel<%s> K = %d, B = %d: max |err| / E = %.3f at %s, max |err| = %.3g, |y| max %.3g" % (
        ", ".join(str(v).lower() for v in inst["targs"]), k, b, r, np.unravel_index(q.argmax(), q.shape), np.abs(got - y).max(), np.abs(y).max()))
    assert np.isfinite(got).all()
    assert r <= 1.0, (r, np.argwhere(q > 1.0)[:8].tolist())
    assert _untouched(buf, out, k)


@pytest.mark.parametrize("inst,k,b", SINGLE_CASES)
def test_every_single_layer_instantiation_integer_exact(ctx, inst, k, b):
    """`integer` inputs: every product, sum and rounding is exact, so the device's halves are the integers' halves."""
    h = inst["h"]
    inp = TR.integer(h, k, b, 0, inst["exact"])
    y, _ = TR.reference(inp)
    buf, out = _run(ctx, inp, TR.case_ldc(k), inst["variant"])
    assert _same_bits(out[..., k:k + 32], y.astype(np.float16), "%s K = %d" % (inst["id"], k))
    assert _untouched(buf, out, k)


def _persistent_batch(h, remap):
    """B with more tiles than workgroups and a tile count that is no multiple of the grid (launch_geom: one workgroup per CU, rounded down
    to 8): 33 / 40 at 56 x 56 on 256 CUs, 17 / 24 at 64 x 64, 65 / 72 at 32 x 32, 129 / 136 at 28 x 28, 257 / 264 for whole-frame tiles"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    tpi = h // TR.rout(h)
    b = ncu // tpi + 1
    if remap:
        b = (b + 7) // 8 * 8
    while (b % 8 == 0) != remap or (b * tpi) % ncu == 0:
        b += 8 if remap else 1
    assert b * tpi > ncu
    return b


@pytest.mark.parametrize("kind", ["noisy", "integer"])
@pytest.mark.parametrize("remap", [False, True], ids=["Bodd", "Bx8"])
@pytest.mark.parametrize("tiles", [1, 4], ids=["1tile", "4tiles"])
@pytest.mark.parametrize("inst", PERSISTENT, ids=[r["id"] for r in PERSISTENT])
def test_persistent_walk_and_batch_position(ctx, inst, tiles, remap, kind):
    """More tiles than workgroups: every workgroup walks on to a next tile whose first k-tiles it requested while the last one drained
    (one k-tile: the `nk > 1` priming of the NEXT tile; four: the steady state).  The same frame first, in the middle and last in the batch
    gives the same bits, the bits of a launch of that frame alone, and a second launch reproduces the first."""
    h, exact, variant = inst["h"], inst["exact"], inst["variant"]
    k = tiles * TR.bk_of(h) if tiles > 1 else 32
    b = _persistent_batch(h, remap)
    ldc = TR.case_ldc(k)
    inp = (TR.noisy if kind == "noisy" else TR.integer)(h, k, 1, 1, exact)
    ops = _pack(ctx, inp, h)
    frame = torch.from_numpy(TR.buffer(inp["x"], ldc)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(h * 1000 + k)
    batch = (torch.randn((b, h, h, ldc), generator=g, device="cuda", dtype=torch.float32) * 1.5).to(torch.float16)
    places = (0, b // 2, b - 1)
    for i in places:
        batch[i] = frame[0]
    first, second, alone = batch.clone(), batch.clone(), frame.clone()
    _launch(ctx, ops, first, ldc, k, b, h, variant, exact)
    _launch(ctx, ops, second, ldc, k, b, h, variant, exact)
    _launch(ctx, ops, alone, ldc, k, 1, h, variant, exact)
    bits = lambda t: t.view(torch.int16)
    for i in places:
        assert torch.equal(bits(first[i]), bits(alone[0])), i
    assert torch.equal(bits(first), bits(second))
    keep = torch.ones(ldc, dtype=torch.bool, device="cuda")
    keep[k:k + 32] = False
    assert torch.equal(bits(first[..., keep]), bits(batch[..., keep]))
    # and the frame is the right one, not merely the same one three times
    y, bound = TR.reference(inp)
    got = alone[:, :, :, k:k + 32].cpu().numpy()
    if kind == "noisy":
        assert TR.ratio(got, y, bound) <= 1.0
    else:
        assert _same_bits(got, y.astype(np.float16), inst["id"])
    # every workgroup stored its tiles: (nearly) no output half is the random number that was there before
    written = (bits(first[..., k:k + 32]) != bits(batch[..., k:k + 32])).float().mean(dim=(1, 2, 3))
    assert torch.isfinite(first[..., k:k + 32].float()).all() and float(written.min()) > 0.99, float(written.min())


def _single_variant(variant):
    """the single-layer launch a chained one is compared with: the same K-loop flavour (the 8 x 1 wave split of bit 5 exists per layer as
    bit 9; the 4 x 2 split with the flat loop only chained - the order of the sum over k does not depend on the wave split)"""
    return 512 if variant & 32 else variant


@pytest.mark.parametrize("inst,k0,n,b", CHAIN_CASES)
def test_every_chained_instantiation_integer_exact(ctx, inst, k0, n, b):
    """`chain_integer` inputs: the whole chain bit for bit."""
    from tennis_amd import _lib
    h, exact = inst["h"], inst["exact"]
    ldc = TR.smallest_ldc(k0 + 32 * (n - 1)) + (64 if b == 8 else 0)
    x, layers = TR.chain_integer(h, k0, n, b, 0, exact)
    want = TR.chain_reference(x, layers).astype(np.float16)
    buf = TR.buffer(x, ldc, 32 * n)
    d = torch.from_numpy(buf).cuda()
    _lib.check(_rc_chain(ctx, [_pack(ctx, p, h) for p in layers], d, ldc, k0, b, h, inst["variant"], exact), "dense_chain")
    out = d.cpu().numpy()
    assert _same_bits(out[..., k0:k0 + 32 * n], want[..., k0:], "%s K0 = %d, n = %d" % (inst["id"], k0, n))
    assert _untouched(buf, out, k0, 32 * n)


@pytest.mark.parametrize("inst,k0,n,b", CHAIN_CASES)
def test_every_chained_instantiation_against_float64_and_per_layer_launches(ctx, report, inst, k0, n, b):
    """`noisy` inputs.  Every layer l against float64 from the device's own final buffer - input buf[..., :K0 + 32 l], output the next 32
    channels - so the divergence of a float64 chain never enters; and the chain's bits against n per-layer launches on a copy."""
    from tennis_amd import _lib
    h, exact = inst["h"], inst["exact"]
    ldc = TR.smallest_ldc(k0 + 32 * (n - 1)) + (64 if b == 8 else 0)
    x, layers = TR.chain_noisy(h, k0, n, b, 0, exact)
    ops = [_pack(ctx, p, h) for p in layers]
    buf = TR.buffer(x, ldc, 32 * n)
    d = torch.from_numpy(buf).cuda()
    per_layer = d.clone()
    _lib.check(_rc_chain(ctx, ops, d, ldc, k0, b, h, inst["variant"], exact), "dense_chain")
    for l in range(n):
        _launch(ctx, ops[l], per_layer, ldc, k0 + 32 * l, b, h, _single_variant(inst["variant"]), exact)
    out = d.cpu().numpy()
    assert np.isfinite(out[..., :k0 + 32 * n].astype(np.float32)).all()
    assert _untouched(buf, out, k0, 32 * n)
    assert np.array_equal(out.view(np.uint16), per_layer.cpu().numpy().view(np.uint16))
    worst = 0.0
    for l, p in enumerate(layers):
        k = k0 + 32 * l
        y, bound = TR.reference(dict(x=out[..., :k], **p))
        q = np.abs(out[..., k:k + 32].astype(np.float64) - y) / bound
        worst = max(worst, float(q.max()))
        assert q.max() <= 1.0, (l, k, float(q.max()), np.argwhere(q > 1.0)[:8].tolist())
    report["dense_tile_f64_ratio_%s_K%d_n%d_B%d" % (inst["id"], k0, n, b)] = worst
    report["dense_tile_f64_ratio_%s" % inst["id"]] = max(worst, report.get("dense_tile_f64_ratio_%s" % inst["id"], 0.0))
    print("dense_layer_kernel<%s> K0 = %d, n = %d, B = %d: worst layer max |err| / E = %.3f" % (", ".join(str(v).lower() for v in inst["targs"]), k0, n, b, worst))


@pytest.mark.parametrize("inst", CHAINED, ids=[r["id"] for r in CHAINED])
def test_chain_of_one_layer_at_the_smallest_k(ctx, inst):
    """nchain = 1 requests nothing ahead: accepted from K = 32, and the bits of the single-layer launch."""
    from tennis_amd import _lib
    h, exact = inst["h"], inst["exact"]
    inp = TR.integer(h, 32, 3, 4, exact)
    y, _ = TR.reference(inp)
    o = _pack(ctx, inp, h)
    d = torch.from_numpy(TR.buffer(inp["x"], 64)).cuda()
    _lib.check(_rc_chain(ctx, [o], d, 64, 32, 3, h, inst["variant"], exact), "dense_chain")
    assert _same_bits(d.cpu().numpy()[..., 32:64], y.astype(np.float16), inst["id"])


NO_LAYER_ARRAY = 1 << 19
REFUSED_LAYERS = [  # (H, K, ldc, variant, exact, what the message has to name)
    (20, 64, 128, 0, False, ("unsupported spatial size", "20 x 20")),
    (128, 64, 128, 0, False, ("unsupported spatial size", "128 x 128")),
    (14, 80, 128, 0, False, ("multiple of 32", "14 x 14", "K = 80")),
    (28, 128, 128, 0, False, ("28 x 28", "K = 128", "ldc = 128")),          # ldc < K + 32
    (56, 96, 132, 0, True, ("56 x 56", "K = 96", "ldc = 132")),             # ldc % 8 != 0
    (56, 288, 320, 0, False, ("56 x 56", "K = 288", "256")),                # past KMAX
    (28, 544, 576, 8, False, ("28 x 28", "K = 544", "512")),
    (7, 1056, 1088, 0, True, ("7 x 7", "K = 1056", "1024")),
]
REFUSED_CHAINS = [  # (H, K0, nchain, ldc, variant, exact, what the message has to name)
    (56, 64, 2, 256, 0, False, ("whole-frame tiles", "56 x 56", "nchain = 2")),
    (28, 128, 2, 512, 0, True, ("whole-frame tiles", "28 x 28", "nchain = 2")),
    (32, 128, 3, 512, 0, False, ("whole-frame tiles", "32 x 32", "nchain = 3")),
    (14, 256, 3, 320, 0, False, ("14 x 14", "K = 256", "ldc = 320", "nchain = 3")),      # ldc < klast + 32
    (14, 992, 3, 1088, 0, False, ("14 x 14", "K = 992", "nchain = 3", "1024")),          # the last layer past KMAX
    (14, 256, 2, 512, NO_LAYER_ARRAY, False, ("without the chain's layer array", "14 x 14", "nchain = 2")),
    (7, 512, 1, 1024, NO_LAYER_ARRAY, True, ("without the chain's layer array", "7 x 7", "nchain = 1")),
    # the k-tiles the chained kernel requests ahead for the second layer would reach into the first layer's own output
    (14, 96, 2, 256, 0, False, ("starts at K >= 128", "2 k-tiles of 64", "14 x 14", "K = 96")),
    (14, 32, 2, 128, 0, False, ("starts at K >= 128", "14 x 14", "K = 32")),
    (16, 32, 2, 128, 0, False, ("starts at K >= 64", "2 k-tiles of 32", "16 x 16", "K = 32")),
    (7, 160, 2, 256, 0, False, ("starts at K >= 192", "3 k-tiles of 64", "7 x 7", "K = 160")),
    (7, 96, 2, 256, 512, False, ("starts at K >= 128", "2 k-tiles of 64", "7 x 7", "K = 96")),
    (7, 64, 3, 256, 32, False, ("starts at K >= 128", "7 x 7", "K = 64")),
    (14, 96, 2, 256, 0, True, ("starts at K >= 128", "14 x 14", "K = 96", "exact")),
    (16, 32, 2, 128, 0, True, ("starts at K >= 64", "16 x 16", "K = 32", "exact")),
    (7, 96, 4, 256, 0, True, ("starts at K >= 128", "7 x 7", "K = 96", "exact")),
]


def test_unsupported_geometries_are_refused(ctx):
    from tennis_amd import _lib
    dummy = torch.zeros(1 << 18, dtype=torch.float16, device="cuda")
    f32 = torch.zeros(2048, dtype=torch.float32, device="cuda")
    o = dict(lo=f32, hi=f32, w1=dummy, s2=f32, t2=f32, wp=dummy)
    for h, k, ldc, variant, exact, names in REFUSED_LAYERS:
        rc = _rc_layer(ctx, o, dummy, ldc, k, 1, h, variant, exact)
        assert rc != 0, (h, k, ldc)
        with pytest.raises(RuntimeError) as ei:
            _lib.check(rc, "dense_layer")
        msg = str(ei.value)
        assert "dense_layer" in msg and all(n in msg for n in names), (h, k, ldc, msg)
    for h, k0, n, ldc, variant, exact, names in REFUSED_CHAINS:
        rc = _rc_chain(ctx, [o] * n, dummy, ldc, k0, 1, h, variant, exact)
        assert rc != 0, (h, k0, n, ldc)
        with pytest.raises(RuntimeError) as ei:
            _lib.check(rc, "dense_chain")
        msg = str(ei.value)
        assert "dense_layer" in msg and all(n_ in msg for n_ in names), (h, k0, n, ldc, msg)
    torch.cuda.synchronize()
    assert not dummy.any()                                     # nothing was launched
    # the boundary is where tile_ref.chain_min_k0 says it is: one step below the smallest K0 is refused for every chained instantiation
    for r in CHAINED:
        k0 = TR.chain_min_k0(r["h"], r["variant"], r["exact"]) - 32
        if k0 >= 32:
            assert _rc_chain(ctx, [o] * 2, dummy, k0 + 64, k0, 1, r["h"], r["variant"], r["exact"]) != 0, r["id"]
    # a good call afterwards still works
    inp = TR.integer(14, 64, 1, 2)
    y, _ = TR.reference(inp)
    _, out = _run(ctx, inp, TR.case_ldc(64), 0)
    assert np.array_equal(out[..., 64:96].view(np.uint16), y.astype(np.float16).view(np.uint16))
