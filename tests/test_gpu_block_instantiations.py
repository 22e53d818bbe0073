"""-m gpu: the three whole-block dense kernels (csrc/dense_block7.hip, dense_block14.hip, dense_block28.hip) through
tn_dbg_block{7,14,28}_create / _run / _destroy against the float64 reference and the derived bound of tests/tools/block_ref.py (what
the bound can and cannot see, and why the shape lists cover every loop variant: tests/test_cpu_block_ref.py).

  * every shape of block_ref.SHAPES - every K0 the kernel accepts as a FIRST layer behind the prologue, the network's own blocks, every K in
    one launch - on `noisy` inputs (large magnitudes planted wherever a wave, a pass, a pixel tile or a ring slot changes owner), every
    layer judged from the device's own final buffer, max |y_dev - y| / E <= 1; on `chain_integer` inputs the integers bit for bit;
    everything outside the produced channels untouched; a second run on a fresh copy gives the same bits;
  * place in the batch: more workgroups than CUs and no multiple of the CU count - a frame's bits do not depend on its place and equal
    those of a launch of that frame alone;
  * dirty scratch: after a launch over Inf, NaN and 6e4 the same handle gives, on ordinary inputs, the bits of a fresh handle - at a first
    layer whose last super-step is half empty and at one where it is full (14 x 14, 28 x 28), and at 7 x 7, which has no scratch, as a control;
  * what the launchers rule out is refused with a message that names the geometry, and nothing is launched.  (A handle of one streamed
    kernel cannot reach the other's launcher: the handle carries its kernel, dbg.hip::dbg_stream_run - not tested.)

The row pitch is the smallest legal one in half of the cases and 64 more in the others (block_ref.case_ldc); at the smallest pitch the last
frame's last pixel ends the allocation (docs/numerics.md has the reading of every address the kernels form there).

Measured worst ratios: docs/numerics.md "The whole-block kernels, every loop variant"."""
import ctypes as C

import numpy as np
import pytest
import torch

from tools import block_ref as BR

pytestmark = pytest.mark.gpu

CASES = [pytest.param(h, k0, nl, id="%d-K%d-nl%d" % (h, k0, nl)) for h in BR.SIZES for k0, nl, _ in BR.SHAPES[h]]
SHORT = {7: (448, 2), 14: (256, 2), 28: (128, 2)}


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _fn(ctx, h, what):
    return getattr(ctx.lib, "tn_dbg_block%d_%s" % (h, what))


def _rc_create(ctx, h, k0, nl, layers, handle):
    cat = lambda name: np.ascontiguousarray(np.concatenate([np.asarray(p[name], np.float32).ravel() for p in layers])) if layers else np.zeros(1, np.float32)
    ops = [cat(n) for n in ("w1", "lo", "hi", "s2", "t2", "w3")]
    return _fn(ctx, h, "create")(ctx.handle, k0, nl, *[_vp(o) for o in ops], C.byref(handle))


class Block:
    """a tn_dbg_block* handle, destroyed on exit"""

    def __init__(self, ctx, h, k0, layers):
        from tennis_amd import _lib
        self.ctx, self.h, self.handle = ctx, h, C.c_void_p()
        _lib.check(_rc_create(ctx, h, k0, len(layers), layers, self.handle), "block%d_create" % h)

    def rc(self, d, ldc, b):
        from tennis_amd import _lib
        return _fn(self.ctx, self.h, "run")(self.handle, _lib.ptr(d), ldc, b)

    def run(self, d, ldc, b):
        from tennis_amd import _lib
        _lib.check(self.rc(d, ldc, b), "block%d_run" % self.h)
        torch.cuda.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _fn(self.ctx, self.h, "destroy")(self.handle)


def _bits(a):
    return a.view(np.uint16) if isinstance(a, np.ndarray) else a.view(torch.int16)


def _untouched(buf, out, k0, nout):
    keep = np.ones(buf.shape[-1], bool)
    keep[k0:k0 + nout] = False
    return np.array_equal(_bits(out[..., keep]), _bits(buf[..., keep]))


def _same_bits(got, want, what):
    same = _bits(got) == _bits(want)
    if not same.all():
        bad = np.argwhere(~same)
        print("%s: %d of %d outputs differ; first (frame, row, column, channel): %s" % (what, len(bad), same.size, bad[:8].tolist()))
        for i in bad[:8]:
            print("  %s: device %g, exact %g" % (tuple(i), float(got[tuple(i)]), float(want[tuple(i)])))
    return bool(same.all())


def _run_twice(ctx, h, k0, x, layers):
    """-> (the buffer as it went in, as it came out): one handle, two launches on fresh copies, which have to agree bit for bit"""
    nl, b = len(layers), x.shape[0]
    ldc = BR.case_ldc(h, k0, nl)
    buf = BR.buffer(x, ldc, 32 * nl)
    with Block(ctx, h, k0, layers) as blk:
        d, d2 = torch.from_numpy(buf).cuda(), torch.from_numpy(buf).cuda()
        blk.run(d, ldc, b)
        blk.run(d2, ldc, b)
    assert torch.equal(_bits(d), _bits(d2)), "a second run on a fresh copy differs"
    return buf, d.cpu().numpy()


@pytest.mark.parametrize("h,k0,nl", CASES)
def test_every_block_shape_against_float64(ctx, report, h, k0, nl):
    x, layers = BR.noisy(h, k0, nl, BR.BATCH[h], 0)
    buf, out = _run_twice(ctx, h, k0, x, layers)
    assert np.isfinite(out[..., :k0 + 32 * nl].astype(np.float32)).all()
    rs = BR.block_ratios(out, k0, layers, h)
    print("dense_block%d K0 = %d, nl = %d: max |err| / E per layer: %s" % (h, k0, nl, " ".join("%.3f" % r for r in rs)))
    report["dense_block%d_f64_ratio_K%d_nl%d" % (h, k0, nl)] = max(rs)
    assert max(rs) <= 1.0, [(l, r) for l, r in enumerate(rs) if r > 1.0]
    assert _untouched(buf, out, k0, 32 * nl)


@pytest.mark.parametrize("h,k0,nl", CASES)
def test_every_block_shape_integer_exact(ctx, h, k0, nl):
    x, layers = BR.integer_block(h, k0, nl, BR.BATCH[h], 0)
    want = BR.chain_reference(x, layers, h)
    a1 = np.clip(want[..., k0:], 0.0, 1.0)                              # no produced channel is a dead input of the layers behind it
    assert np.all(a1.min(axis=(0, 1, 2)) == 0) and np.all(a1.max(axis=(0, 1, 2)) == 1) and np.abs(want).max() < 2048
    buf, out = _run_twice(ctx, h, k0, x, layers)
    assert _same_bits(out[..., k0:k0 + 32 * nl], want[..., k0:].astype(np.float16), "dense_block%d K0 = %d, nl = %d" % (h, k0, nl))
    assert _untouched(buf, out, k0, 32 * nl)


@pytest.mark.parametrize("kind", ["noisy", "integer"])
@pytest.mark.parametrize("h", BR.SIZES)
def test_place_in_the_batch(ctx, h, kind):
    """One workgroup per frame: B = the CU count + 3 is more workgroups than CUs and no multiple of it.  The same frame first, in the
    middle and last gives the same bits, the bits of a launch of that frame alone, and the right ones."""
    k0, nl = SHORT[h]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    b = ncu + 3
    assert b > ncu and b % ncu
    ldc = BR.smallest_ldc(h, k0, nl)
    x, layers = (BR.noisy if kind == "noisy" else BR.integer_block)(h, k0, nl, 1, 1)
    frame = torch.from_numpy(BR.buffer(x, ldc, 32 * nl)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(h * 1000 + k0)
    batch = (torch.randn((b, h, h, ldc), generator=g, device="cuda", dtype=torch.float32) * 1.5).to(torch.float16)
    places = (0, b // 2, b - 1)
    for i in places:
        batch[i] = frame[0]
    first, second, alone = batch.clone(), batch.clone(), frame.clone()
    with Block(ctx, h, k0, layers) as blk:
        blk.run(first, ldc, b)
        blk.run(second, ldc, b)
    with Block(ctx, h, k0, layers) as blk:
        blk.run(alone, ldc, 1)
    for i in places:
        assert torch.equal(_bits(first[i]), _bits(alone[0])), i
    assert torch.equal(_bits(first), _bits(second))
    keep = torch.ones(ldc, dtype=torch.bool, device="cuda")
    keep[k0:k0 + 32 * nl] = False
    assert torch.equal(_bits(first[..., keep]), _bits(batch[..., keep]))
    out = alone.cpu().numpy()
    if kind == "noisy":
        assert max(BR.block_ratios(out, k0, layers, h)) <= 1.0
    else:
        assert _same_bits(out[..., k0:k0 + 32 * nl], BR.chain_reference(x, layers, h)[..., k0:].astype(np.float16), "dense_block%d alone" % h)
    # every workgroup stored its frame: (nearly) no produced half is the random number that was there before
    prod = slice(k0, k0 + 32 * nl)
    written = (_bits(first[..., prod]) != _bits(batch[..., prod])).float().mean(dim=(1, 2, 3))
    assert torch.isfinite(first[..., prod].float()).all() and float(written.min()) > 0.99, float(written.min())


# (h, K0): at 14 x 14 the first layer reads K0 - 32 channels from memory - half-empty last super-step at K0 = 256, full at 288; at 28 x 28
# it reads K0 - half-empty at 160, whose pad half is the planes of channels 160 ... 191, which only a previous launch can have written
DIRTY = [(14, 256), (14, 288), (28, 160), (28, 128), (7, 448)]


@pytest.mark.parametrize("h,k0", DIRTY, ids=["%d-K%d" % c for c in DIRTY])
def test_a_dirty_scratch_does_not_reach_the_next_launch(ctx, h, k0):
    """The streamed kernels' scratch is zeroed once and then reused (dbg.hip::dbg_stream_run, encoder.hip).  The first launch of a handle
    computes with large finite values, +-Inf and NaN - data, not a fault - and leaves what came of them in the scratch planes of the
    channels it produced; the pad half of a half-empty last super-step, and at 28 x 28 the lanes of rows 28 ... 31, read such planes against
    zero weights and zero clamp constants, or behind the mask of the shift k-step.  The second launch, on ordinary inputs, has to give the
    bits of a fresh handle."""
    nl, b = 2, BR.BATCH[h]
    ldc = BR.case_ldc(h, k0, nl)
    x, layers = BR.noisy(h, k0, nl, b, 2)
    buf = BR.buffer(x, ldc, 32 * nl)
    with Block(ctx, h, k0, layers) as blk:
        d0 = torch.from_numpy(BR.buffer(BR.dirty(h, k0, b, 0), ldc, 32 * nl)).cuda()
        blk.run(d0, ldc, b)
        assert not torch.isfinite(d0[..., k0:k0 + 32 * nl].float()).all()       # the first launch did produce non-finite channels
        used = torch.from_numpy(buf).cuda()
        blk.run(used, ldc, b)
    with Block(ctx, h, k0, layers) as blk:
        fresh = torch.from_numpy(buf).cuda()
        blk.run(fresh, ldc, b)
    out = used.cpu().numpy()
    assert _same_bits(out, fresh.cpu().numpy(), "dense_block%d K0 = %d behind a dirty launch" % (h, k0))
    assert max(BR.block_ratios(out, k0, layers, h)) <= 1.0 and _untouched(buf, out, k0, 32 * nl)


@pytest.mark.parametrize("h", BR.SIZES)
def test_unsupported_geometries_are_refused(ctx, h):
    from tennis_amd import _lib
    k0, nl = SHORT[h]
    x, layers = BR.integer_block(h, k0, nl, 1, 3)
    dummy = torch.zeros(1 << 20, dtype=torch.float16, device="cuda")
    rows = BR.refusals(h)
    with Block(ctx, h, k0, layers) as good:
        for rk0, rnl, ldc, b, names in rows:
            if not BR.supported(h, rk0, rnl):                     # the kernel's predicate: refused before anything is packed
                handle = C.c_void_p()
                rc, what = _rc_create(ctx, h, rk0, rnl, [], handle), "block%d_create" % h
                assert not handle.value
            else:                                                 # the launcher's checks: the pitch and the batch
                assert (rk0, rnl) == (k0, nl)
                rc, what = good.rc(dummy, ldc, b), "block%d_run" % h
            assert rc != 0, (rk0, rnl, ldc, b)
            with pytest.raises(RuntimeError) as ei:
                _lib.check(rc, what)
            msg = str(ei.value)
            assert "block%d" % h in msg and all(n in msg for n in names), (rk0, rnl, ldc, b, msg)
        torch.cuda.synchronize()
        assert not dummy.any()                                    # nothing was launched
        # a good call afterwards still works
        ldc = BR.smallest_ldc(h, k0, nl)
        d = torch.from_numpy(BR.buffer(x, ldc, 32 * nl)).cuda()
        good.run(d, ldc, 1)
    want = BR.chain_reference(x, layers, h)[..., k0:].astype(np.float16)
    assert _same_bits(d.cpu().numpy()[..., k0:k0 + 32 * nl], want, "dense_block%d after the refusals" % h)
