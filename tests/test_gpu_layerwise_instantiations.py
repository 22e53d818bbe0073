"""-m gpu: every instantiation of the transition and layer-wise kernels - conv1x1_kernel<MI, POOL, NB, EX, ONCE> (csrc/conv1x1.hip),
trans_ws_kernel<NK, BM, NB> (csrc/trans_ws.hip), conv3x3_kernel<V, EX> (csrc/conv3x3.hip) - on its own, through tn_dbg_conv1x1_ex and
tn_dbg_conv3x3_dev, against the float64 reference and the derived bound of tests/tools/layerwise_ref.py (what the bound can and cannot
see: tests/test_cpu_layerwise_ref.py).

Every case (layerwise_ref.CASES; the CPU test holds each to the instantiation it names) runs once, with the fp32 side output y32 where
the kernel has one, on buffers with a row pitch beyond the channels used: 300.0 behind K in x, around the output columns of y (written
at column 40) and behind N in y32, a stale value inside.  Asserted: finite outputs; max |y_dev - y| / E16 <= 1 and max |y32_dev - y| /
E32 <= 1 (which a stale value left in place cannot meet); the sentinels untouched; on `integer` inputs y32 bit for bit the float64 value
and y its round-to-nearest-even half.

The two non-temporal instantiations are reached with TN_TRANS_NT_MB=0, which a process reads once: one child process runs their cases
and writes .npy files, the parent holds them to the reference and to the bits of its own default-path launch on the same operands (the
loads differ in their cache hint only).  The warp-specialised kernel gets its weight fragments from the HOST packer, as
tn_densenet121_create does; the device packer's image is held bit-equal to it.

Measured worst ratios: docs/numerics.md "The transition and layer-wise kernels, every instantiation"."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tools import layerwise_ref as LR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def host_frags(lib, w16):
    """[N][K] fp16 -> the fragment image of the host packer (tn_dbg_pack_trans_frags -> pack_trans_frags)"""
    n, k = w16.shape
    w16 = np.ascontiguousarray(w16)
    out = np.empty(n * k, np.float16)
    assert lib.tn_dbg_pack_trans_frags(_vp(w16), n, k, _vp(out)) == 0
    return out


def run_case(ctx, c, inp):
    """one launch of the case on fresh buffers -> (y (M, ldy) fp16, y32 (M, ld32) fp32 | None), numpy"""
    from tennis_amd import _lib
    lib = ctx.lib
    ybuf, y32buf = LR.y_buffers(c)
    yd = torch.from_numpy(ybuf).cuda()
    s, t = _dev(inp["s"]), _dev(inp["t"])
    flags = c["variant"] | (LR.EXACT if c["exact"] else 0)
    if c["op"] == "c3":
        imgs = []
        for part in [inp["w"]] + ([inp["w_lo"]] if c["exact"] else []):
            wp = np.empty(2 * 72 * 64 * 8, np.uint16)           # both MFMA operand layouts
            assert lib.tn_dbg_pack_conv3x3(_vp(np.ascontiguousarray(part, np.float32)), _vp(wp)) == 0
            imgs.append(wp)
        wd = torch.from_numpy(np.concatenate(imgs).view(np.int16)).cuda()
        xd = torch.from_numpy(np.ascontiguousarray(inp["x"])).cuda()
        rc = lib.tn_dbg_conv3x3_dev(ctx.handle, _lib.ptr(xd), _lib.ptr(s), _lib.ptr(t), _lib.ptr(wd), _lib.ptr(yd), ybuf.shape[1], LR.YOFF, c["B"], c["H"],
                                    c["W"], flags)
        _lib.check(rc, "tn_dbg_conv3x3_dev")
        torch.cuda.synchronize()
        return yd.cpu().numpy(), None
    xd = torch.from_numpy(LR.x_buffer(c, inp)).cuda()
    w16 = LR.weight_rows(inp)
    wd = torch.from_numpy(w16).cuda()
    y32d = torch.from_numpy(y32buf).cuda()
    bias = _dev(inp["bias"]) if c["bias"] else None
    frag = torch.from_numpy(host_frags(lib, w16)).cuda() if c["op"] == "ws" else None
    rc = lib.tn_dbg_conv1x1_ex(ctx.handle, _lib.ptr(xd), LR.ldx_of(c), c["K"], _lib.ptr(s), _lib.ptr(t), _lib.ptr(wd), c["N"], _lib.ptr(yd), ybuf.shape[1],
                               LR.YOFF, c["M"], int(c["op"] != "c1"), c["H"], c["W"], flags, _lib.ptr(bias), int(c["clamp"]), _lib.ptr(y32d), y32buf.shape[1],
                               _lib.ptr(frag))
    _lib.check(rc, "tn_dbg_conv1x1_ex")
    torch.cuda.synchronize()
    return yd.cpu().numpy(), y32d.cpu().numpy()


def _bits_equal(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    same = g.view(np.uint16 if g.dtype == np.float16 else np.uint32) == w.view(np.uint16 if w.dtype == np.float16 else np.uint32)
    if not same.all():
        bad = np.argwhere(~same)
        print("%s: %d of %d outputs differ; first (row, channel): %s" % (what, len(bad), same.size, bad[:8].tolist()))
        for i in bad[:8]:
            print("  %s: device %r, exact %r" % (tuple(i), float(g[tuple(i)]), float(w[tuple(i)])))
    return bool(same.all())


def check_case(c, inp, y_out, y32_out, report=None):
    """the assertions of one case on what the device left in the buffers"""
    n = c["N"]
    y, e16, y32, e32 = (v.reshape(c["M"], n) for v in LR.reference(inp))
    got = y_out[:, LR.YOFF:LR.YOFF + n]
    assert np.isfinite(got.astype(np.float32)).all()
    assert np.all(y_out[:, :LR.YOFF] == LR.SENTINEL) and np.all(y_out[:, LR.YOFF + n:] == LR.SENTINEL)
    q16 = np.abs(got.astype(np.float64) - y) / e16
    r16, r32 = float(q16.max()), None
    if y32_out is not None:
        got32 = y32_out[:, :n]
        assert np.isfinite(got32).all() and np.all(y32_out[:, n:] == LR.SENTINEL)
        q32 = np.abs(got32.astype(np.float64) - y32) / e32
        r32 = float(q32.max())
    print("%s<%s> %s: max |err| / E  y %.3f%s, |y| max %.3g" % (c["inst"][0], ", ".join(str(v).lower() for v in c["inst"][1]), c["id"], r16,
                                                              "" if r32 is None else "  y32 %.3f" % r32, np.abs(y).max()))
    if report is not None:
        report["layerwise_%s_err_over_bound" % c["id"]] = r16
        key = "layerwise_worst_%s<%s>" % (c["inst"][0], ",".join(str(v).lower() for v in c["inst"][1]))
        report[key] = max(r16, report.get(key, 0.0))
        if r32 is not None:
            report["layerwise_%s_y32_err_over_bound" % c["id"]] = r32
            report[key + "_y32"] = max(r32, report.get(key + "_y32", 0.0))
    assert r16 <= 1.0, (r16, np.argwhere(q16 > 1.0)[:8].tolist())
    assert r32 is None or r32 <= 1.0, (r32, np.argwhere(q32 > 1.0)[:8].tolist())
    if c["gen"] == "integer":
        assert _bits_equal(got, y.astype(np.float16), c["id"] + " y")
        if y32_out is not None:
            assert _bits_equal(got32, y32.astype(np.float32), c["id"] + " y32")


@pytest.mark.parametrize("c", LR.CASES, ids=lambda c: c["id"])
def test_every_instantiation_against_float64(ctx, report, c):
    inp = LR.make(c)
    y_out, y32_out = run_case(ctx, c, inp)
    check_case(c, inp, y_out, y32_out, report)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import test_gpu_layerwise_instantiations as T
from tools import layerwise_ref as LR
from tennis_amd import _lib
ctx = _lib.default_context(0)
for c in LR.ONCE_CASES:
    y, y32 = T.run_case(ctx, c, LR.make(c))
    np.save(sys.argv[3] + c["id"] + "-y.npy", y)
    np.save(sys.argv[3] + c["id"] + "-y32.npy", y32)
"""


def test_non_temporal_instantiations_in_a_child_process(ctx, report, tmp_path):
    """conv1x1_kernel<2, true, 256, false, true> and <2, true, 128, false, true>: TN_TRANS_NT_MB=0 makes every single-column-tile
    transition stream its activations."""
    prefix = str(tmp_path) + os.sep
    r = subprocess.run([sys.executable, "-c", _CHILD, HERE, os.path.dirname(HERE), prefix], env=dict(os.environ, TN_TRANS_NT_MB="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for c in LR.ONCE_CASES:
        inp = LR.make(c)
        y_out, y32_out = np.load(prefix + c["id"] + "-y.npy"), np.load(prefix + c["id"] + "-y32.npy")
        check_case(c, inp, y_out, y32_out, report)
        mine, mine32 = run_case(ctx, dict(c, nt_mb=128), inp)        # this process: the default threshold, the plain loads
        assert _bits_equal(y_out, mine, c["id"] + " y against the default path") and _bits_equal(y32_out, mine32, c["id"] + " y32 against the default path")


@pytest.mark.parametrize("n,k", [(512, 1024), (256, 128), (512, 256)])
def test_device_packer_image_is_the_host_packer_image(ctx, n, k):
    """pack_trans_frags_kernel (what the tiled-against-warp-specialised comparison of test_gpu_kernels.py packs with) and pack_trans_frags
    (what create packs with) - every half a different bit pattern"""
    from tennis_amd import _lib
    w = np.arange(n * k, dtype=np.uint16).reshape(n, k).view(np.float16)
    wd = torch.from_numpy(w.view(np.int16)).cuda()
    out = torch.full((n * k,), -1, dtype=torch.int16, device="cuda")
    _lib.check(ctx.lib.tn_dbg_pack_trans_frags_dev(ctx.handle, _lib.ptr(wd), n, k, _lib.ptr(out)), "tn_dbg_pack_trans_frags_dev")
    torch.cuda.synchronize()
    host = host_frags(ctx.lib, w)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), host.view(np.uint16))
    assert np.array_equal(host.view(np.uint16), LR.frag_order(w.view(np.uint16)))


def test_hooks_refuse_bad_arguments(ctx):
    from tennis_amd import _lib
    lib, h = ctx.lib, ctx.handle
    x = torch.zeros(1 << 20, dtype=torch.float16, device="cuda")
    y = torch.full((1 << 20,), LR.SENTINEL, dtype=torch.float16, device="cuda")
    y32 = torch.full((1 << 20,), LR.SENTINEL, dtype=torch.float32, device="cuda")
    f = torch.zeros(4096, dtype=torch.float32, device="cuda")
    px, py, p32, pf = _lib.ptr(x), _lib.ptr(y), _lib.ptr(y32), _lib.ptr(f)

    def c1(ldx=128, K=64, N=128, ldy=256, yoff=8, M=98, pool=0, H=0, W=0, variant=0, bias=None, clamp=0, y32p=None, ld32=0, wfrag=None, xp=px):
        return lib.tn_dbg_conv1x1_ex(h, xp, ldx, K, pf, pf, px, N, py, ldy, yoff, M, pool, H, W, variant, bias, clamp, y32p, ld32, wfrag)

    def refused(rc, word):
        msg = lib.tn_last_error().decode()
        assert rc != 0 and word in msg, (rc, word, msg)

    refused(c1(K=48), "K%32")
    refused(c1(N=64, ldy=128), "N%128")
    refused(c1(ldx=100), "multiples of 8")
    refused(c1(ldy=252), "multiples of 8")
    refused(c1(yoff=4), "multiples of 8")
    refused(c1(K=96, pool=1, H=14, W=14, variant=LR.EXACT), "K % 64")
    refused(c1(K=128, ldx=128, N=512, ldy=1024, M=98, pool=1, H=15, W=15, wfrag=px), "wfrag")                 # odd map
    refused(c1(K=128, ldx=128, N=384, ldy=1024, M=98, pool=1, H=14, W=14, wfrag=px), "wfrag")                 # N = 384
    refused(c1(K=128, ldx=128, N=512, ldy=1024, M=98, pool=1, H=14, W=14, wfrag=px, bias=pf), "wfrag")        # a bias
    refused(c1(K=128, ldx=128, N=512, ldy=1024, M=98, pool=1, H=14, W=14, wfrag=px, variant=LR.EXACT), "wfrag")
    refused(c1(y32p=p32, ld32=120), "ld32")
    refused(c1(y32p=p32, ld32=130), "ld32")
    refused(c1(ldx=32), "bad shape")
    refused(c1(M=97, pool=1, H=14, W=14), "pooling")
    refused(c1(xp=None), "null")
    refused(lib.tn_dbg_conv3x3_dev(h, px, pf, pf, px, py, 96, 40, 1, 2, 241, 0), "W too large")
    refused(lib.tn_dbg_conv3x3_dev(h, px, pf, pf, px, py, 96, 40, 1, 2, 241, LR.EXACT), "W too large")
    refused(lib.tn_dbg_conv3x3_dev(h, px, pf, pf, px, py, 92, 40, 1, 2, 24, 0), "multiples of 8")
    refused(lib.tn_dbg_pack_trans_frags_dev(h, px, 48, 64, py), "N % 32")
    refused(lib.tn_dbg_pack_trans_frags_dev(h, None, 64, 64, py), "null")
    torch.cuda.synchronize()
    assert torch.all(y == LR.SENTINEL) and torch.all(y32 == LR.SENTINEL)             # nothing was launched
    # a good call afterwards still works
    c = next(c for c in LR.CASES if c["id"] == "c1-M1-K64-N128-bias-integer")
    inp = LR.make(c)
    check_case(c, inp, *run_case(ctx, c, inp))
