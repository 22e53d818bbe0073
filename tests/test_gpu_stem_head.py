"""-m gpu: the first and the last kernels of every forward on their own, against float64 (tests/tools/stem_ref.py).

  * csrc/stem_pool.hip, all 12 instantiations (layout x fetch path x weights, each with its border-only conv), and the unfused
    route csrc/stem.hip + maxpool_kernel, through tn_dbg_stem - which folds with the function tn_densenet121_create folds with;
  * maxpool_kernel and head_kernel<false / true> through tn_dbg_maxpool / tn_dbg_head.

Tolerances are derived, not measured (docs/numerics.md "The stem and head kernels on their own"):
  slack = 160 * 2^-24 * A, A = |s| sum |w| |x|: fp32 accumulation of 147 products plus the BatchNorm fma;
  fused:    |got - ref| <= ulp16(|ref|) + slack      (the dithered truncation lands on one of the value's two fp16 neighbours);
  unfused:  |got - ref| <= ulp16(|ref|) / 2 + slack  (round-to-nearest at the conv map, and the max of halves is exact);
  2^-24 stands for the ulp of a subnormal half.  Exact mode: the same against hi + lo weights.
The bitwise check pins the dither itself: wherever moving the reference by +- slack does not change the emulated half, the device half
IS the emulated half (tests/test_cpu_stem_ref.py establishes that this leaves out under 5 % of every case).  Each case records its
worst error as a fraction of its bound in the parity report (stem_<case>_err_over_bound)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tools import stem_ref as SR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHARE_CAP = 0.05
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _fp(a):
    return None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)


def pooled_size(h, w):
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (ho - 1) // 2 + 1, (wo - 1) // 2 + 1


def run_stem(ctx, p, x, layout, exact, fused, ldy=64):
    """-> (B,Hp,Wp,ldy) float16 from tn_dbg_stem, the columns past 64 pre-set to SENTINEL"""
    from tennis_amd import _lib
    if layout == SR.LAYOUT_NCHW_F32:
        b, _, h, w = x.shape
    else:
        b, h, w, _ = x.shape
    hp, wp = pooled_size(h, w)
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((b, hp, wp, ldy), SENTINEL, dtype=torch.float16, device="cuda")
    keep = [np.ascontiguousarray(p[k], np.float32) for k in ("w0", "gamma", "beta", "mean", "var")]
    mc = None if p["m_c"] is None else np.ascontiguousarray(p["m_c"], np.float32)
    _lib.check(ctx.lib.tn_dbg_stem(ctx.handle, *[_fp(a) for a in keep], _fp(mc), int(exact), int(fused), layout, b, h, w, _lib.ptr(xd), _lib.ptr(yd),
                                   ldy), "tn_dbg_stem")
    return yd.cpu().numpy()


def interior(hp, wp, h, w):
    """pooled positions whose 11 x 11 input footprint (rows 4r - 5 .. 4r + 5) lies inside the frame"""
    r = np.arange(hp); c = np.arange(wp)
    return np.ix_((4 * r - 5 >= 0) & (4 * r + 5 <= h - 1), (4 * c - 5 >= 0) & (4 * c + 5 <= w - 1))


@pytest.mark.parametrize("case", SR.STEM_CASES, ids=[c[0] for c in SR.STEM_CASES])
def test_stem_against_float64(ctx, report, case):
    """Frames per case (stem_ref.stem_frames): uniform noise; constant 0 and constant 255 (the padding constant and the shift_u8 bias are
    the whole signal at their border); 128 inside a one-pixel ring; single-pixel impulses at corners, edge midpoints and the centre
    (footprint, kx / ky order).  Parameters: stem_ref.stem_params.  Interior and border outputs hold the same bound."""
    name, h, w, layout, exact, fused = case
    p, x, ref, A, pre = SR.case_reference(case)
    ldy = 64 if "80x80" in name else 256
    y = run_stem(ctx, p, x, layout, exact, fused, ldy)
    assert np.all(y[..., 64:] == SENTINEL)                                  # ldy = 256 is the encoder's stride (block 1's concat buffer)
    got = y[..., :64]
    assert np.all(np.isfinite(got))
    g64 = got.astype(np.float64)
    sl = SR.slack(A)
    bound = SR.ulp16(ref) * (1.0 if fused else 0.5) + sl
    err = np.abs(g64 - ref)
    frac = err / bound
    hp, wp = ref.shape[1:3]
    ii = interior(hp, wp, h, w)
    border = np.ones((hp, wp), bool); border[ii] = False
    print("%s: worst err / bound %.3f (interior %.3f, border %.3f), max err %.3g, subnormal outputs %d" % (
        name, frac.max(), frac[:, ~border].max(), frac[:, border].max(), err.max(), int(((np.abs(ref) < 2.0 ** -14) & (ref != 0)).sum())))
    report[f"stem_{name}_err_over_bound"] = float(frac.max())
    assert np.all(err <= bound), (name, np.argwhere(err > bound)[:8].tolist())
    if not fused:
        return
    # ---- bitwise: the dither key is (pooled row, pooled column, channel) - not the frame, the batch, the tile origin or the grid ----
    emu, ok = SR.decided(pre, A, p["m_c"])
    share = 1.0 - ok.mean()
    mism = ok & (got != emu)               # (compared as numbers: +0 and -0, the floor of an un-centred channel, are the same output)
    print("%s: undecided share %.4f, mismatches among the decided %d" % (name, share, int(mism.sum())))
    report[f"stem_{name}_undecided_share"] = float(share)
    assert share < SHARE_CAP
    assert not mism.any(), (name, int(mism.sum()), np.argwhere(mism)[:8].tolist())
    # ---- flat frames, interior: the mean signed error of a channel within 5 sigma = 5 * 0.5 ulp / sqrt(N) of zero; looser by the
    # case's slack, 160 * 2^-24 * A of the channel (the kernel's fp32 sum may sit that far from the float64 one, at every position alike)
    for f in SR.CONSTANT_FRAMES:
        r, g, s = ref[f][ii], g64[f][ii], sl[f][ii]
        n = r.shape[0] * r.shape[1]
        assert np.all(r == r[0, 0]) and n >= 100, (name, f, n)                        # flat inside: one value per channel
        bias = (g - r).mean(axis=(0, 1))
        lim = 5 * 0.5 * SR.ulp16(r[0, 0]) / np.sqrt(n) + s[0, 0]
        print("%s frame %d: worst channel bias / limit %.3f (N = %d)" % (name, f, (np.abs(bias) / lim).max(), n))
        report[f"stem_{name}_flat{f}_bias_over_limit"] = float((np.abs(bias) / lim).max())
        assert np.all(np.abs(bias) <= lim), (name, f, np.argwhere(np.abs(bias) > lim).ravel().tolist())


@pytest.mark.parametrize("layout,exact", [(SR.LAYOUT_NHWC_U8, False), (SR.LAYOUT_NHWC_F16, True)])
def test_stem_frame_bits_do_not_depend_on_the_batch(ctx, layout, exact):
    """The same frame first and last in batches of 1, 3 and 40: identical bits.  40 frames of 224 x 224 are 2240 tiles, more than
    three workgroups per CU, so the persistent ranges cross frame boundaries and the frame meets other tile positions of a range."""
    p = SR.stem_params("batch_invariance")
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, (1, 224, 224, 3), dtype=np.uint8)
    outs = []
    for b in (1, 3, 40):
        u8 = rng.integers(0, 256, (b, 224, 224, 3), dtype=np.uint8)
        u8[0] = frame[0]; u8[-1] = frame[0]
        y = run_stem(ctx, p, SR.layout_input(u8, layout), layout, exact, True, 64)
        outs += [y[0], y[-1]]
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint16), outs[0].view(np.uint16))


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import test_gpu_stem_head as T
from tools import stem_ref as SR
from tennis_amd import _lib
case = [c for c in SR.STEM_CASES if c[0] == sys.argv[3]][0]
p = SR.stem_params(case[0])
x = SR.layout_input(SR.stem_frames(case[1], case[2]), case[3])
np.save(sys.argv[4], T.run_stem(_lib.default_context(0), p, x, case[3], case[4], case[5], 64))
"""


def test_stem_uneven_persistent_ranges(ctx, tmp_path):
    """TN_STEM_WGS=7 (read once per process: a child): the 375 tiles of 5 frames of 232 x 232 as ranges of 54 and 53.  The bits are
    those of the default grid, which test_stem_against_float64 holds to the reference."""
    name = "fused_f16_rounded_232x232"
    case = [c for c in SR.STEM_CASES if c[0] == name][0]
    out = str(tmp_path / "wgs7.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, HERE, os.path.dirname(HERE), name, out], env=dict(os.environ, TN_STEM_WGS="7"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    p = SR.stem_params(name)
    y = run_stem(ctx, p, SR.layout_input(SR.stem_frames(case[1], case[2]), case[3]), case[3], case[4], case[5], 64)
    assert np.array_equal(np.load(out).view(np.uint16), y.view(np.uint16))


@pytest.mark.parametrize("B,H,W,C,ldy", [(2, 113, 113, 64, 256), (3, 112, 112, 64, 64), (2, 9, 13, 8, 24), (1, 113, 112, 8, 8), (2, 9, 13, 64, 72)])
def test_maxpool_is_the_float64_maxpool(ctx, B, H, W, C, ldy):
    """maxpool_kernel: bit-equal to MaxPool2D(3, 2, pad 1) with -inf padding.  Every input is negative, so a zero in place of the padding
    would win at the border; odd and even H and W (113: the last window reads past the map), ldy > C with a sentinel behind."""
    from tennis_amd import _lib
    rng = np.random.default_rng(B * H + W + C)
    x = (-np.abs(rng.normal(0, 2.0, (B, H, W, C))) - 0.01).astype(np.float16)
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((B, ho, wo, ldy), SENTINEL, dtype=torch.float16, device="cuda")
    _lib.check(ctx.lib.tn_dbg_maxpool(ctx.handle, _lib.ptr(xd), B, H, W, C, _lib.ptr(yd), ldy, ho, wo), "tn_dbg_maxpool")
    y = yd.cpu().numpy()
    ref = SR.maxpool_ref(x)
    assert ref.max() < 0
    assert np.array_equal(y[..., :C].astype(np.float64), ref)
    assert np.all(y[..., C:] == SENTINEL)


def _head_ref(x64, scale, shift, PH, PW):
    """float64 BatchNorm + ReLU + AvgPool2D(7) + NCHW flatten -> (feat (B, C PH PW), mean of |terms| in the same order)"""
    b, h, w, c = x64.shape
    terms = np.maximum(x64 * scale.astype(np.float64) + shift.astype(np.float64), 0.0)
    win = terms[:, :7 * PH, :7 * PW].reshape(b, PH, 7, PW, 7, c)
    mean = win.mean(axis=(2, 4))                                             # (B,PH,PW,C)
    return mean.transpose(0, 3, 1, 2).reshape(b, -1), np.abs(win).mean(axis=(2, 4)).transpose(0, 3, 1, 2).reshape(b, -1), mean


@pytest.mark.parametrize("x32", [False, True], ids=["f16", "x32"])
@pytest.mark.parametrize("H,W,PH,PW,C,B", [(7, 7, 1, 1, 1024, 5), (14, 14, 2, 2, 1024, 3), (16, 16, 2, 2, 1024, 3), (8, 8, 1, 1, 520, 3), (7, 7, 1, 1, 8, 1)])
def test_head_against_float64(ctx, report, H, W, PH, PW, C, B, x32):
    """head_kernel<false> (fp16 map) and <true> (fp32 side buffer; the fp16 pointer is poisoned and must not be read).  Bound:
    64 * 2^-24 * mean |terms| (49 fp32 additions, the fma of every term, the 1 / 49) plus one fp32 ulp of the result.  Random data give
    every (frame, channel, ph, pw) an expected value of its own, so the flatten index c PH PW + ph PW + pw is checked by the values.
    16 x 16 with PH = PW = 2: oracle/densenet_np.avgpool is AvgPool2D(7), stride 7, no padding, floor - windows at rows / columns
    0-6 and 7-13, the remainder rows and columns 14, 15 are dropped; asserted here by planting large values there."""
    from oracle import densenet_np as dn
    from tennis_amd import _lib
    rng = np.random.default_rng(H * W + C + B)
    xf = rng.normal(0, 1.5, (B, H, W, C)).astype(np.float32)
    if H > 7 * PH:
        xf[:, 7 * PH:] = 1000.0; xf[:, :, 7 * PW:] = 1000.0                   # what the oracle drops
    scale = (rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.4, -1.0, 1.0)).astype(np.float32)
    shift = rng.normal(0, 0.3, C).astype(np.float32)
    xh = xf.astype(np.float16)
    x64 = (xf if x32 else xh).astype(np.float64)
    ref, mag, ref_nhwc = _head_ref(x64, scale, shift, PH, PW)
    # the oracle's own pooling and flatten of the same terms (fp32) agree with the float64 restatement
    terms32 = np.maximum(x64 * scale.astype(np.float64) + shift.astype(np.float64), 0.0).astype(np.float32)
    orc = np.ascontiguousarray(dn.avgpool(terms32, 7).transpose(0, 3, 1, 2)).reshape(B, -1)
    assert orc.shape == ref.shape == (B, C * PH * PW) and np.abs(orc - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())
    poison = torch.full((B, H, W, C), float("nan"), dtype=torch.float16, device="cuda")
    xd = torch.from_numpy(xf).cuda() if x32 else torch.from_numpy(xh).cuda()
    sd, td = torch.from_numpy(scale).cuda(), torch.from_numpy(shift).cuda()
    fd = torch.full((B, C * PH * PW), -3.0, dtype=torch.float32, device="cuda")
    _lib.check(ctx.lib.tn_dbg_head(ctx.handle, _lib.ptr(poison if x32 else xd), _lib.ptr(xd if x32 else None), B, H, W, C, _lib.ptr(sd), _lib.ptr(td),
                                   _lib.ptr(fd), PH, PW), "tn_dbg_head")
    got = fd.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    ulp32 = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 23)
    bound = 64 * 2.0 ** -24 * mag + ulp32
    err = np.abs(got - ref)
    key = f"head_{'x32' if x32 else 'f16'}_{H}x{W}_p{PH}x{PW}_c{C}_err_over_bound"
    print("%s: %.3f (max err %.3g)" % (key, (err / bound).max(), err.max()))
    report[key] = float((err / bound).max())
    assert np.all(err <= bound)
    if PH * PW > 1:      # the check discriminates: the same values in another flatten order miss the bound
        for other in (ref_nhwc.reshape(B, -1), ref_nhwc.transpose(0, 3, 2, 1).reshape(B, -1)):
            assert not np.all(np.abs(got - other) <= bound)


def test_hooks_refuse_bad_arguments(ctx):
    from tennis_amd import _lib
    lib, h = ctx.lib, ctx.handle
    p = SR.stem_params("refusals")
    a = [_fp(np.ascontiguousarray(p[k], np.float32)) for k in ("w0", "gamma", "beta", "mean", "var")]
    x = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="cuda")
    y = torch.full((1, 16, 16, 64), SENTINEL, dtype=torch.float16, device="cuda")

    def refused(rc, word):
        msg = lib.tn_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    refused(lib.tn_dbg_stem(h, *a, None, 0, 1, 3, 1, 64, 64, _lib.ptr(x), _lib.ptr(y), 64), "layout")
    refused(lib.tn_dbg_stem(h, *a, None, 0, 1, 2, 1, 64, 64, _lib.ptr(x), _lib.ptr(y), 60), "stride")
    refused(lib.tn_dbg_stem(h, *a, None, 0, 1, 2, 1, 64, 8, _lib.ptr(x), _lib.ptr(y), 64), "shape")
    refused(lib.tn_dbg_stem(h, *a, None, 0, 1, 2, 0, 64, 64, _lib.ptr(x), _lib.ptr(y), 64), "shape")
    refused(lib.tn_dbg_stem(h, *a, None, 1, 0, 2, 1, 64, 64, _lib.ptr(x), _lib.ptr(y), 64), "exact")
    refused(lib.tn_dbg_stem(h, a[0], None, *a[2:], None, 0, 1, 2, 1, 64, 64, _lib.ptr(x), _lib.ptr(y), 64), "null")
    refused(lib.tn_dbg_stem(h, *a, None, 0, 1, 2, 1, 64, 64, None, _lib.ptr(y), 64), "null")
    assert torch.all(y == SENTINEL)
    m = torch.zeros((1, 9, 13, 8), dtype=torch.float16, device="cuda")
    o = torch.zeros((1, 5, 7, 8), dtype=torch.float16, device="cuda")
    refused(lib.tn_dbg_maxpool(h, _lib.ptr(m), 1, 9, 13, 8, _lib.ptr(o), 8, 4, 7), "output")
    refused(lib.tn_dbg_maxpool(h, _lib.ptr(m), 1, 9, 13, 8, _lib.ptr(o), 4, 5, 7), "shape")
    refused(lib.tn_dbg_maxpool(h, _lib.ptr(m), 1, 9, 13, 12, _lib.ptr(o), 16, 5, 7), "multiple of 8")
    refused(lib.tn_dbg_maxpool(h, None, 1, 9, 13, 8, _lib.ptr(o), 8, 5, 7), "null")
    s = torch.zeros(16, dtype=torch.float32, device="cuda")
    f = torch.zeros(64, dtype=torch.float32, device="cuda")
    hm = torch.zeros((1, 7, 7, 16), dtype=torch.float16, device="cuda")
    refused(lib.tn_dbg_head(h, _lib.ptr(hm), None, 1, 7, 7, 16, _lib.ptr(s), _lib.ptr(s), _lib.ptr(f), 2, 1), "shape")
    refused(lib.tn_dbg_head(h, _lib.ptr(hm), None, 1, 7, 7, 12, _lib.ptr(s), _lib.ptr(s), _lib.ptr(f), 1, 1), "multiple of 8")
    refused(lib.tn_dbg_head(h, None, None, 1, 7, 7, 16, _lib.ptr(s), _lib.ptr(s), _lib.ptr(f), 1, 1), "null")
    refused(lib.tn_dbg_head(h, _lib.ptr(hm), None, 1, 7, 7, 16, None, _lib.ptr(s), _lib.ptr(f), 1, 1), "null")
