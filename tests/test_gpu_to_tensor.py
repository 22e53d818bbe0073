"""-m gpu: tn_to_tensor_normalize (csrc/preprocess.hip), the input of the fine-tuning, CNN-RNN and captioner-from-frames steps,
bitwise against the float32 evaluation of the formula the header documents, (x / 255 - mean) / std with numpy float32 scalars: every
byte value in every channel at each of the 12 byte positions of a four-pixel group, pixel counts on both sides of a group and of a
workgroup (the byte-wise tail), and source / destination pointers off the alignment the 12-bytes-in / three-float4-out path needs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
OTHER = ((0.1, 0.5, 0.8125), (0.3, 1.0, 0.07))            # a std of exactly 1 and parameters that are no ImageNet numbers


def _table(mean, std):
    """(256, 3) float32: the documented formula, one numpy float32 scalar operation after the other; and the same in float64 on
    the same float32 parameters"""
    t32, t64 = np.zeros((256, 3), np.float32), np.zeros((256, 3), np.float64)
    for c in range(3):
        m, s = np.float32(mean[c]), np.float32(std[c])
        for v in range(256):
            t32[v, c] = (np.float32(v) / np.float32(255.0) - m) / s
            t64[v, c] = (v / 255.0 - float(m)) / float(s)
    return t32, t64


def _want(src_np, mean, std):
    t32, t64 = _table(mean, std)
    x = src_np.reshape(-1, 3).astype(np.int64)
    ch = np.arange(3)[None, :]
    return t32[x, ch], t64[x, ch]


def _abi(ctx, src, pixels, mean, std, dst):
    from tennis_amd import _lib
    m, sd = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    rc = ctx.lib.tn_to_tensor_normalize(ctx.handle, _lib.ptr(src), pixels, m, sd, _lib.ptr(dst))
    torch.cuda.synchronize()
    return rc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def test_the_two_float32_formulas_differ():
    """Why the kernel divides: multiplying by the float32 1 / std is another number for 230 of the 768 (byte, channel) pairs"""
    t32, _ = _table(*IMAGENET)
    mul = np.zeros_like(t32)
    for c in range(3):
        inv = np.float32(1.0) / np.float32(IMAGENET[1][c])
        for v in range(256):
            mul[v, c] = (np.float32(v) / np.float32(255.0) - np.float32(IMAGENET[0][c])) * inv
    assert int((_bits(mul) != _bits(t32)).sum()) == 230


@pytest.mark.parametrize("mean,std", [IMAGENET, OTHER])
def test_every_byte_value_in_every_channel_at_every_position_of_a_group(ctx, report, mean, std):
    from tennis_amd.engine import to_tensor_normalize
    g, j = np.meshgrid(np.arange(256), np.arange(12), indexing="ij")
    src = ((g + 21 * j) % 256).astype(np.uint8)              # group g, byte j: as g runs, every position sees every value
    for pos in range(12):
        assert len(set(src[:, pos].tolist())) == 256
    got = to_tensor_normalize(torch.from_numpy(src.reshape(1, 32, 32, 3)).cuda(), mean, std, ctx).cpu().numpy().reshape(-1, 3)
    w32, w64 = _want(src, mean, std)
    report[f"to_tensor_normalize_maxabs_err_vs_f64_std{std[0]}"] = float(np.abs(got.astype(np.float64) - w64).max())
    bad = np.argwhere(_bits(got) != _bits(w32))
    assert len(bad) == 0, (len(bad), [(int(src.reshape(-1, 3)[p, c]), int(c), float(got[p, c]), float(w32[p, c])) for p, c in bad[:4]])


@pytest.mark.parametrize("pixels", [1, 2, 3, 4, 5, 1023, 1024, 1025, 4 * 256 + 3])
def test_pixel_counts_around_a_group_and_a_workgroup(ctx, pixels):
    """Every float of dst is written, tail pixels included, and nothing behind them: dst starts as NaN with 16 floats of guard"""
    rng = np.random.default_rng(pixels)
    src = rng.integers(0, 256, (pixels, 3), dtype=np.uint8)
    dst = torch.full((pixels * 3 + 16,), float("nan"), device="cuda")
    assert _abi(ctx, torch.from_numpy(src).cuda(), pixels, *IMAGENET, dst) == 0
    got = dst.cpu().numpy()
    w32, _ = _want(src, *IMAGENET)
    assert np.array_equal(_bits(got[:pixels * 3]), _bits(w32.ravel()))
    assert np.isnan(got[pixels * 3:]).all()


def test_an_odd_frame_shape_with_other_parameters(ctx):
    from tennis_amd.engine import to_tensor_normalize
    src = np.random.default_rng(3).integers(0, 256, (2, 15, 15, 3), dtype=np.uint8)          # 450 pixels: 112 groups and 2 pixels
    got = to_tensor_normalize(torch.from_numpy(src).cuda(), *OTHER, ctx)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 15, 15, 3)
    assert np.array_equal(_bits(got.cpu().numpy().reshape(-1, 3)), _bits(_want(src, *OTHER)[0]))


@pytest.mark.parametrize("src_off", [0, 1, 2, 3])
@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
def test_pointers_off_the_vector_path_alignment(ctx, src_off, dst_off):
    """src a contiguous view that starts src_off bytes into a flat buffer, dst one that starts dst_off floats into another: the
    launcher takes the byte-wise loop unless src is 4-byte and dst 16-byte aligned.  Same bits either way, nothing written outside."""
    pixels = 4 * 256 + 3
    src = np.random.default_rng(10 * src_off + dst_off).integers(0, 256, (pixels, 3), dtype=np.uint8)
    sbuf = torch.zeros((pixels * 3 + 8,), dtype=torch.uint8, device="cuda")
    dbuf = torch.full((pixels * 3 + 24,), float("nan"), device="cuda")
    assert sbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
    sview = sbuf[src_off:src_off + pixels * 3]
    sview.copy_(torch.from_numpy(src.ravel()))
    dview = dbuf[4 + dst_off:4 + dst_off + pixels * 3]
    assert sview.is_contiguous() and sview.data_ptr() % 4 == src_off and dview.data_ptr() % 16 == 4 * dst_off
    assert _abi(ctx, sview, pixels, *IMAGENET, dview) == 0
    got = dbuf.cpu().numpy()
    lo = 4 + dst_off
    assert np.array_equal(_bits(got[lo:lo + pixels * 3]), _bits(_want(src, *IMAGENET)[0].ravel()))
    assert np.isnan(got[:lo]).all() and np.isnan(got[lo + pixels * 3:]).all()


def test_a_misaligned_view_through_the_module_function(ctx):
    from tennis_amd.engine import to_tensor_normalize
    src = np.random.default_rng(5).integers(0, 256, (6, 7, 3), dtype=np.uint8)
    buf = torch.zeros((6 * 7 * 3 + 4,), dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3):
        view = buf[off:off + 126].view(6, 7, 3)
        view.copy_(torch.from_numpy(src))
        assert view.is_contiguous() and view.data_ptr() % 4 == off
        got = to_tensor_normalize(view, ctx=ctx).cpu().numpy()
        assert np.array_equal(_bits(got.reshape(-1, 3)), _bits(_want(src, *IMAGENET)[0]))


def test_zero_std_is_still_refused(ctx):
    src = torch.zeros((4, 3), dtype=torch.uint8, device="cuda")
    dst = torch.full((12,), float("nan"), device="cuda")
    for k in range(3):
        std = [0.229, 0.224, 0.225]
        std[k] = 0.0
        assert _abi(ctx, src, 4, IMAGENET[0], std, dst) != 0
        assert b"zero std" in ctx.lib.tn_last_error()
    assert bool(torch.isnan(dst).all())
