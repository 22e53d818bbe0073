"""The image oracle (oracle/image_np.py) against a per-pixel scalar restatement written only for this file, on the edge windows that
tests/test_gpu_augment_edges.py holds the augmentation kernels to.  The oracle is vectorised, so an indexing mistake in it could be
the kernel's mistake too; the restatement below has no array indexing beyond img[y][x][c] and follows the text of the oracle's
docstring one output pixel at a time.  Also the two facts the GPU test leans on: the image's mean grey does not depend on the order
of the sum, and the oracle accepts every window at the sizes around the crop kernel's 256-thread workgroup."""
import math

import numpy as np
import pytest

from oracle import image_np as im
from tools import augment_cases as AC

F = np.float32


def _tap(d, src, dst, clamp):
    """One axis of cv::resize's INTER_LINEAR table: the coordinate (d + 0.5) * scale - 0.5 worked out in double and held as a float,
    the first source index, and the two 11-bit coefficients rounded half to even (Python's round is cvRound's rounding)."""
    f = F((d + 0.5) * (float(src) / dst) - 0.5)
    s = math.floor(float(f))
    f = F(f - F(s))
    if clamp:                      # the x axis: at the borders the offset is clamped and the fraction dropped
        if s < 0:
            s, f = 0, F(0)
        if s >= src - 1:
            s, f = src - 1, F(0)
    return s, round(float(F(F(1) - f) * F(2048))), round(float(f * F(2048)))


def _resize_scalar(img, out_h, out_w, box=True):
    H, W = len(img), len(img[0])
    out = np.zeros((out_h, out_w, 3), np.uint8)
    for y in range(out_h):
        for x in range(out_w):
            for c in range(3):
                if box and W == 2 * out_w and H == 2 * out_h:      # the INTER_AREA 2 x 2 average substituted for an exact 2x reduction
                    v = (int(img[2 * y][2 * x][c]) + int(img[2 * y][2 * x + 1][c]) + int(img[2 * y + 1][2 * x][c])
                         + int(img[2 * y + 1][2 * x + 1][c]) + 2) >> 2
                else:
                    sx, a0, a1 = _tap(x, W, out_w, True)
                    sy, b0, b1 = _tap(y, H, out_h, False)
                    x1 = min(sx + 1, W - 1)
                    r0, r1 = min(max(sy, 0), H - 1), min(max(sy + 1, 0), H - 1)      # the y axis: rows are clipped when they are read
                    s0 = int(img[r0][sx][c]) * a0 + int(img[r0][x1][c]) * a1
                    s1 = int(img[r1][sx][c]) * a0 + int(img[r1][x1][c]) * a1
                    v = (((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2
                assert 0 <= v <= 255, (y, x, c, v)
                out[y, x, c] = v
    return out


def _sat(v):
    """saturate_cast<uint8>(float) as the oracle takes it: clamp, then truncate"""
    return int(min(max(v, F(0)), F(255)))


def _gray(p):
    return F(F(F(p[0]) * F(0.299)) + F(F(p[1]) * F(0.587))) + F(F(p[2]) * F(0.114))


def _augment_scalar(img, r, size):
    x0, y0, cw, ch = r["win"]
    a = _resize_scalar([row[x0:x0 + cw] for row in img[y0:y0 + ch]], size, size)
    if r["flip"]:
        a = np.stack([[a[y, size - 1 - x] for x in range(size)] for y in range(size)])
    px = [[[int(v) for v in a[y, x]] for x in range(size)] for y in range(size)]
    b, c, s = F(r["brightness"]), F(r["contrast"]), F(r["saturation"])
    for op in r["order"]:
        if op == 1:           # the mean grey of the image as this operator finds it
            gm = F(math.fsum(float(_gray(p)) for row in px for p in row) / (size * size))
        for row in px:
            for p in row:
                if op == 0:
                    p[:] = [_sat(F(v) * b) for v in p]
                elif op == 1:
                    p[:] = [_sat(F(F(v) * c) + F(F(1) - c) * gm) for v in p]
                elif op == 2:
                    g = _gray(p) * F(F(1) - s)
                    p[:] = [_sat(F(F(v) * s) + g) for v in p]
    return np.array([[[_sat(F(v) + F(l)) for v, l in zip(p, r["light"])] for p in row] for row in px], np.uint8)


@pytest.mark.parametrize("size", [1, 2, 7, 33])
def test_oracle_matches_the_scalar_restatement_on_the_edge_windows(size):
    for H, W in AC.sources(size):
        frame = AC.frames(H, W, 1, 7 * size + H)[0]
        rows = frame.tolist()
        for r in AC.geometry_records(H, W, size):
            x0, y0, cw, ch = r["win"]
            want = _resize_scalar([row[x0:x0 + cw] for row in rows[y0:y0 + ch]], size, size)
            got = im.resize_bilinear_u8(frame[y0:y0 + ch, x0:x0 + cw], size, size)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (r["name"], H, W)
            assert np.array_equal(AC.oracle(im, frame, r, size), _augment_scalar(rows, r, size)), (r["name"], H, W)


@pytest.mark.parametrize("size", [1, 7])
def test_oracle_colour_matches_the_scalar_restatement(size):
    """The jitter and lighting arithmetic on the frames that saturate: dark, half dark and half bright, all 0, all 255; contrast
    first and contrast last."""
    H, W = AC.sources(size)[0]
    fr, recs, _ = AC.colour_records(H, W, size)
    for f, r in zip(fr, recs):
        assert np.array_equal(AC.oracle(im, f, r, size), _augment_scalar(f.tolist(), r, size)), r["name"]


def test_exact_2x_bilinear_equals_the_box_average():
    """Why no output can tell which path an exact 2x window took: its coordinates are 2 d + 0.5, all four coefficients 1024, and
    ((1024 * ((a + b) * 1024 >> 4)) >> 16) = a + b, so the fixed-point bilinear IS (a + b + c + d + 2) >> 2.  What the tests can see
    is the box path taken where only ONE axis is 2x - and there the two differ."""
    img = AC.frames(14, 18, 1, 3)[0].tolist()
    assert np.array_equal(_resize_scalar(img, 7, 9, box=True), _resize_scalar(img, 7, 9, box=False))
    frame = AC.frames(45, 61, 1, 4)[0]
    w = AC.windows(45, 61, 7)
    for name in ("twice_in_x_only", "twice_in_y_only"):
        x0, y0, cw, ch = w[name]
        a = frame[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
        a = a[:14, :14]                                   # what a box path would read: rows 2 y, 2 y + 1, columns 2 x, 2 x + 1
        box = ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        assert not np.array_equal(im.resize_bilinear_u8(frame[y0:y0 + ch, x0:x0 + cw], 7, 7), box), name


def test_mean_grey_does_not_depend_on_the_order_of_the_sum():
    """aug_gray_mean_kernel adds the float32 grey values in double, 256 strided partial sums and a tree; the oracle adds them with
    numpy's pairwise sum.  At 512 x 512 every grey value is a multiple of 2^-27 below 2^8, so a sum of 2^18 of them stays below
    2^53 units and every order gives the same double."""
    img = AC.frames(512, 512, 1, 12)[0]
    g = im._gray(img)
    assert g.dtype == np.float32 and g.shape == (512, 512)
    units = g.astype(np.float64) * 2.0 ** 27
    assert np.array_equal(units, np.floor(units)) and float(units.max()) < 2.0 ** 35
    flat = g.astype(np.float64).ravel()
    exact = math.fsum(flat.tolist())
    forward = float(np.add.accumulate(flat)[-1])                     # accumulate adds one element after the other
    reverse = float(np.add.accumulate(flat[::-1])[-1])
    part = np.add.accumulate(flat.reshape(-1, 256), axis=0)[-1]      # thread t: elements t, t + 256, ...
    o = 128
    while o:                                                         # the kernel's tree
        part = part[:o] + part[o:2 * o]
        o >>= 1
    assert forward == exact and reverse == exact and float(part[0]) == exact and float(flat.sum()) == exact


@pytest.mark.parametrize("size", [1, 2, 7, 255, 256, 257])
def test_oracle_accepts_every_window(size):
    for H, W in AC.sources(size):
        frame = AC.frames(H, W, 1, size)[0]
        recs = AC.geometry_records(H, W, size)
        assert len(recs) == 22
        for r in recs:
            out = AC.oracle(im, frame, r, size)
            assert out.shape == (size, size, 3) and out.dtype == np.uint8, r["name"]


def test_column_256_is_not_a_copy_of_column_255():
    """At size 257 output column 256 is the one pixel of a row that the crop kernel's second workgroup computes.  A slip by one there
    (column 255's taps) can only be seen where the two columns differ.  Column 255 sits on the clamped last source pixel, as
    column 256 always does, when 255.5 cw / 257 - 0.5 >= cw - 1, that is cw <= 85: the one-pixel-wide windows and the 5 x 3 one.
    The seven wider windows tell the two columns apart, with either flip."""
    (H, W), = AC.sources(257)
    frame = AC.frames(H, W, 1, 5)[0]
    seen = 0
    for r in AC.geometry_records(H, W, 257):
        out = AC.oracle(im, frame, r, 257)
        a, b = (out[:, 0], out[:, 1]) if r["flip"] else (out[:, 256], out[:, 255])        # a flip stores column x at size - 1 - x
        assert np.array_equal(a, b) == (r["win"][2] <= 85), r["name"]
        seen += r["win"][2] > 85
    assert seen == 14


def test_colour_cases_saturate_where_they_say():
    """The shares the GPU test asserts, here without a GPU: every colour case marked lo / hi has at least 1 % of its oracle output
    at 0 / at 255, at both sizes the GPU test uses."""
    for size in (7, 257):
        H, W = AC.sources(size)[0]
        fr, recs, expect = AC.colour_records(H, W, size)
        for f, r, e in zip(fr, recs, expect):
            out = AC.oracle(im, f, r, size)
            lo, hi = float((out == 0).mean()), float((out == 255).mean())
            assert (lo >= 0.01 or "lo" not in (e or "")) and (hi >= 0.01 or "hi" not in (e or "")), (size, r["name"], lo, hi)
