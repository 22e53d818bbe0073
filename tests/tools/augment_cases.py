"""The edge cases of the train-time augmentation (tn_augment_forward), as data: source shapes, crop windows, colour records and
frames.  tests/test_cpu_image_edges.py holds the oracle (oracle/image_np.py) to a scalar restatement on them,
tests/test_gpu_augment_edges.py the kernels to the oracle.  Nothing here is drawn by the transform's generator: every record is
written down, so that each edge is met on purpose."""
import itertools

import numpy as np

ORDERS = list(itertools.permutations(range(4)))      # 0 brightness, 1 contrast, 2 saturation, 3 hue (nothing)
WINDOW_NAMES = ("first_pixel", "last_pixel", "one_row", "one_column", "enlarge_5x3", "whole_frame", "ends_at_WH", "one_to_one",
                "twice_in_x_only", "twice_in_y_only", "twice_both_odd_origin")
ENDS_AT_WH = ("last_pixel", "whole_frame", "ends_at_WH")      # windows whose last byte is the frame's last byte


def sources(size):
    """(H, W) of the source frames for an output size: the two small frames where every window fits them, otherwise the smallest
    frame with room for a 2x window at an odd origin and one more row / column behind it."""
    if 2 * size + 1 <= 45:
        return [(45, 61), (64, 64)]
    return [(2 * size + 3, 2 * size + 6)]


def windows(H, W, size):
    """name -> (x0, y0, cw, ch) in an H x W source for output size x size; see the assertions for what each has to be"""
    s2 = 2 * size
    cw, ch = W // 2 + 2, H // 3 + 1
    w = {"first_pixel": (0, 0, 1, 1),
         "last_pixel": (W - 1, H - 1, 1, 1),
         "one_row": (0, 0, W, 1),
         "one_column": (0, 0, 1, H),
         "enlarge_5x3": (7, 4, 5, 3),
         "whole_frame": (0, 0, W, H),
         "ends_at_WH": (W - cw, H - ch, cw, ch),
         "one_to_one": (2, 1, size, size),
         "twice_in_x_only": (1, 2, s2, s2 + 1),
         "twice_in_y_only": (2, 1, s2 + 1, s2),
         "twice_both_odd_origin": (1, 3, s2, s2)}
    assert tuple(w) == WINDOW_NAMES
    for name, (x0, y0, a, b) in w.items():
        assert x0 >= 0 and y0 >= 0 and a > 0 and b > 0 and x0 + a <= W and y0 + b <= H, (name, H, W, size)
        assert (a == s2 and b == s2) == (name == "twice_both_odd_origin"), (name, H, W, size)      # the box path: that one only
        if name in ENDS_AT_WH:
            assert x0 + a == W and y0 + b == H
    return w


def takes_box(win, size):
    return win[2] == 2 * size and win[3] == 2 * size


def record(win, flip, k):
    """A whole record for window ``win``: the k-th operator order, alphas and lighting offsets that change with k (both ends of the
    jitter's range, 0.6 and 1.4, among them)"""
    alphas = (0.6, 1.4, 1.0, 0.8125, 1.37)
    return dict(win=tuple(int(v) for v in win), flip=int(flip), order=list(ORDERS[(5 * k + 3) % 24]), brightness=alphas[k % 5],
                contrast=alphas[(k + 1) % 5], saturation=alphas[(k + 3) % 5],
                light=[(-1) ** k * 3.25 * (k % 4), 1.5 - k % 3, (-1) ** (k // 2) * 0.7 * (k % 5)])


def geometry_records(H, W, size):
    """The 11 windows with flip 0 and flip 1: 22 records, in WINDOW_NAMES order"""
    w = windows(H, W, size)
    return [dict(record(w[n], flip, 2 * i + flip), name=f"{n}/flip{flip}") for i, n in enumerate(WINDOW_NAMES) for flip in (0, 1)]


def batches_of_5(recs):
    """Index lists into ``geometry_records``: four other windows and, as the batch's LAST frame, one that ends at (W, H) - a read
    past it is a read past the batch."""
    last = [i for i, r in enumerate(recs) if r["name"].split("/")[0] in ENDS_AT_WH]
    rest = [i for i in range(len(recs)) if i not in last]
    assert len(rest) == 16 and len(last) == 6
    return [rest[4 * j:4 * j + 4] + [last[j]] for j in range(4)]


def frames(H, W, n, seed, kind="random"):
    """(n, H, W, 3) uint8.  random: 0..255; dark: 0..60; halves: the left half 0..40, the right half 200..255; black / white."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if kind == "dark":
        return rng.integers(0, 61, (n, H, W, 3), dtype=np.uint8)
    if kind == "halves":
        f = rng.integers(0, 41, (n, H, W, 3), dtype=np.uint8)
        f[:, :, W // 2:] = rng.integers(200, 256, (n, H, W - W // 2, 3), dtype=np.uint8)
        return f
    if kind in ("black", "white"):
        return np.full((n, H, W, 3), 0 if kind == "black" else 255, np.uint8)
    raise ValueError(kind)


# Colour cases: (frame kind, order, brightness, contrast, saturation, light, what has to saturate in the ORACLE's output: "lo" at
# least 1 % of the values 0, "hi" at least 1 % 255).  The shares the alphas give on random 0..255 content: (1.4, 1.4, 1.4, +30)
# 45 % at 255; (0.6, 0.6, 0.6, -30) only 0.016 % at 0, hence the dark frames.
B_C_S_H, C_B_S_H, B_S_H_C, S_B_C_H = [0, 1, 2, 3], [1, 0, 2, 3], [0, 2, 3, 1], [2, 0, 1, 3]
COLOUR_CASES = [
    ("random", B_C_S_H, 1.4, 1.4, 1.4, [30.0, 30.0, 30.0], "hi"),
    ("dark", B_C_S_H, 0.6, 0.6, 0.6, [-30.0, -30.0, -30.0], "lo"),
    ("halves", S_B_C_H, 1.4, 1.4, 0.6, [-12.5, 20.25, -3.0], "lohi"),      # contrast 1.4 about a mid grey: both ends in one image
    ("halves", B_C_S_H, 0.6, 1.4, 1.4, [-30.0, -11.0, -30.0], "lo"),
    ("black", B_C_S_H, 1.4, 0.6, 1.4, [-30.0, 30.0, 0.0], "lo"),
    ("white", B_C_S_H, 0.6, 1.4, 0.6, [150.0, -30.0, 0.5], "hi"),
    ("white", C_B_S_H, 1.4, 1.4, 1.4, [0.0, 0.0, 0.0], "hi"),
    # contrast position.  First: the mean grey of the resized image itself.  Last, behind a brightness that saturates the bright
    # half: the mean grey has to be that of the SATURATED bytes (a mean taken in front of the brightness operator, or of unsaturated
    # products, is another number)
    ("halves", C_B_S_H, 1.4, 0.6, 1.0, [4.0, -4.0, 0.0], "hi"),
    ("halves", B_S_H_C, 1.4, 1.4, 0.6, [-2.0, 0.0, 2.0], "lohi"),
    ("random", B_S_H_C, 1.4, 0.6, 1.4, [0.0, -7.5, 7.5], None),
    ("random", C_B_S_H, 0.6, 1.4, 0.6, [-30.0, 0.0, 30.0], "lo"),
]


def colour_records(H, W, size):
    """-> (frames (n, H, W, 3), records, expectations): one frame per colour case, windows that change from frame to frame (whole
    frame, a mild reduction / enlargement, flipped every other time)"""
    fr, recs, expect = [], [], []
    for i, (kind, order, b, c, s, light, exp) in enumerate(COLOUR_CASES):
        fr.append(frames(H, W, 1, 100 + i, kind)[0])
        win = (0, 0, W, H) if i % 2 == 0 else (W // 8, H // 8, W - W // 4, H - H // 4)
        recs.append(dict(win=win, flip=i % 2, order=list(order), brightness=b, contrast=c, saturation=s, light=list(light),
                         name=f"colour{i}/{kind}"))
        expect.append(exp)
    return np.stack(fr), recs, expect


def oracle(im, frame, r, size):
    x0, y0, cw, ch = r["win"]
    return im.augment_u8(frame, x0, y0, cw, ch, r["flip"], r["order"], r["brightness"], r["contrast"], r["saturation"], r["light"], size)
