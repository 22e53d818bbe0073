"""-m gpu: tn_augment_forward (aug_crop_resize_kernel, aug_gray_mean_kernel, aug_color_kernel; csrc/preprocess.hip) at its edges,
bit for bit against oracle/image_np.py::augment_u8 fed the same records.  The records are written down (tests/tools/augment_cases.py),
not drawn: windows of one pixel, one row, one column, the frame's last pixel, windows that end on its last row and column, enlarging,
1:1, 2x on one axis only and on both from an odd origin; output sizes on both sides of the 256 threads of a workgroup, where a row of
the crop kernel first spans two; colour records that really saturate to 0 and to 255; contrast in front of and behind a saturating
brightness.  tests/test_cpu_image_edges.py holds the oracle itself to a scalar restatement on the same cases."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import image_np as im
from tools import augment_cases as AC

pytestmark = pytest.mark.gpu


def _compose(size, seed=0):
    from tennis_amd import transforms as T
    return T.Compose([T.RandomResizedCrop(size), T.RandomFlipLeftRight(), T.RandomColorJitter(0.4, 0.4, 0.4), T.RandomLighting(0.1),
                      T.ToTensor(), T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])], seed=seed)


def _rec(recs):
    from tennis_amd.transforms import AugFrame
    out = (AugFrame * len(recs))()
    for i, r in enumerate(recs):
        out[i] = AugFrame(*r["win"], r["flip"], sum(o << (2 * k) for k, o in enumerate(r["order"])), r["brightness"], r["contrast"],
                          r["saturation"], (C.c_float * 3)(*r["light"]))
    return out


def _run(tf, frames_dev, idx, recs):
    """frames idx of the device batch with their records, one launch -> (len(idx), size, size, 3) uint8 on the host"""
    sel = frames_dev[torch.as_tensor(idx, device=frames_dev.device)].contiguous()
    return tf.augment(sel, _rec(recs)).cpu().numpy()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} bytes differ, first at (y, x, c) = {tuple(bad[0])}: "
                             f"{int(got[tuple(bad[0])])} for {int(want[tuple(bad[0])])}")


@pytest.mark.parametrize("size", [1, 7, 255, 256, 257])
def test_every_edge_window_alone_and_in_a_batch_of_five(size):
    """The 11 windows x 2 flips: each alone (batch 1), then in batches of 5 with a different window per frame, the last frame's window
    ending on the frame's last byte.  Frame j of the five belongs to record j mod 5 in both runs, so one oracle call serves both."""
    tf = _compose(size)
    for H, W in AC.sources(size):
        frames = AC.frames(H, W, 5, 31 * size + W)
        dev = torch.from_numpy(frames).cuda()
        recs = AC.geometry_records(H, W, size)
        groups = AC.batches_of_5(recs)
        slot = {i: k for g in groups for k, i in enumerate(g)}          # record -> its frame; the two records in no group: frame 0
        want = [AC.oracle(im, frames[slot.get(i, 0)], r, size) for i, r in enumerate(recs)]
        for i, r in enumerate(recs):
            _same(_run(tf, dev, [slot.get(i, 0)], [r])[0], want[i], f"size {size}, {H}x{W}, alone, {r['name']} {r['win']}")
        for g in groups:
            assert [slot[i] for i in g] == [0, 1, 2, 3, 4] and recs[g[-1]]["name"].split("/")[0] in AC.ENDS_AT_WH
            got = _run(tf, dev, [0, 1, 2, 3, 4], [recs[i] for i in g])
            for k, i in enumerate(g):
                _same(got[k], want[i], f"size {size}, {H}x{W}, frame {k} of 5, {recs[i]['name']} {recs[i]['win']}")


@pytest.mark.parametrize("size", [224, 512])
def test_training_sizes(size):
    """The two sizes training uses, one batch of five each: enlarging, 1:1, 2x in x only, 2x on both axes from an odd origin, and
    last a window that ends at (W, H).  At 512 a row spans two workgroups whichever path it takes."""
    (H, W), = AC.sources(size)
    frames = AC.frames(H, W, 5, size)
    recs = {r["name"]: r for r in AC.geometry_records(H, W, size)}
    pick = [recs[n] for n in ("enlarge_5x3/flip1", "one_to_one/flip0", "twice_in_x_only/flip1", "twice_both_odd_origin/flip1",
                              "ends_at_WH/flip0")]
    got = _run(_compose(size), torch.from_numpy(frames).cuda(), [0, 1, 2, 3, 4], pick)
    for k, r in enumerate(pick):
        _same(got[k], AC.oracle(im, frames[k], r, size), f"size {size}, frame {k}, {r['name']} {r['win']}")


@pytest.mark.parametrize("size", [7, 257])
def test_colour_saturates_at_both_ends_and_contrast_sees_what_is_in_front_of_it(size, report):
    """49 pixels (fewer than the grey-mean kernel's 256 threads) and 257 x 257.  The shares are the ORACLE's: every case marked lo has
    at least 1 % of its bytes at 0, every case marked hi at least 1 % at 255, and so has the batch as a whole - asserted before the
    device's output is looked at."""
    H, W = AC.sources(size)[0]
    frames, recs, expect = AC.colour_records(H, W, size)
    want = np.stack([AC.oracle(im, f, r, size) for f, r in zip(frames, recs)])
    for w, r, e in zip(want, recs, expect):
        lo, hi = float((w == 0).mean()), float((w == 255).mean())
        report[f"augment_edges_share_at_0_255_size{size}_{r['name']}"] = [lo, hi]
        assert lo >= 0.01 or "lo" not in (e or ""), (r["name"], lo)
        assert hi >= 0.01 or "hi" not in (e or ""), (r["name"], hi)
    assert float((want == 0).mean()) >= 0.01 and float((want == 255).mean()) >= 0.01
    got = _run(_compose(size), torch.from_numpy(frames).cuda(), list(range(len(recs))), recs)
    for k, r in enumerate(recs):
        _same(got[k], want[k], f"size {size}, {r['name']}, order {r['order']}")


def test_call_path_on_a_window_batch():
    """Compose.__call__ on a (2, 3, H, W, 3) window batch: shape, dtype, and the records it drew (last_params), fed to the oracle,
    reproduce every frame."""
    frames = AC.frames(45, 61, 6, 77).reshape(2, 3, 45, 61, 3)
    tf = _compose(33, seed=4)
    out = tf(frames)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (2, 3, 33, 33, 3)
    assert len(tf.last_params) == 1 and len(tf.last_params[0]) == 6
    got = out.cpu().numpy().reshape(6, 33, 33, 3)
    for i, r in enumerate(tf.last_params[0]):
        want = im.augment_u8(frames.reshape(6, 45, 61, 3)[i], r.x0, r.y0, r.cw, r.ch, r.flip, [(r.order >> (2 * k)) & 3 for k in range(4)],
                             r.brightness, r.contrast, r.saturation, list(r.light), 33)
        _same(got[i], want, f"call path, frame {i}, window {(r.x0, r.y0, r.cw, r.ch)}")
