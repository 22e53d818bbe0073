"""Dense evaluation through a row table, host side: the frame-level view of a ``TennisSet`` over ``window_table()``'s frames, the
video-boundary cutter for tables (``definitions.table_chunks``), ``evaluate --dense_windows``' flag logic, and the two new entry
points of the C ABI.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dataset(every, stride, split_first, window=7, **kw):
    from tennis_amd.dataset import TennisSet
    return TennisSet(root="/nonexistent", videos=("V1", "V2", "V3"), frames_per_video=11, window=window, every=every, stride=stride,
                     split_first=split_first, balance=False, synthetic=True, data_shape=8, **kw)


@pytest.mark.parametrize("every,stride,split_first", [(e, s, f) for e in (1, 2) for s in (1, 2, 3) for f in (3, 4)])
def test_frame_view_is_the_table_frames_in_order(every, stride, split_first):
    ds = _dataset(every, stride, split_first)
    frames, idx = ds.window_table()
    view = ds.frame_view()
    assert len(view) == len(frames) and view._window == 1
    assert [(s[0], s[1]) for s in view._samples] == list(frames)
    assert [view.sample_frames(i) for i in range(len(view))] == [[vf] for vf in frames]
    for i in (0, len(view) // 2, len(view) - 1):
        img, _label, j = view[i]
        assert j == i and img.shape == (3, 8, 8) and img.dtype == np.float32
        assert np.array_equal(img, ds._load(*frames[i]))                      # the dataset's own load + transform
    # a view of some of the frames, in the order given; the dataset itself is untouched
    some = [frames[3], frames[0]]
    assert [(s[0], s[1]) for s in ds.frame_view(some)._samples] == some
    assert ds._window == 7 and len(ds) == 3 * len(range(split_first, split_first + 11, every))
    # every window frame is in the view, also those that are no sample of the split
    in_split = {(s[0], s[1]) for s in ds._samples}
    assert {frames[r] for r in idx.ravel()} == set(frames)
    if split_first > 0 and stride * 3 > 1:
        assert set(frames) - in_split


def test_frame_view_goes_through_the_loader_and_a_device_batched_transform():
    from tennis_amd.dataset import DataLoader
    ds = _dataset(2, 3, 4)
    frames, _ = ds.window_table()
    batches = list(DataLoader(ds.frame_view(), batch_size=4))
    assert sum(len(b[0]) for b in batches) == len(frames) and batches[0][0].shape == (4, 3, 8, 8)
    assert np.array_equal(np.concatenate([b[2] for b in batches]), np.arange(len(frames)))
    assert np.array_equal(batches[1][0][2], ds._load(*frames[6]))

    class Batched:                      # the decoded uint8 frame is handed over, the transform runs once per batch
        device_batched = True

        def __call__(self, x):
            return x
    ds2 = _dataset(1, 1, 0, transform=Batched())
    img, _, _ = ds2.frame_view()[1]
    assert img.dtype == np.uint8 and np.array_equal(img, ds2.frame_u8(*ds2.window_table()[0][1]))


def _table(ds):
    frames, idx = ds.window_table()
    return frames, idx, [v for v, _ in frames]


@pytest.mark.parametrize("budget", [10 ** 6, 40, 27, 14])
def test_table_chunks_cut_at_video_boundaries(budget):
    from tennis_amd.models.vision.definitions import table_chunks
    ds = _dataset(2, 3, 4)
    frames, idx, vids = _table(ds)
    per_video = len(frames) // 3
    assert per_video <= 14 < 2 * per_video                                     # 14: one video per piece; 27 / 40: two and one
    pieces = table_chunks(idx, vids, budget)
    assert pieces[0][0] == 0 and pieces[-1][1] == len(frames)
    assert all(p[1] == q[0] for p, q in zip(pieces, pieces[1:]))
    assert sorted(np.concatenate([p[2] for p in pieces]).tolist()) == list(range(len(ds)))       # every sample once
    for a, b, ids, local in pieces:
        assert b - a <= budget
        assert a == 0 or vids[a] != vids[a - 1]                                # a cut is a video boundary
        assert np.array_equal(local, idx[ids] - a)
        assert local.min() >= 0 and local.max() < b - a                        # every index of a sample inside its piece
    assert len(pieces) == {10 ** 6: 1, 40: 1 if len(frames) <= 40 else 2, 27: 2, 14: 3}[budget]


def test_table_chunks_refusals():
    from tennis_amd.models.vision.definitions import table_chunks
    ds = _dataset(2, 3, 4)
    frames, idx, vids = _table(ds)
    per_video = len(frames) // 3
    with pytest.raises(ValueError, match="does not fit"):
        table_chunks(idx, vids, per_video - 1)
    bad = idx.copy()
    bad[0, 0] = len(frames) - 1                                                # a sample that reads two videos
    with pytest.raises(ValueError, match="two videos"):
        table_chunks(bad, vids, per_video)
    bad[0, 0] = -1
    with pytest.raises(ValueError, match="inside"):
        table_chunks(bad, vids, per_video)
    assert len(table_chunks(bad, vids, 10 ** 6)) == 1                          # a table that fits is not inspected: the kernel clamps


def test_evaluate_dense_windows_flag_logic():
    from tennis_amd.evaluate import build_parser, check_dense_windows
    parse = build_parser().parse_args
    assert check_dense_windows(parse(["--dense_windows", "--window", "7", "--temp_pool", "gru"])) == "frames"
    assert check_dense_windows(parse(["--dense_windows", "--window", "7", "--temp_pool", "max"])) == "frames"
    assert check_dense_windows(parse(["--dense_windows", "--window", "7", "--temp_pool", "lstm", "--feats_model", "0006"])) == "windows"
    assert check_dense_windows(parse(["--window", "1"])) is None                # without the flag nothing is checked
    assert check_dense_windows(parse(["--dense_windows", "--corpus_frames", "64", "--window", "1"])) is None
    for argv, why in ((["--dense_windows", "--window", "1", "--temp_pool", "gru"], r"--window W \(> 1\)"),
                      (["--dense_windows", "--window", "7"], r"--temp_pool gru\|lstm\|mean\|max"),
                      (["--dense_windows", "--window", "7", "--feats_model", "0006"], r"--temp_pool"),
                      (["--dense_windows", "--window", "1", "--temp_pool", "gru", "--feats_model", "0006"], r"--window")):
        with pytest.raises(SystemExit, match=why) as e:
            check_dense_windows(parse(argv))
        assert "--feats_model" not in str(e.value)                             # no longer a condition


def test_abi_surface_of_the_table_form():
    from tennis_amd import _lib
    header = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    declared = _lib.declared_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("tn_window_head_forward_rows", "tn_temporal_pool_rows"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in declared, name
        assert getattr(lib, name) is not None, name
    for site in ("evaluate.py:274-303", "dataset.py:190-201", "definitions.py:66-69", "definitions.py:104-109"):
        assert site in header, site
    # the existing entry points keep their signatures
    assert re.search(r"int tn_window_head_forward\(tn_window_head \*h, const int32_t \*centre, const int32_t \*lo, const int32_t \*hi, "
                     r"int samples,\s+int window, int stride, float \*pooled, float \*logits\);", header)
