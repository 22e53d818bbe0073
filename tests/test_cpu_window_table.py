"""``TennisSet.window_table``: every sample's window as rows of a feature table that assumes nothing about the sample list
(thinned out, gapped, windows reaching frames that are no sample), against ``window_frames`` (reference dataset.py:190-201);
``evaluate.load_feature_table`` reading every file once; and the ``train --dense_windows`` flag's refusals.  No GPU."""
import os
import random

import numpy as np
import pytest

from tennis_amd.dataset import TennisSet


def _table_names_the_window_frames(ds, stride=None):
    frames, idx = ds.window_table(stride)
    assert idx.dtype == np.int32 and idx.shape == (len(ds), ds._window)
    assert frames == sorted(set(frames)), "frames must be sorted and free of duplicates"
    assert idx.min() >= 0 and idx.max() < len(frames)
    used = set()
    for i, sample in enumerate(ds._samples):
        want = [(sample[0], f) for f in ds.window_frames(sample, stride)]
        assert [frames[r] for r in idx[i]] == want, (i, sample)
        used.update(want)
    assert used == set(frames), "the table holds exactly the frames some window reads"
    return frames, idx


@pytest.mark.parametrize("window", [2, 7, 8])
@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("stride", [1, 3])
def test_window_table_names_the_window_frames(window, every, stride):
    # 1 and 5 frames: shorter than most windows, so both ends clamp inside one window; 17: windows clamped at either end only
    for n in (1, 5, 17):
        ds = TennisSet(videos=("A", "B", "C"), frames_per_video=n, every=every, window=window, stride=stride, synthetic=True)
        frames, idx = _table_names_the_window_frames(ds)
        # clamped at both video ends: the first sample's window starts at frame 0, the last one's ends at the video's last window frame
        # (or, where the video is longer than the window, at the frame the last offset names)
        if n <= every:        # (a video shorter than `every`: the reference's max_frame is negative and every window reads it)
            continue
        assert frames[idx[0, 0]] == ("A", 0)
        assert frames[idx[-1, -1]] == ("C", min(ds._samples[-1][1] + (-(-window // 2) - 1) * stride, ds._max_frame("C")))


def test_window_table_stride_argument_overrides_the_datasets():
    ds = TennisSet(videos=("A", "B"), frames_per_video=20, window=7, stride=1, synthetic=True)
    _, idx1 = _table_names_the_window_frames(ds)
    _, idx3 = _table_names_the_window_frames(ds, stride=3)
    assert ds._stride == 1 and not np.array_equal(idx1, idx3)


@pytest.mark.parametrize("every,stride,window", [(1, 1, 7), (2, 3, 8), (1, 3, 2)])
def test_window_table_thinned_out_sample_list(every, stride, window):
    """what ``_balance_classes`` leaves: a random subset, whose windows read frames that are no sample any more"""
    ds = TennisSet(videos=("A", "B", "C"), frames_per_video=17, every=every, window=window, stride=stride, synthetic=True)
    rnd = random.Random(5)
    ds._samples = [s for s in ds._samples if rnd.uniform(0, 1) < 0.4]
    assert 0 < len(ds) < 3 * 17
    frames, _ = _table_names_the_window_frames(ds)
    assert set(frames) - {(s[0], s[1]) for s in ds._samples}, "some window frame is not a sample: the case window_rows refuses"
    with pytest.raises(ValueError):
        ds.window_rows()


def test_window_table_gap_in_the_middle_of_a_video_and_any_order():
    """split_id 02: a video's samples lie in separate sections; the windows next to the gap read frames inside it"""
    ds = TennisSet(videos=("A", "B"), frames_per_video=17, window=7, synthetic=True)
    ds._samples = [s for s in ds._samples if not (s[0] == "A" and 6 <= s[1] <= 11)]
    frames, idx = _table_names_the_window_frames(ds)
    assert ("A", 8) in frames and ["A", 8] not in [s[:2] for s in ds._samples]
    with pytest.raises(ValueError):
        ds.window_rows()
    # the order of the samples is free too: the table is the same, the rows of idx follow the samples
    order = np.random.default_rng(2).permutation(len(ds))
    ds._samples = [ds._samples[i] for i in order]
    frames2, idx2 = _table_names_the_window_frames(ds)
    assert frames2 == frames and np.array_equal(idx2, idx[order])


def test_window_table_split_inside_a_longer_video():
    """windows reach frames before and behind the split's range: no sample of the split, but frames of the video"""
    ds = TennisSet(videos=("A",), frames_per_video=12, split_first=20, video_length=60, window=7, synthetic=True)
    frames, _ = _table_names_the_window_frames(ds)
    assert frames[0] == ("A", 17) and frames[-1] == ("A", 34)


@pytest.mark.parametrize("window", [2, 7, 8])
@pytest.mark.parametrize("every,stride", [(1, 1), (1, 3), (2, 2), (2, 6)])
def test_window_table_agrees_with_window_rows_where_those_exist(window, every, stride):
    compared = 0
    for n in (1, 5, 17):
        ds = TennisSet(videos=("A", "B", "C"), frames_per_video=n, every=every, window=window, stride=stride, synthetic=True)
        try:
            centre, lo, hi, row_stride = ds.window_rows()
        except ValueError:      # (a video shorter than `every`: the reference's max_frame is negative, a frame with no row)
            assert n < every
            continue
        compared += 1
        frames, idx = ds.window_table()
        t = np.arange(window)
        for i in range(len(ds)):
            rows = np.clip(int(centre[i]) + (t - window // 2) * row_stride, int(lo[i]), int(hi[i]))
            assert [tuple(ds._samples[r][:2]) for r in rows] == [frames[r] for r in idx[i]]
    assert compared >= 2


def test_window_table_needs_a_window():
    with pytest.raises(ValueError, match="window > 1"):
        TennisSet(videos=("A",), frames_per_video=5, window=1, synthetic=True).window_table()


def test_load_feature_table_reads_every_file_once(tmp_path, monkeypatch):
    from tennis_amd import evaluate as ev
    assert 1 <= ev.TABLE_LOAD_THREADS <= 16
    F = 6
    ds = TennisSet(root=str(tmp_path), videos=("A", "B"), frames_per_video=17, window=7, stride=3, feats_model="0001", synthetic=True)
    rnd = random.Random(1)
    ds._samples = [s for s in ds._samples if rnd.uniform(0, 1) < 0.5]
    frames, idx = ds.window_table()
    want = {}
    for r, (v, f) in enumerate(frames):
        path = ds.get_feature_path(ds.feat_dir, v, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        want[path] = np.random.default_rng(r).normal(0, 1, F).astype(np.float32)
        np.save(path, want[path])
    opened = []
    real_load = np.load

    def counting_load(path, *a, **k):
        opened.append(str(path))
        return real_load(path, *a, **k)

    monkeypatch.setattr(np, "load", counting_load)
    table = ev.load_feature_table(ds, frames)
    monkeypatch.undo()
    assert sorted(opened) == sorted(want), "every file of the table exactly once, and no other"
    assert table.dtype == np.float32 and table.shape == (len(frames), F)
    for r, (v, f) in enumerate(frames):
        assert np.array_equal(table[r], want[ds.get_feature_path(ds.feat_dir, v, f)])
    # the table gathered by idx is the batch the loader stacks for the same samples
    for i in (0, len(ds) // 2, len(ds) - 1):
        assert np.array_equal(table[idx[i]], ds[i][0])


def test_dense_windows_flag_default_off_and_refusals():
    from tennis_amd.train import build_parser, check_dense_windows
    assert build_parser().parse_args([]).dense_windows is False
    ok = ["--feats_model", "0001", "--window", "4", "--temp_pool", "gru", "--dense_windows"]
    check_dense_windows(build_parser().parse_args(ok))
    check_dense_windows(build_parser().parse_args(["--window", "1"]))          # without the flag nothing is checked
    for argv, why in ((["--window", "4", "--temp_pool", "gru", "--dense_windows"], "--feats_model"),
                      (["--feats_model", "0001", "--window", "1", "--temp_pool", "gru", "--dense_windows"], "--window > 1"),
                      (["--feats_model", "0001", "--window", "4", "--temp_pool", "mean", "--dense_windows"], "gru\\|lstm"),
                      (["--feats_model", "0001", "--window", "4", "--temp_pool", "max", "--dense_windows"], "gru\\|lstm")):
        with pytest.raises(SystemExit, match=why):
            check_dense_windows(build_parser().parse_args(argv))
