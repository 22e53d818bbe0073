"""``TennisSet.window_rows``: every sample's window in units of rows of the dataset-order feature matrix, against
``window_frames`` (reference dataset.py:190-201), and the ``--dense_windows`` flag.  No GPU."""
import numpy as np
import pytest

from tennis_amd.dataset import TennisSet
from tennis_amd.evaluate import build_parser


def _rows_name_the_window_frames(ds, stride=None):
    centre, lo, hi, row_stride = ds.window_rows(stride)
    assert centre.dtype == lo.dtype == hi.dtype == np.int32 and len(centre) == len(lo) == len(hi) == len(ds)
    frame_of_row = [s[1] for s in ds._samples]
    video_of_row = [s[0] for s in ds._samples]
    t = np.arange(ds._window)
    for i, sample in enumerate(ds._samples):
        rows = np.clip(int(centre[i]) + (t - ds._window // 2) * row_stride, int(lo[i]), int(hi[i]))
        assert [frame_of_row[r] for r in rows] == ds.window_frames(sample, stride), (i, sample)
        assert {video_of_row[r] for r in rows} == {sample[0]}
    return row_stride


@pytest.mark.parametrize("window", [2, 7, 8, 30])
@pytest.mark.parametrize("every,stride", [(1, 1), (1, 2), (1, 3), (2, 2), (2, 4), (2, 6)])
def test_window_rows_name_the_window_frames(window, every, stride):
    # 5 frames / every: shorter than every window but 2; three videos, so lo / hi differ per sample
    for frames in (5, 40, 17):
        ds = TennisSet(videos=("A", "B", "C"), frames_per_video=frames, every=every, window=window, stride=stride, synthetic=True)
        assert _rows_name_the_window_frames(ds) == stride // every


def test_window_rows_stride_argument_overrides_the_datasets():
    ds = TennisSet(videos=("A", "B"), frames_per_video=20, window=7, stride=1, synthetic=True)
    assert _rows_name_the_window_frames(ds, stride=3) == 3
    assert ds._stride == 1


def test_window_rows_one_row_videos():
    ds = TennisSet(videos=("A", "B"), frames_per_video=1, window=8, stride=1, synthetic=True)
    centre, lo, hi, _ = ds.window_rows()
    assert list(centre) == [0, 1] and list(lo) == [0, 1] and list(hi) == [0, 1]
    _rows_name_the_window_frames(ds)


def test_window_rows_save_feats_padding():
    # the split covers the whole video: save_feats adds no padding frame that exists, rows stay one run per video
    ds = TennisSet(videos=("A", "B"), frames_per_video=12, window=8, save_feats=True, synthetic=True)
    assert len(ds) == 24
    _rows_name_the_window_frames(ds)
    # the split sits inside a longer video: the +-255 'OTH' frames are appended behind all videos, min-1, max+1, min-2, ... -
    # the rows of a video are then neither contiguous nor ascending, and there is no (centre, lo, hi) for them
    ds = TennisSet(videos=("A", "B"), frames_per_video=12, split_first=20, video_length=60, window=8, save_feats=True, synthetic=True)
    assert len(ds) > 24
    with pytest.raises(ValueError, match="not contiguous"):
        ds.window_rows()


def test_window_rows_illegal_combinations_raise():
    with pytest.raises(ValueError, match="multiple of every"):
        TennisSet(videos=("A",), frames_per_video=12, every=2, window=7, stride=3, synthetic=True).window_rows()
    with pytest.raises(ValueError, match="multiple of every"):
        TennisSet(videos=("A",), frames_per_video=12, every=2, window=7, stride=2, synthetic=True).window_rows(stride=1)
    # a window frame with no row: the split starts at frame 20 of the video, the first windows reach frames 17..19 (>= 0: not clamped)
    ds = TennisSet(videos=("A",), frames_per_video=12, split_first=20, video_length=60, window=7, synthetic=True)
    with pytest.raises(ValueError, match="has no row"):
        ds.window_rows()
    # ... and past the end: the video goes on behind the split's last frame
    ds = TennisSet(videos=("A",), frames_per_video=12, split_first=0, video_length=60, window=7, synthetic=True)
    with pytest.raises(ValueError, match="has no row"):
        ds.window_rows()
    # window 1 reaches nowhere: the same set maps
    ds = TennisSet(videos=("A",), frames_per_video=12, split_first=20, video_length=60, window=1, synthetic=True)
    _rows_name_the_window_frames(ds)
    # rows of one video that are not equally spaced / not contiguous in dataset order
    ds = TennisSet(videos=("A", "B"), frames_per_video=12, window=7, synthetic=True)
    del ds._samples[3]
    with pytest.raises(ValueError, match="equally spaced"):
        ds.window_rows()
    ds = TennisSet(videos=("A", "B"), frames_per_video=12, window=7, synthetic=True)
    ds._samples.append(ds._samples.pop(2))
    with pytest.raises(ValueError, match="not contiguous"):
        ds.window_rows()


def test_parser_has_dense_windows_default_off():
    assert build_parser().parse_args([]).dense_windows is False
    assert build_parser().parse_args(["--dense_windows"]).dense_windows is True
