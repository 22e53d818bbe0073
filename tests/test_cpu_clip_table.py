"""``CaptionSet.clip_table`` / ``captions.load_clip_table`` / ``bucketed_batches(rows=...)``: a caption split as rows of one feature
table - what ``train_gnmt --feats_on_device`` uploads once - against the loader route (``__getitem__`` + ``pad_batchify``), on the
synthetic source and on a small on-disk tree with ragged, overlapping, out-of-order points.  No GPU."""
import numpy as np
import pytest

from tennis_amd import captions as cp
from tennis_amd.captions import CaptionSet
from tools import clip_tree

F = 20


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("clip_tree") / "data")
    return root, clip_tree.write(root, feature_dim=F)


def _sets(tree, every):
    root, _ = tree
    disk = lambda split, **kw: CaptionSet(split=split, every=every, root=root, feats_model="0042", **kw)
    train = disk("train")
    return [CaptionSet(split="train", every=every, n_points=9, feature_dim=12, mean_frames=10),
            CaptionSet(split="val", every=every, n_points=5, feature_dim=12, mean_frames=6, inference=True), train,
            disk("val", vocab=train.vocab, inference=True)]


def _count_loads(monkeypatch):
    opened, real = [], np.load

    def counting(path, *a, **k):
        opened.append(str(path))
        return real(path, *a, **k)

    monkeypatch.setattr(np, "load", counting)
    return opened


@pytest.mark.parametrize("every", [1, 3])
def test_clip_table_names_the_frames_each_item_stacks(tree, every):
    for ds in _sets(tree, every):
        frames, idx, lens = ds.clip_table()
        assert frames == sorted(set(frames)) and all(len(vf) == 2 for vf in frames)
        assert idx.dtype == np.int32 and idx.shape == (len(ds), max(lens)) and lens == ds.get_clip_lens()
        assert idx.max() == len(frames) - 1 and idx.min() == -1 and len(set(lens)) > 1, "ragged clips: some row is padded"
        used = set()
        for i in range(len(ds)):
            p = ds._points[ds._samples[i]]
            want = [(p[0], f) for c, f in enumerate(range(int(p[1]), int(p[2]))) if c % every == 0]     # __getitem__'s own selection
            assert lens[i] == len(want) == ds[i][2]
            assert [frames[r] for r in idx[i, :lens[i]]] == want
            assert (idx[i, lens[i]:] == -1).all() and (idx[i, :lens[i]] >= 0).all()
            used.update(want)
        assert used == set(frames), "the table holds exactly the frames some point reads"


def test_overlapping_points_share_rows(tree):
    ds = _sets(tree, 1)[2]
    frames, idx, lens = ds.clip_table()
    a, b = ds._samples.index("Ptrain03"), ds._samples.index("Ptrain04")
    shared = set(idx[a, :lens[a]]) & set(idx[b, :lens[b]])
    assert len(shared) == 3 and len(frames) < sum(lens)
    # the order of the points is free: the table stays, the rows of idx follow the points
    order = np.random.default_rng(1).permutation(len(ds))
    ds._samples = [ds._samples[i] for i in order]
    frames2, idx2, lens2 = ds.clip_table()
    assert frames2 == frames and np.array_equal(idx2, idx[order]) and lens2 == [lens[i] for i in order]


@pytest.mark.parametrize("every", [1, 3])
def test_load_clip_table_rows_are_the_stacked_items_and_each_file_is_read_once(tree, every, monkeypatch):
    for ds in _sets(tree, every):
        frames, idx, lens = ds.clip_table()
        opened = _count_loads(monkeypatch)
        table = cp.load_clip_table(ds, frames)
        monkeypatch.undo()
        if ds._feat_dir is not None:
            want = sorted(ds._feat_path(ds._feat_dir, v, f) for v, f in frames)
            assert sorted(opened) == want and len(set(opened)) == len(opened), "every file of the table exactly once, and no other"
        else:
            assert opened == []
        assert table.dtype == np.float32 and table.shape == (len(frames), ds[0][0].shape[1])
        for i in range(len(ds)):
            assert np.array_equal(table[idx[i, :lens[i]]], ds[i][0])


def test_load_feature_table_still_reads_through_the_shared_pool(tmp_path):
    """the head's table loader now shares ``read_rows`` with the clip table: same rows, same dtype, same refusal of an empty list"""
    import os
    from tennis_amd import evaluate as ev
    from tennis_amd.dataset import TennisSet
    ds = TennisSet(root=str(tmp_path), videos=("A",), frames_per_video=9, window=3, feats_model="0001", synthetic=True)
    frames, _ = ds.window_table()
    for r, (v, f) in enumerate(frames):
        path = ds.get_feature_path(ds.feat_dir, v, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, np.full((1, 5), r, np.float64))              # another dtype and shape on disk: flattened, cast to float32
    table = ev.load_feature_table(ds, frames)
    assert table.dtype == np.float32 and np.array_equal(table, np.arange(len(frames), dtype=np.float32)[:, None].repeat(5, 1))
    with pytest.raises(ValueError):
        ev.load_feature_table(ds, [])
    with pytest.raises(ValueError):
        cp.load_clip_table(ds, [])


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("world", [1, 2])
def test_bucketed_batches_by_rows_yields_the_loader_routes_batches(tree, shuffle, world, monkeypatch):
    several = 0
    for every in (1, 3):
        for ds in _sets(tree, every):
            frames, idx, lens = ds.clip_table()
            table = cp.load_clip_table(ds, frames)
            padded = np.concatenate([table, np.zeros((1, table.shape[1]), np.float32)])        # row -1: the zero row
            for rank in range(world):
                kw = dict(batch_size=3, num_buckets=2, shuffle=shuffle, seed=4, epoch=1, rank=rank, world=world)
                want = list(cp.bucketed_batches(ds, **kw))
                opened = _count_loads(monkeypatch)
                monkeypatch.setattr(type(ds), "__getitem__", lambda *a: pytest.fail("the rows route reads no item"))
                got = list(cp.bucketed_batches(ds, rows=idx, **kw))
                monkeypatch.undo()
                assert opened == [] and len(got) == len(want) >= 1
                several += len(got) > 1
                for g, w in zip(got, want):
                    assert len(g) == len(w) == (5 if ds._inference else 4)
                    assert g[0].dtype == np.int32 and g[0].shape == w[0].shape[:2]
                    for a, b in zip(g[1:], w[1:]):                                              # targets, lengths, (ids)
                        assert a.dtype == b.dtype and np.array_equal(a, b)
                    assert np.array_equal(padded[g[0]], w[0]), "the zero-padded gather is pad_batchify's source"
                    assert g[0].shape[1] == int(g[2].max()), "padded to the batch's longest clip, not the split's"
    assert several >= 4, "most sets yield more than one batch"


def test_feats_on_device_flag_default_off_and_frame_mode_refusal():
    from tennis_amd.train_gnmt import build_parser, require_feature_mode
    assert build_parser().parse_args([]).feats_on_device is False
    require_feature_mode(build_parser().parse_args(["--feats_model", "0042", "--data_root", "d", "--feats_on_device"]))
    require_feature_mode(build_parser().parse_args(["--feats_on_device"]))               # synthetic features: feature mode
    require_feature_mode(build_parser().parse_args(["--data_root", "d"]))               # without the flag nothing is checked
    for argv in (["--data_root", "d", "--feats_on_device"], ["--frames", "--feats_on_device"]):
        with pytest.raises(SystemExit, match="--feats_model"):
            require_feature_mode(build_parser().parse_args(argv))


def test_clip_table_is_a_feature_mode_call():
    ds = CaptionSet(split="train", n_points=3, frames=True, data_shape=32, mean_frames=5)
    with pytest.raises(ValueError, match="feature mode"):
        ds.clip_table()
