"""-m gpu: evaluate --save_events --event_transitions train|FILE.npy on the tiny synthetic split of tests/test_gpu_save_events.py (2
videos of 20 frames, window 4, stored features 64 wide; the loader route and --dense_windows).  Three runs of the driver per route -
without the flags, with the train split's bigrams and with a matrix file that forbids transitions: the printed per-frame scores and
the returned dicts must not change, and each file must hold its matrix and the runs of events.viterbi_labels (float32, the kernel's
arithmetic) on the run's own logits under that matrix."""
import contextlib
import io
import os

import numpy as np
import pytest

from tools import events_ref as ER
from tools import transitions_ref as TR

pytestmark = pytest.mark.gpu

FRAMES, WINDOW, FEAT = 20, 4, 64
PRIOR, SCALE = 0.5, 2.0
ROUTES = {"loader": ["--feats_model", "0006"], "dense_features": ["--feats_model", "0006", "--dense_windows"]}


def _scores(out):
    """the confusion matrix and the [Finished] line without its time"""
    text = out[out.index("Test set:"):]
    return text[:text.index("Time Taken")]


def _dataset(root, split="test", **kw):
    from tennis_amd.dataset import TennisSet
    return TennisSet(root=root, window=WINDOW, stride=2, frames_per_video=FRAMES, data_shape=224, split=split, balance=False, **kw)


def _file_matrix(c):
    """multiples of 1/4 in [-2, 0] with a fifth of the off-diagonal entries forbidden"""
    rng = np.random.default_rng(3)
    t = (-rng.integers(0, 9, (c, c)) / 4.0).astype(np.float32)
    t[(rng.random((c, c)) < 0.2) & ~np.eye(c, dtype=bool)] = -np.inf
    return t


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """route -> per run of the driver what it printed, returned, decoded and wrote"""
    from tennis_amd import evaluate as ev
    base = tmp_path_factory.mktemp("save_events_transitions")
    root = str(base / "data")
    ds = _dataset(root, feats_model="0006")
    rng = np.random.default_rng(2)
    for v, f in ds.window_table()[0]:                                            # the stored features: 64 wide, one file per frame
        path = ds.get_feature_path(ds.feat_dir, v, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, (np.abs(rng.normal(0, 1, FEAT)) * 0.5).astype(np.float32))
    matrix_file = str(base / "grammar.npy")
    np.save(matrix_file, _file_matrix(len(ds.classes)))
    flags = {"plain": [], "train": ["--save_events", "--event_transitions", "train", "--event_transition_prior", str(PRIOR),
                                    "--event_transition_scale", str(SCALE)],
             "file": ["--save_events", "--event_transitions", matrix_file]}
    out = {}
    for route, extra in ROUTES.items():
        exp = str(base / ("exp_" + route))
        args = ["--root", root, "--frames_per_video", str(FRAMES), "--data_shape", "224", "--window", str(WINDOW), "--stride", "2",
                "--temp_pool", "gru", "--batch_size", "8", "--exp_root", exp] + extra
        file = os.path.join(exp, "0000", "test_events.npz")
        rec = dict(root=root)
        with pytest.MonkeyPatch.context() as mp:
            returned, decoded = [], []
            for name in ("evaluate_model", "evaluate_windows", "evaluate_table"):
                def wrapped(*a, _f=getattr(ev, name), **k):
                    r = _f(*a, **k)
                    returned.append(r)
                    return r
                mp.setattr(ev, name, wrapped)

            def decoding(dataset, logits, order=None, **k):
                decoded.append((logits.cpu().numpy().copy(), None if order is None else list(order), dict(k)))
                return ev_decode(dataset, logits, order, **k)
            ev_decode = ev.decode_split
            mp.setattr(ev, "decode_split", decoding)
            for name, flag in flags.items():
                del returned[:], decoded[:]
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    assert ev.main(args + flag) == 0
                cols = None
                if name == "plain":
                    assert not os.path.exists(file)
                else:
                    with np.load(file, allow_pickle=False) as z:
                        cols = {k: z[k] for k in z.files}
                assert len(returned) == 1
                rec[name] = dict(text=buf.getvalue(), returned=returned[0], decoded=list(decoded), cols=cols)
        out[route] = rec
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_matrix_changes_no_score_and_no_result(runs, route):
    rec = runs[route]
    assert _scores(rec["plain"]["text"]) == _scores(rec["train"]["text"]) == _scores(rec["file"]["text"])
    assert "Events:" not in rec["plain"]["text"] and "Event transitions" not in rec["plain"]["text"]
    for name, source in (("train", "label bigrams of the train split (prior 0.5, scale 2)"), ("file", "grammar.npy")):
        text = rec[name]["text"]
        line = [ln for ln in text.splitlines() if ln.startswith("Event transitions")]
        assert len(line) == 1 and source in line[0] and "smallest diagonal entry" in line[0] and "largest off-diagonal entry" in line[0]
        assert "(transition matrix)" in text
        (res_a, gt_a), (res_b, gt_b) = rec["plain"]["returned"][:2], rec[name]["returned"][:2]
        assert list(res_a) == list(res_b) and gt_a == gt_b and len(res_a) == 2 * FRAMES
        assert all(np.array_equal(res_a[k], res_b[k]) and res_a[k].dtype == res_b[k].dtype for k in res_a)


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_file_holds_its_matrix(runs, route):
    from tennis_amd.events import EVENT_COLUMNS, time_order, transition_scores
    rec = runs[route]
    for name in ("train", "file"):
        cols = rec[name]["cols"]
        assert set(cols) == set(EVENT_COLUMNS) | {"transitions"} and int(cols["smooth"]) == 1
        assert cols["transitions"].dtype == np.float32
        (_, _, kw), = rec[name]["decoded"]
        assert np.array_equal(kw["transitions"], cols["transitions"]) and "switch_cost" not in kw
    train = _dataset(rec["root"], split="train")                                 # labels only
    rows, start, _, _ = time_order(train)
    labels = [train.classes.index(train._samples[int(i)][2]) for i in rows]
    want = transition_scores(labels, start, len(train.classes), prior=PRIOR, scale=SCALE)
    assert np.array_equal(rec["train"]["cols"]["transitions"], want) and np.all(np.isfinite(want))
    assert np.array_equal(rec["file"]["cols"]["transitions"], _file_matrix(len(train.classes)))
    assert np.isneginf(rec["file"]["cols"]["transitions"]).any()


@pytest.mark.parametrize("name", ["train", "file"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_the_file_holds_the_runs_of_the_best_path_under_its_matrix(runs, route, name):
    from tennis_amd.events import label_runs, time_order, viterbi_labels
    rec = runs[route]
    (logits, order, kw), = rec[name]["decoded"]
    d = rec[name]["cols"]
    trans = d["transitions"]
    ds = _dataset(rec["root"], feats_model="0006")
    assert logits.dtype == np.float32 and logits.shape == (len(ds), len(ds.classes)) and sorted(order) == list(range(len(ds)))
    res = rec[name]["returned"][0]
    keys = [ds.get_image_path(ds._frames_dir, *ds._samples[i][:2]) for i in order]
    assert np.array_equal(logits, np.stack([res[k] for k in keys]))              # what was decoded is what the run returned
    rows, start, video, frame = time_order(ds, order)
    assert list(start.nonzero()[0]) == [0, FRAMES]
    label = viterbi_labels(logits, rows, start, dtype=np.float32, transitions=trans)
    e = TR.emissions(logits, rows)
    if name == "train":                                                          # (path_bound is derived for finite matrices)
        short = TR.optimum(e, start, trans) - TR.path_score(e, label, start, trans)
        assert -1e-9 <= short <= TR.path_bound(len(rows), np.abs(trans).max(), np.abs(e).max())
    assert TR.forbidden_pairs(label, start, trans) == 0
    first, last, cls = label_runs(label, start)
    assert np.array_equal(d["cls"], cls)
    assert list(d["video"]) == list(video[first]) and np.array_equal(d["first_frame"], frame[first]) and np.array_equal(d["last_frame"], frame[last])
    order = np.asarray(order)
    assert np.array_equal(d["first_sample"], order[rows[first]]) and np.array_equal(d["last_sample"], order[rows[last]])
    # score and peak: the unsmoothed probability of the path's label
    p = ER.decode_ref(logits, rows, start, 1)["p"]
    conf = p[np.arange(len(rows)), label]
    sb = ER.score_bound(logits.shape[1], 1)
    assert np.all(np.abs(d["peak"] - np.asarray([conf[a:b + 1].max() for a, b in zip(first, last)])) <= sb)
    assert np.all(np.abs(d["score"] - np.asarray([conf[a:b + 1].mean() for a, b in zip(first, last)]))
                  <= sb + np.asarray([ER.mean_bound(int(b - a + 1)) for a, b in zip(first, last)]))
    # the ground truth as without the matrix
    labels = np.asarray([ds.classes.index(ds._samples[i][2]) for i in order[rows]])
    gfirst, glast, gcls = label_runs(labels, start)
    assert np.array_equal(d["gt_cls"], gcls) and np.array_equal(d["gt_first_frame"], frame[gfirst]) and np.array_equal(d["gt_last_frame"], frame[glast])
