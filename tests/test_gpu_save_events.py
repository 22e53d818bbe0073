"""-m gpu: evaluate --save_events on a tiny synthetic split (2 videos of 20 frames, window 4) through the three routes that yield
per-sample logits for a windowed model - the loader route and --dense_windows over stored features (64 wide), and --dense_windows on
frames.  Every route runs once without and once with the flag: the printed per-frame scores and the returned dicts must not change,
the file must hold the events of tests/tools/events_ref.py applied to the run's own logits and the runs of the split's labels."""
import contextlib
import io
import os

import numpy as np
import pytest

from tools import events_ref as ER

pytestmark = pytest.mark.gpu

FRAMES, WINDOW, FEAT = 20, 4, 64
SMOOTH = 3
ROUTES = {"loader": ["--feats_model", "0006"], "dense_features": ["--feats_model", "0006", "--dense_windows"],
          "dense_frames": ["--dense_windows"]}


def _scores(out):
    """the confusion matrix and the [Finished] line without its time"""
    text = out[out.index("Test set:"):]
    return text[:text.index("Time Taken")]


def _dataset(root, feats):
    from tennis_amd.dataset import TennisSet
    return TennisSet(root=root, window=WINDOW, stride=2, frames_per_video=FRAMES, data_shape=224, split="test", balance=False,
                     feats_model="0006" if feats else None)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """route -> what the two runs of the driver printed, returned and decoded"""
    from tennis_amd import evaluate as ev
    base = tmp_path_factory.mktemp("save_events")
    root = str(base / "data")
    ds = _dataset(root, True)
    rng = np.random.default_rng(2)
    for v, f in ds.window_table()[0]:                                            # the stored features: 64 wide, one file per frame
        path = ds.get_feature_path(ds.feat_dir, v, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, (np.abs(rng.normal(0, 1, FEAT)) * 0.5).astype(np.float32))
    out = {}
    for route, extra in ROUTES.items():
        exp = str(base / ("exp_" + route))
        args = ["--root", root, "--frames_per_video", str(FRAMES), "--data_shape", "224", "--window", str(WINDOW), "--stride", "2",
                "--temp_pool", "gru", "--batch_size", "8", "--exp_root", exp] + extra
        rec = dict(root=root, returned=[], decoded=[], file=os.path.join(exp, "0000", "test_events.npz"))
        with pytest.MonkeyPatch.context() as mp:
            for name in ("evaluate_model", "evaluate_windows", "evaluate_table"):
                def wrapped(*a, _f=getattr(ev, name), **k):
                    r = _f(*a, **k)
                    rec["returned"].append(r)
                    return r
                mp.setattr(ev, name, wrapped)

            def decoding(dataset, logits, order=None, **k):
                rec["decoded"].append((logits.cpu().numpy().copy(), None if order is None else list(order), dict(k)))
                return ev_decode(dataset, logits, order, **k)
            ev_decode = ev.decode_split
            mp.setattr(ev, "decode_split", decoding)
            texts = []
            for flag in ([], ["--save_events", "--event_smooth", str(SMOOTH)]):
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    assert ev.main(args + flag) == 0
                texts.append(buf.getvalue())
                if not flag:
                    assert not os.path.exists(rec["file"])
        rec["plain"], rec["flagged"] = texts
        out[route] = rec
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_flag_changes_no_score_and_no_result(runs, route):
    rec = runs[route]
    assert _scores(rec["plain"]) == _scores(rec["flagged"])                      # the confusion matrix and every printed per-frame score
    assert "Events:" not in rec["plain"] and "Events:" in rec["flagged"] and "Saved" in rec["flagged"] and "[Events] AVG_prec@0.1" in rec["flagged"]
    assert len(rec["returned"]) == 2 and len(rec["decoded"]) == 1
    (res_a, gt_a), (res_b, gt_b) = (r[:2] for r in rec["returned"])
    assert list(res_a) == list(res_b) and gt_a == gt_b and len(res_a) == 2 * FRAMES
    assert all(np.array_equal(res_a[k], res_b[k]) and res_a[k].dtype == res_b[k].dtype for k in res_a)


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_file_holds_the_events_of_the_runs_own_logits(runs, route):
    from tennis_amd.events import EVENT_COLUMNS, label_runs, load_events, time_order
    from tennis_amd.metrics.events import EventPRF1
    rec = runs[route]
    with np.load(rec["file"], allow_pickle=False) as z:
        assert set(z.files) == set(EVENT_COLUMNS)
    d = load_events(rec["file"])
    logits, order, kw = rec["decoded"][0]
    assert kw.get("smooth") == SMOOTH and int(d["smooth"]) == SMOOTH
    ds = _dataset(rec["root"], route != "dense_frames")
    assert logits.shape == (len(ds), len(ds.classes)) and sorted(order) == list(range(len(ds)))
    res = rec["returned"][1][0]
    keys = [ds.get_image_path(ds._frames_dir, *ds._samples[i][:2]) for i in order]
    assert np.array_equal(logits, np.stack([res[k] for k in keys]))              # what was decoded is what the run returned
    rows, start, video, frame = time_order(ds, order)
    assert list(start.nonzero()[0]) == [0, FRAMES] and list(frame) == list(range(FRAMES)) * 2
    ref = ER.decode_ref(logits, rows, start, SMOOTH)
    assert ref["margin"].min() > 2 * ER.score_bound(logits.shape[1], SMOOTH)     # (no label of this run is too close to call)
    assert np.array_equal(d["cls"], ref["cls"])
    assert list(d["video"]) == list(video[ref["first"]]) and np.array_equal(d["first_frame"], frame[ref["first"]])
    assert np.array_equal(d["last_frame"], frame[ref["last"]])
    order = np.asarray(order)
    assert np.array_equal(d["first_sample"], order[rows[ref["first"]]]) and np.array_equal(d["last_sample"], order[rows[ref["last"]]])
    length = ref["last"] - ref["first"] + 1
    sb = ER.score_bound(logits.shape[1], SMOOTH)
    assert np.all(np.abs(d["peak"] - ref["ev_peak"]) <= sb)
    assert np.all(np.abs(d["score"] - ref["ev_score"]) <= sb + np.asarray([ER.mean_bound(int(n)) for n in length]))
    # the ground truth: the runs of the split's labels in time order
    labels = np.asarray([ds.classes.index(ds._samples[i][2]) for i in order[rows]])
    gfirst, glast, gcls = label_runs(labels, start)
    assert np.array_equal(d["gt_cls"], gcls) and np.array_equal(d["gt_first_frame"], frame[gfirst]) and np.array_equal(d["gt_last_frame"], frame[glast])
    assert list(d["gt_video"]) == list(video[gfirst]) and len(gcls) > 2
    # and the scores are EventPRF1 of the two
    m = EventPRF1(ds.classes)
    m.update({k: d[k] for k in ("video", "first_frame", "last_frame", "cls", "score")},
             dict(video=d["gt_video"], first_frame=d["gt_first_frame"], last_frame=d["gt_last_frame"], cls=d["gt_cls"]))
    prec, rec_, f1 = m.arrays()
    assert np.array_equal(d["tiou"], [0.1, 0.3, 0.5]) and d["precision"].shape == (3, len(ds.classes))
    assert np.array_equal(d["precision"], prec) and np.array_equal(d["recall"], rec_) and np.array_equal(d["f1"], f1)
    assert (m.tp + m.fn).sum(1).tolist() == [len(gcls)] * 3 and (m.tp + m.fp).sum(1).tolist() == [len(d["cls"])] * 3


def test_the_routes_agree_on_the_events_where_their_labels_agree(runs):
    from tennis_amd.events import load_events, time_order
    per_route = {}
    for route, rec in runs.items():
        logits, order, _ = rec["decoded"][0]
        ds = _dataset(rec["root"], route != "dense_frames")
        rows, start, _, _ = time_order(ds, order)
        per_route[route] = (ER.decode_ref(logits, rows, start, SMOOTH)["label"], load_events(rec["file"]))
    names = list(per_route)
    compared = 0
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (la, da), (lb, db) = per_route[a], per_route[b]
            if np.array_equal(la, lb):
                compared += 1
                for k in ("video", "first_frame", "last_frame", "cls", "first_sample", "last_sample"):
                    assert np.array_equal(da[k], db[k]), (a, b, k)
            for k in ("gt_video", "gt_first_frame", "gt_last_frame", "gt_cls"):      # the ground truth is the split's, whatever the route
                assert np.array_equal(da[k], db[k]), (a, b, k)
    assert compared >= 1, "the loader route and the dense route over the same stored features evaluate the same model"
