"""-m gpu: evaluate --save_events --event_switch_cost 2.0 on the tiny synthetic split of tests/test_gpu_save_events.py (2 videos of 20
frames, window 4, stored features 64 wide; the loader route and --dense_windows).  Three runs of the driver per route - without the
flags, with --save_events alone and with the switch cost: the printed per-frame scores and the returned dicts must not change, the
file of the last run must hold the runs of events.viterbi_labels on the run's own logits, and the file of the run without the cost
must have exactly the columns it had."""
import contextlib
import io
import os

import numpy as np
import pytest

from tools import events_ref as ER
from tools import viterbi_ref as VR

pytestmark = pytest.mark.gpu

FRAMES, WINDOW, FEAT = 20, 4, 64
COST = 2.0
ROUTES = {"loader": ["--feats_model", "0006"], "dense_features": ["--feats_model", "0006", "--dense_windows"]}
FLAGS = {"plain": [], "events": ["--save_events"], "path": ["--save_events", "--event_switch_cost", str(COST)]}


def _scores(out):
    """the confusion matrix and the [Finished] line without its time"""
    text = out[out.index("Test set:"):]
    return text[:text.index("Time Taken")]


def _dataset(root):
    from tennis_amd.dataset import TennisSet
    return TennisSet(root=root, window=WINDOW, stride=2, frames_per_video=FRAMES, data_shape=224, split="test", balance=False,
                     feats_model="0006")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """route -> per run of the driver what it printed, returned, decoded and wrote"""
    from tennis_amd import evaluate as ev
    base = tmp_path_factory.mktemp("save_events_viterbi")
    root = str(base / "data")
    ds = _dataset(root)
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
            for name, flag in FLAGS.items():
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
def test_the_switch_cost_changes_no_score_and_no_result(runs, route):
    rec = runs[route]
    assert _scores(rec["plain"]["text"]) == _scores(rec["events"]["text"]) == _scores(rec["path"]["text"])
    assert "switch cost 2" in rec["path"]["text"] and "smooth 1" in rec["events"]["text"] and "Events:" not in rec["plain"]["text"]
    (res_a, gt_a), (res_b, gt_b) = rec["plain"]["returned"][:2], rec["path"]["returned"][:2]
    assert list(res_a) == list(res_b) and gt_a == gt_b and len(res_a) == 2 * FRAMES
    assert all(np.array_equal(res_a[k], res_b[k]) and res_a[k].dtype == res_b[k].dtype for k in res_a)


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_columns_without_the_cost_are_the_columns_of_before(runs, route):
    from tennis_amd.events import EVENT_COLUMNS
    rec = runs[route]
    assert set(rec["events"]["cols"]) == set(EVENT_COLUMNS) and "switch_cost" not in EVENT_COLUMNS
    assert set(rec["path"]["cols"]) == set(EVENT_COLUMNS) | {"switch_cost"}
    assert float(rec["path"]["cols"]["switch_cost"]) == COST and int(rec["path"]["cols"]["smooth"]) == 1
    (_, _, kw_events), (_, _, kw_path) = rec["events"]["decoded"][0], rec["path"]["decoded"][0]
    assert "switch_cost" not in kw_events and kw_path["switch_cost"] == COST     # without the flag the call is the call it was


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_file_holds_the_runs_of_the_best_path_through_the_runs_own_logits(runs, route):
    from tennis_amd.events import label_runs, load_events, time_order, viterbi_labels
    from tennis_amd.metrics.events import EventPRF1
    rec = runs[route]
    assert len(rec["path"]["decoded"]) == 1
    logits, order, kw = rec["path"]["decoded"][0]
    d = rec["path"]["cols"]
    ds = _dataset(rec["root"])
    assert logits.shape == (len(ds), len(ds.classes)) and sorted(order) == list(range(len(ds)))
    res = rec["path"]["returned"][0]
    keys = [ds.get_image_path(ds._frames_dir, *ds._samples[i][:2]) for i in order]
    assert np.array_equal(logits, np.stack([res[k] for k in keys]))              # what was decoded is what the run returned
    rows, start, video, frame = time_order(ds, order)
    assert list(start.nonzero()[0]) == [0, FRAMES]
    label = viterbi_labels(logits, rows, start, COST)
    # these logits are no dyadic numbers, so fp32 may legitimately pick another path of (nearly) the same score than float64 does:
    # the comparison below needs inputs on which the float32 run of the definition agrees with the float64 run (a condition on the
    # inputs, asserted here), and the reference's path must be the optimum
    assert np.array_equal(label, viterbi_labels(logits, rows, start, COST, dtype=np.float32))
    e = VR.emissions(logits, rows)
    best = VR.path_score(e, label, start, COST)
    assert abs(best - VR.optimum(e, start, COST)) < 1e-9
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
    # fewer or as many events as the per-frame arg-max of the same logits finds
    assert len(cls) <= len(rec["events"]["cols"]["cls"])
    # the ground truth and the scores as without the cost
    labels = np.asarray([ds.classes.index(ds._samples[i][2]) for i in order[rows]])
    gfirst, glast, gcls = label_runs(labels, start)
    assert np.array_equal(d["gt_cls"], gcls) and np.array_equal(d["gt_first_frame"], frame[gfirst]) and np.array_equal(d["gt_last_frame"], frame[glast])
    m = EventPRF1(ds.classes)
    m.update({k: d[k] for k in ("video", "first_frame", "last_frame", "cls", "score")},
             dict(video=d["gt_video"], first_frame=d["gt_first_frame"], last_frame=d["gt_last_frame"], cls=d["gt_cls"]))
    prec, rec_, f1 = m.arrays()
    assert np.array_equal(d["precision"], prec) and np.array_equal(d["recall"], rec_) and np.array_equal(d["f1"], f1)
