"""No GPU: the event decoder's float64 reference (tests/tools/events_ref.py) on handmade cases, the host side of --save_events
(events.time_order / label_runs / save_events / load_events, metrics.events.EventPRF1), the flag's refusals and the ABI surface."""
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import events_ref as ER


def _onehot(labels, c, scale=8.0):
    x = np.zeros((len(labels), c))
    x[np.arange(len(labels)), labels] = scale
    return x


def test_events_ref_on_handmade_cases():
    # softmax and the first arg-max
    r = ER.decode_ref(np.log(np.array([[1.0, 3.0], [2.0, 2.0]])), [0, 1], [1, 0], 1)
    assert np.allclose(r["p"], [[0.25, 0.75], [0.5, 0.5]]) and list(r["label"]) == [1, 0]          # a tie goes to the smaller class
    assert np.allclose(r["margin"], [0.5, 0.0]) and np.allclose(r["conf"], [0.75, 0.5])
    assert list(r["first"]) == [0, 1] and list(r["last"]) == [0, 1] and list(r["cls"]) == [1, 0]
    # the window is cut at video boundaries and at both ends, and its mean divides by what is left
    lab = [0, 0, 1, 1, 1, 0]
    r = ER.decode_ref(_onehot(lab, 2), np.arange(6), [1, 0, 0, 1, 0, 0], 3)
    assert list(r["lo"]) == [0, 0, 1, 3, 3, 4] and list(r["hi"]) == [1, 2, 2, 4, 5, 5]
    p = r["p"]
    assert np.allclose(r["score"][2], (p[1] + p[2]) / 2) and np.allclose(r["score"][3], (p[3] + p[4]) / 2)
    assert np.allclose(r["score"][4], (p[3] + p[4] + p[5]) / 3)
    # two videos with one label meeting at a boundary are two events; the mean and the peak of an event
    r = ER.decode_ref(_onehot([1, 1, 1, 1], 3), np.arange(4), [1, 0, 1, 0], 1)
    assert list(r["first"]) == [0, 2] and list(r["last"]) == [1, 3] and list(r["cls"]) == [1, 1]
    assert np.allclose(r["ev_score"], r["conf"][0]) and np.allclose(r["ev_peak"], r["conf"][0])
    # rows select, permute and are clamped
    x = _onehot([0, 1, 2], 3)
    r = ER.decode_ref(x, [2, -5, 99, 1], [0, 0, 0, 0], 1)
    assert list(r["label"]) == [2, 0, 2, 1] and list(r["first"]) == [0, 1, 2, 3]
    # one class: every position is class 0, one event per video
    r = ER.decode_ref(np.zeros((5, 1)), np.arange(5), [1, 0, 0, 1, 0], 9)
    assert list(r["first"]) == [0, 3] and np.all(r["conf"] == 1.0) and np.all(np.isinf(r["margin"]))
    # the direct sum and the running-sum form of the window agree
    rng = np.random.default_rng(0)
    x = rng.normal(0, 2, (300, 5))
    st = (rng.random(300) < 0.05).astype(int)
    a = ER.decode_ref(x, np.arange(300), st, 9)
    h = 4
    for m in (0, 7, 150, 299):
        assert a["lo"][m] >= max(0, m - h) and a["hi"][m] <= min(299, m + h)
        assert not np.any(st[a["lo"][m] + 1:a["hi"][m] + 1])                     # no boundary inside a window
        assert np.allclose(a["score"][m], a["p"][a["lo"][m]:a["hi"][m] + 1].mean(0))
    assert ER.score_bound(11, 9) == 28 * 2.0 ** -24 and ER.mean_bound(65) == 9 * 2.0 ** -24


def _fake_set(samples, classes=("OTH", "SERVE", "HIT")):
    return types.SimpleNamespace(_samples=[list(s) for s in samples], classes=list(classes))


def test_time_order_on_unsorted_and_thinned_samples():
    from tennis_amd.events import time_order
    ds = _fake_set([("V2", 4, "OTH"), ("V1", 10, "HIT"), ("V1", 2, "OTH"), ("V2", 0, "SERVE"), ("V1", 7, "HIT")])
    rows, start, video, frame = time_order(ds)
    assert rows.dtype == np.int32 and start.dtype == np.int32
    assert list(rows) == [2, 4, 1, 3, 0] and list(start) == [1, 0, 0, 1, 0]
    assert list(video) == ["V1", "V1", "V1", "V2", "V2"] and list(frame) == [2, 7, 10, 0, 4]
    # order: logits row r belongs to sample order[r] (a loader that skipped sample 3 and shuffled)
    rows, start, video, frame = time_order(ds, order=[4, 0, 2, 1])
    assert list(rows) == [2, 0, 3, 1] and list(start) == [1, 0, 0, 1]
    assert list(video) == ["V1", "V1", "V1", "V2"] and list(frame) == [2, 7, 10, 4]
    # a stable sort: equal keys keep their order
    ds = _fake_set([("V1", 3, "OTH"), ("V1", 3, "HIT"), ("V1", 1, "OTH")])
    assert list(time_order(ds)[0]) == [2, 0, 1]
    rows, start, video, frame = time_order(_fake_set([]))
    assert len(rows) == len(start) == len(video) == len(frame) == 0


def test_label_runs():
    from tennis_amd.events import label_runs
    first, last, cls = label_runs([0, 0, 2, 2, 2, 0, 1], [1, 0, 0, 0, 1, 0, 0])
    assert list(first) == [0, 2, 4, 5, 6] and list(last) == [1, 3, 4, 5, 6] and list(cls) == [0, 2, 2, 0, 1]
    first, last, cls = label_runs([3, 3, 3], [0, 0, 0])                          # position 0 always begins a run
    assert list(first) == [0] and list(last) == [2] and list(cls) == [3]
    assert all(len(a) == 0 for a in label_runs([], []))
    with pytest.raises(ValueError):
        label_runs([1, 2], [1])
    # the same rule as the reference's runs
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 3, 200)
    st = (rng.random(200) < 0.05).astype(int)
    r = ER.decode_ref(_onehot(lab, 3), np.arange(200), st, 1)
    first, last, cls = label_runs(lab, st)
    assert np.array_equal(first, r["first"]) and np.array_equal(last, r["last"]) and np.array_equal(cls, r["cls"])


def _ev(rows, with_score=True):
    """rows of (video, first_frame, last_frame, cls[, score])"""
    d = dict(video=np.asarray([r[0] for r in rows], dtype=np.str_), first_frame=np.asarray([r[1] for r in rows], np.int64),
             last_frame=np.asarray([r[2] for r in rows], np.int64), cls=np.asarray([r[3] for r in rows], np.int64))
    if with_score:
        d["score"] = np.asarray([r[4] for r in rows], np.float64)
    return d


def test_event_prf1_on_handmade_sets():
    from tennis_amd.metrics.events import EventPRF1, tiou
    assert tiou(0, 9, 5, 14) == 5 / 15 and tiou(0, 4, 5, 9) == 0 and tiou(3, 3, 3, 3) == 1
    classes = ["OTH", "SERVE", "HIT"]
    gt = _ev([("V1", 10, 19, 1), ("V1", 40, 49, 2), ("V2", 0, 9, 1)], with_score=False)
    # a perfect match
    m = EventPRF1(classes)
    m.update(_ev([("V1", 10, 19, 1, 0.9), ("V1", 40, 49, 2, 0.8), ("V2", 0, 9, 1, 0.7)]), gt)
    assert m.tp.sum(1).tolist() == [3, 3, 3] and m.fp.sum() == 0 and m.fn.sum() == 0
    assert dict(m.get())["AVG_f1@0.5"] == 1.0 and dict(m.get())["SERVE_rec@0.1"] == 1.0
    # a shifted event: frames 15-24 against 10-19, tIoU = 5 / 15 - passes at 0.1 and 0.3, fails at 0.5
    m = EventPRF1(classes)
    m.update(_ev([("V1", 15, 24, 1, 0.9)]), _ev([("V1", 10, 19, 1)], with_score=False))
    assert m.tp[:, 1].tolist() == [1, 1, 0] and m.fp[:, 1].tolist() == [0, 0, 1] and m.fn[:, 1].tolist() == [0, 0, 1]
    # two predictions on one ground-truth event: the better-scored one takes it, the other is a false positive
    m = EventPRF1(classes)
    m.update(_ev([("V1", 10, 14, 1, 0.5), ("V1", 15, 19, 1, 0.9)]), _ev([("V1", 10, 19, 1)], with_score=False))
    assert m.tp[:, 1].tolist() == [1, 1, 1] and m.fp[:, 1].tolist() == [1, 1, 1] and m.fn[:, 1].tolist() == [0, 0, 0]
    prec, rec, f1 = m.arrays()
    assert prec[0, 1] == 0.5 and rec[0, 1] == 1.0 and prec.shape == (3, 3)
    # a wrong class: one false positive of the predicted class, one false negative of the true one; another video never matches
    m = EventPRF1(classes)
    m.update(_ev([("V1", 10, 19, 2, 0.9), ("V2", 10, 19, 1, 0.9)]), _ev([("V1", 10, 19, 1)], with_score=False))
    assert m.tp.sum() == 0 and m.fp[0].tolist() == [0, 1, 1] and m.fn[0].tolist() == [0, 1, 0]
    # a score tie goes to the earlier first_frame; a tIoU tie goes to the earlier ground-truth event
    m = EventPRF1(classes, tious=(0.5,))
    m.update(_ev([("V1", 12, 21, 1, 0.9), ("V1", 8, 17, 1, 0.9)]), _ev([("V1", 10, 19, 1)], with_score=False))
    assert m.tp[0, 1] == 1 and m.fp[0, 1] == 1
    m = EventPRF1(classes, tious=(0.1,))
    m.update(_ev([("V1", 10, 19, 1, 0.9)]), _ev([("V1", 5, 14, 1), ("V1", 15, 24, 1)], with_score=False))
    assert m.tp[0, 1] == 1 and m.fn[0, 1] == 1
    # ignore leaves a class out of the average only
    pred = _ev([("V1", 0, 9, 0, 0.9), ("V1", 10, 19, 1, 0.9)])
    g2 = _ev([("V1", 0, 4, 0), ("V1", 10, 19, 1)], with_score=False)
    a, b = EventPRF1(classes, tious=(0.9,)), EventPRF1(classes, tious=(0.9,), ignore=("OTH",))
    a.update(pred, g2); b.update(pred, g2)
    assert np.array_equal(a.tp, b.tp) and np.array_equal(a.fp, b.fp)
    assert dict(a.get())["AVG_f1@0.9"] == 0.5 and dict(b.get())["AVG_f1@0.9"] == 1.0
    assert dict(b.get())["OTH_f1@0.9"] == 0.0
    with pytest.raises(ValueError):
        EventPRF1(classes, ignore=("NOPE",))


def test_save_events_round_trip(tmp_path):
    from tennis_amd import events as E
    cols = dict(video=["V1", "V1", "V002"], first_frame=[0, 10, 3], last_frame=[9, 12, 3], cls=[0, 2, 1],
                score=np.asarray([0.5, 0.93, 1.0], np.float32), peak=np.asarray([0.7, 0.99, 1.0], np.float32), first_sample=[4, 0, 9],
                last_sample=[5, 1, 9], gt_video=["V1", "V002"], gt_first_frame=[0, 3], gt_last_frame=[12, 3], gt_cls=[0, 1], smooth=9,
                tiou=[0.1, 0.3, 0.5], precision=np.full((3, 3), 0.5), recall=np.full((3, 3), 0.25), f1=np.full((3, 3), 1 / 3))
    path = str(tmp_path / "sub" / "test_events.npz")
    E.save_events(path, **cols)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS)
    d = E.load_events(path)
    assert d["video"].dtype.kind == "U" and list(d["video"]) == cols["video"] and list(d["gt_video"]) == cols["gt_video"]
    for k in ("first_frame", "last_frame", "cls", "first_sample", "last_sample", "gt_first_frame", "gt_last_frame", "gt_cls"):
        assert d[k].dtype == np.int64 and list(d[k]) == cols[k], k
    assert d["score"].dtype == np.float32 and np.array_equal(d["score"], cols["score"]) and np.array_equal(d["peak"], cols["peak"])
    assert int(d["smooth"]) == 9 and d["tiou"].shape == (3,) and d["precision"].shape == d["recall"].shape == d["f1"].shape == (3, 3)
    with pytest.raises(ValueError, match="cls"):
        E.save_events(path, **dict(cols, cls=[0, 1]))
    with pytest.raises(ValueError, match="gt_cls"):
        E.save_events(path, **dict(cols, gt_cls=[0]))
    np.savez(str(tmp_path / "other.npz"), video=np.asarray(["V1"]))
    with pytest.raises(ValueError, match="not a file of save_events"):
        E.load_events(str(tmp_path / "other.npz"))


def test_save_events_flag_and_refusals():
    from tennis_amd import evaluate as ev
    from tennis_amd.events import check_save_events
    parse = ev.build_parser().parse_args
    assert parse([]).save_events is False and parse([]).event_smooth is None
    assert parse(["--save_events", "--event_smooth", "9"]).event_smooth == 9
    for bad, why in ((["--save_events", "--save_feats"], "--save_feats"), (["--save_events", "--corpus_frames", "64"], "--corpus_frames"),
                     (["--save_events", "--num_gpus", "2"], "--num_gpus 1"), (["--save_events", "--event_smooth", "4"], "odd"),
                     (["--save_events", "--event_smooth", "65"], r"\[1, 63\]"), (["--save_events", "--event_smooth", "-1"], "--event_smooth -1"),
                     (["--save_events", "--event_smooth", "0"], "--event_smooth 0"), (["--event_smooth", "9"], "--save_events")):
        with pytest.raises(SystemExit, match=why):
            ev.main(["--root", "/nonexistent"] + bad)                            # refused before anything is opened or built
    for good in (["--save_events"], ["--save_events", "--event_smooth", "63"], ["--save_events", "--window", "4", "--temp_pool", "gru"],
                 ["--save_events", "--window", "8", "--temp_pool", "max", "--dense_windows", "--feats_model", "0006"],
                 ["--save_events", "--window", "4", "--temp_pool", "gru", "--save_tams"], []):
        check_save_events(parse(good))
    with pytest.raises(SystemExit, match="one rank"):
        check_save_events(parse(["--save_events"]), world=2)
    check_save_events(types.SimpleNamespace(save_feats=True))                    # flags built by hand, without the newer switches


def test_abi_surface_of_the_event_decoder():
    import ctypes
    from tennis_amd import _lib
    pub = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    declared = _lib.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tn_event_decoder_create", "tn_event_decoder_run", "tn_event_decoder_destroy"):
        assert re.search(r"^int %s\(" % name, pub, re.M), name
        assert name in declared and getattr(lib, name) is not None, name
    assert re.search(r"^int tn_dbg_event_decoder_geometry\(", dbg, re.M) and "tn_dbg_event_decoder_geometry" not in pub
    assert "tn_dbg_event_decoder_geometry" in declared
    for words in ("first arg-max", "ascending", "no atomics on floats", "clamp(rows[m], 0, N-1)"):
        assert words in pub, words
    # the geometry hook touches no device
    from tennis_amd.engine import event_decoder_geometry
    tile, scan = event_decoder_geometry()
    assert tile >= 64 and tile % 64 == 0 and scan >= 64
    assert _lib.load().tn_dbg_event_decoder_geometry(None, None) != 0 and b"tile" in _lib.load().tn_last_error()
    # kernels.md carries the contract
    doc = open(os.path.join(ROOT, "docs", "kernels.md")).read()
    assert "Event decoding" in doc and "event_score_kernel" in doc
