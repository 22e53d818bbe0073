"""-m gpu: evaluate --save_events --event_transitions train --event_posteriors on the tiny synthetic split of
tests/test_gpu_save_events_transitions.py (2 videos of 20 frames, window 4, stored features 64 wide; the loader route and
--dense_windows).  Two runs of the driver per route, without and with the flag: the printed scores and the events must not change, the
file gains its ``posteriors`` column only with the flag, and its scores are then those of events.hmm_posteriors on the run's own
logits."""
import contextlib
import io
import os

import numpy as np
import pytest

from tools import events_ref as ER

pytestmark = pytest.mark.gpu

FRAMES, WINDOW, FEAT = 20, 4, 64
ROUTES = {"loader": ["--feats_model", "0006"], "dense_features": ["--feats_model", "0006", "--dense_windows"]}


def _scores(out):
    """the confusion matrix and the [Finished] line without its time"""
    text = out[out.index("Test set:"):]
    return text[:text.index("Time Taken")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """route -> per run of the driver what it printed, decoded and wrote"""
    from tennis_amd import evaluate as ev
    from tennis_amd.dataset import TennisSet
    base = tmp_path_factory.mktemp("save_events_posteriors")
    root = str(base / "data")
    ds = TennisSet(root=root, window=WINDOW, stride=2, frames_per_video=FRAMES, data_shape=224, split="test", balance=False, feats_model="0006")
    rng = np.random.default_rng(2)
    for v, f in ds.window_table()[0]:                                            # the stored features: 64 wide, one file per frame
        path = ds.get_feature_path(ds.feat_dir, v, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, (np.abs(rng.normal(0, 1, FEAT)) * 0.5).astype(np.float32))
    flags = {"path": ["--save_events", "--event_transitions", "train"],
             "post": ["--save_events", "--event_transitions", "train", "--event_posteriors"]}
    out = {}
    for route, extra in ROUTES.items():
        exp = str(base / ("exp_" + route))
        args = ["--root", root, "--frames_per_video", str(FRAMES), "--data_shape", "224", "--window", str(WINDOW), "--stride", "2",
                "--temp_pool", "gru", "--batch_size", "8", "--exp_root", exp] + extra
        file = os.path.join(exp, "0000", "test_events.npz")
        rec = dict(dataset=ds)
        with pytest.MonkeyPatch.context() as mp:
            decoded = []

            def decoding(dataset, logits, order=None, **k):
                decoded.append((logits.cpu().numpy().copy(), None if order is None else list(order), dict(k)))
                return ev_decode(dataset, logits, order, **k)
            ev_decode = ev.decode_split
            mp.setattr(ev, "decode_split", decoding)
            for name, flag in flags.items():
                del decoded[:]
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    assert ev.main(args + flag) == 0
                with np.load(file, allow_pickle=False) as z:
                    cols = {k: z[k] for k in z.files}
                rec[name] = dict(text=buf.getvalue(), decoded=list(decoded), cols=cols)
        out[route] = rec
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_flag_adds_its_column_and_moves_no_event_and_no_metric(runs, route):
    from tennis_amd.events import EVENT_COLUMNS
    path, post = runs[route]["path"], runs[route]["post"]
    assert _scores(path["text"]) == _scores(post["text"])
    assert [ln for ln in path["text"].splitlines() if ln.startswith("[Events]")] == [ln for ln in post["text"].splitlines() if ln.startswith("[Events]")]
    assert "(transition matrix)" in path["text"] and "(transition matrix, posterior scores)" in post["text"]
    assert set(path["cols"]) == set(EVENT_COLUMNS) | {"transitions"}
    assert set(post["cols"]) == set(EVENT_COLUMNS) | {"transitions", "posteriors"}
    assert post["cols"]["posteriors"].shape == () and bool(post["cols"]["posteriors"])
    (_, _, kw_path), = path["decoded"]
    (_, _, kw_post), = post["decoded"]
    assert "posteriors" not in kw_path and kw_post["posteriors"] is True         # without the flag the call is the call it was
    for k in ("video", "first_frame", "last_frame", "cls", "first_sample", "last_sample", "gt_video", "gt_first_frame", "gt_last_frame", "gt_cls",
              "transitions", "precision", "recall", "f1"):
        assert np.array_equal(path["cols"][k], post["cols"][k]), k
    for cols in (path["cols"], post["cols"]):
        assert np.all(cols["score"] > 0) and np.all(cols["score"] <= 1) and np.all(cols["peak"] > 0) and np.all(cols["peak"] <= 1)
        assert np.all(cols["score"] <= cols["peak"] * (1 + 2.0 ** -20))
    assert not np.array_equal(path["cols"]["score"], post["cols"]["score"])


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_scores_are_those_of_the_posteriors_of_the_run_s_own_logits(runs, route):
    from tennis_amd.events import hmm_posteriors, label_runs, time_order, viterbi_labels
    rec = runs[route]
    (logits, order, _), = rec["post"]["decoded"]
    d = rec["post"]["cols"]
    rows, start, _, _ = time_order(rec["dataset"], order)
    label = viterbi_labels(logits, rows, start, dtype=np.float32, transitions=d["transitions"])
    first, last, cls = label_runs(label, start)
    assert np.array_equal(d["cls"], cls)
    g64 = hmm_posteriors(logits, rows, start, d["transitions"])
    # gamma = softmax(ah + bh): a log-domain value has magnitude <= S = max|e| + max|T| and carries the roundings of its last step
    # (about ten, of relative size u = 2^-24 each; what earlier steps left is shared by the classes up to the chain's mixing and
    # cancels in the softmax), and |d gamma| <= gamma (1 - gamma) |d g_c - d g_c'| <= 1/4 * 2 * 2 * 10 u S; with the softmax's own
    # roundings and a spare factor of 3: 32 u (1 + S)
    x = logits[rows].astype(np.float64)
    spread = float((x.max(1) - x.min(1)).max()) + float(np.abs(d["transitions"][np.isfinite(d["transitions"])]).max())
    bar = 32 * ER.U * (1 + spread)
    conf = g64[np.arange(len(rows)), label]
    assert np.all(np.abs(d["peak"] - np.asarray([conf[a:b + 1].max() for a, b in zip(first, last)])) <= bar)
    assert np.all(np.abs(d["score"] - np.asarray([conf[a:b + 1].mean() for a, b in zip(first, last)]))
                  <= bar + np.asarray([ER.mean_bound(int(b - a + 1)) for a, b in zip(first, last)]))
