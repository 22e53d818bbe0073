"""No GPU: ``events.viterbi_labels(transitions=...)`` (the host restatement of the transition-matrix path decoder) against the
brute-force optimum (tests/tools/transitions_ref.py), its Potts form against ``viterbi_labels(switch_cost=...)``, its float32 run
against its float64 run on dyadic inputs, forbidden transitions, ``events.transition_scores`` against a hand count, the refusals of
``--event_transitions``, the ``transitions`` column and the ABI surface."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import transitions_ref as TR

LAYOUTS = [lambda t: np.zeros(t, np.int32), lambda t: (np.arange(t) % 3 == 0).astype(np.int32), lambda t: (np.arange(t) == t // 2).astype(np.int32),
           lambda t: np.ones(t, np.int32)]


def _dyadic_matrix(rng, c, holes):
    """multiples of 1/4 in [-4, 0], asymmetric; ``holes``: some off-diagonal entries -inf"""
    t = (-rng.integers(0, 17, (c, c)) / 4.0).astype(np.float32)
    if holes and c > 1:
        t[(rng.random((c, c)) < 0.3) & ~np.eye(c, dtype=bool)] = -np.inf
    return t


def _tiny_cases():
    rng = np.random.default_rng(0)
    for i in range(240):
        c = int(rng.integers(1, 5))
        t = int(rng.integers(1, {1: 8, 2: 8, 3: 8, 4: 8}[c]))                     # C^M <= 4^7
        logits = rng.normal(0, 1.5, (t, c)).astype(np.float32)
        if i % 3 == 0:
            logits = np.round(logits * 2) / 2                                    # a coarse grid: ties between paths
        yield logits, LAYOUTS[i % len(LAYOUTS)](t), _dyadic_matrix(rng, c, i % 2 == 1)


def test_the_matrix_form_reaches_the_brute_force_optimum():
    from tennis_amd.events import viterbi_labels
    worst, holes = 0.0, 0
    for logits, start, trans in _tiny_cases():
        t, c = logits.shape
        rows = np.arange(t)
        e = TR.emissions(logits, rows)
        lab = viterbi_labels(logits, rows, start, transitions=trans)
        assert lab.shape == (t,) and lab.dtype == np.int64 and lab.min() >= 0 and lab.max() < c
        best = TR.brute_force(e, start, trans)
        got = TR.path_score(e, lab, start, trans)
        holes += int(np.isneginf(trans).any())
        worst = max(worst, best - got)
        assert np.isfinite(best) and got <= best + 1e-12 and best - got <= 1e-12 * (1 + abs(best)), (logits, start, trans, lab)
        assert abs(TR.optimum(e, start, trans) - best) <= 1e-12 * (1 + abs(best))       # the textbook recursion agrees as well
        assert TR.forbidden_pairs(lab, start, trans) == 0
    assert holes > 40
    print("viterbi_labels(transitions=) against brute force: largest shortfall %.3g" % worst)


@pytest.mark.parametrize("cost", [0.0, 0.25, 1.0, 3.5])
def test_the_potts_form_gives_the_switch_cost_labels(cost):
    from tennis_amd.events import viterbi_labels
    rng = np.random.default_rng(int(cost * 4) + 1)
    for c in (1, 2, 3, 11, 17):
        m = 300
        logits = (rng.integers(-8, 9, (m + 20, c)) / 4.0).astype(np.float32)      # multiples of 2^-2: every operation is exact
        rows = rng.permutation(m + 20)[:m]
        start = (rng.random(m) < 0.03).astype(np.int32)
        want = viterbi_labels(logits, rows, start, cost)
        for dtype in (np.float32, np.float64):
            assert np.array_equal(viterbi_labels(logits, rows, start, dtype=dtype, transitions=TR.potts(c, cost)), want), (c, dtype)
        assert np.array_equal(viterbi_labels(logits, rows, start, None, np.float64, TR.potts(c, cost)), want)      # positional


def test_float32_and_float64_agree_exactly_on_dyadic_inputs():
    from tennis_amd.events import viterbi_labels
    rng = np.random.default_rng(1)
    for c, holes in ((1, False), (2, False), (3, True), (11, False), (11, True), (64, True)):
        m = 300
        logits = (rng.integers(-8, 9, (m + 20, c)) / 4.0).astype(np.float32)
        rows = rng.permutation(m + 20)[:m]
        start = (rng.random(m) < 0.03).astype(np.int32)
        trans = _dyadic_matrix(rng, c, holes)
        a = viterbi_labels(logits, rows, start, dtype=np.float32, transitions=trans)
        b = viterbi_labels(logits, rows, start, dtype=np.float64, transitions=trans)
        assert np.array_equal(a, b), (c, holes)
        _, amax_tie, stay_tie, pred_tie = TR.forward_values(TR.emissions(logits, rows), start, trans)
        if c > 2:
            assert amax_tie.any() and stay_tie.any() and pred_tie.any()          # the ties the two runs had to agree on


def test_no_forbidden_transition_is_taken():
    from tennis_amd.events import viterbi_labels
    rng = np.random.default_rng(2)
    for c in (3, 4, 11):                                                         # (with two classes the cycle forbids nothing)
        m = 400
        logits = rng.normal(0, 3, (m, c)).astype(np.float32)
        start = (rng.random(m) < 0.02).astype(np.int32)
        trans = TR.cyclic(c)
        for dtype in (np.float32, np.float64):
            lab = viterbi_labels(logits, np.arange(m), start, dtype=dtype, transitions=trans)
            assert TR.forbidden_pairs(lab, start, trans) == 0
            assert len(set(lab.tolist())) == c                                   # (the grammar does not pin the path to one class)
        free = logits.argmax(1)
        assert TR.forbidden_pairs(free, start, trans) > 0                        # the per-frame arg-max does take them
    # rows are clipped, position 0 begins a video whatever its flag says
    t3 = TR.cyclic(3)
    x = rng.normal(0, 1, (50, 3)).astype(np.float32)
    assert np.array_equal(viterbi_labels(x, [-5, 10 ** 6], [0, 0], transitions=t3), viterbi_labels(x, [0, 49], [1, 0], transitions=t3))
    assert len(viterbi_labels(x, [], [], transitions=t3)) == 0


def test_viterbi_labels_refusals():
    from tennis_amd.events import viterbi_labels
    x = np.zeros((4, 3), np.float32)
    r, s = np.arange(4), np.zeros(4)
    with pytest.raises(ValueError, match="exactly one"):
        viterbi_labels(x, r, s)
    with pytest.raises(ValueError, match="exactly one"):
        viterbi_labels(x, r, s, 1.0, transitions=np.zeros((3, 3)))
    for bad, why in ((np.zeros((2, 2)), r"\(3, 3\)"), (np.zeros(9), r"\(3, 3\)"), (np.full((3, 3), np.nan), r"\[0\]\[0\] is NaN"),
                     (np.array([[0, 0, 0], [0, 0, 0.5], [0, 0, 0]]), r"\[1\]\[2\] is positive"),
                     (np.array([[0, 0, 0], [np.inf, 0, 0], [0, 0, 0]]), r"\[1\]\[0\] is positive"),
                     (np.array([[0, 0, 0], [0, 0, 0], [0, 0, -np.inf]]), r"\[2\]\[2\] is not finite")):
        with pytest.raises(ValueError, match=why):
            viterbi_labels(x, r, s, transitions=bad)
    with pytest.raises(ValueError, match="start flags"):
        viterbi_labels(x, [0, 1], [1], transitions=np.zeros((3, 3)))


def test_transition_scores_against_a_hand_count():
    from tennis_amd.events import transition_scores
    labels, start = [0, 0, 1, 1, 1, 0, 2, 2], [1, 0, 0, 0, 0, 0, 1, 0]
    counts = np.zeros((3, 3))
    counts[0, 0], counts[0, 1], counts[1, 1], counts[1, 0], counts[2, 2] = 1, 1, 2, 1, 1      # (1 -> 0 | 2 across the video start: not counted)
    for prior, scale in ((1.0, 1.0), (0.5, 2.0), (3.0, 0.25)):
        t = transition_scores(labels, start, 3, prior=prior, scale=scale)
        assert t.dtype == np.float32 and t.shape == (3, 3) and np.all(np.isfinite(t)) and np.all(t < 0)
        want = scale * np.log((counts + prior) / (counts.sum(1, keepdims=True) + 3 * prior))
        assert np.array_equal(t, want.astype(np.float32))
        assert np.allclose(np.exp(t.astype(np.float64) / scale).sum(1), 1.0, atol=1e-6)
    assert np.array_equal(transition_scores(labels, [0] + start[1:], 3), transition_scores(labels, start, 3))      # position 0 never counts
    four = transition_scores(labels, start, 4)                                  # a class nobody saw: a uniform row
    assert np.array_equal(four[3], np.full(4, np.log(0.25), np.float32))
    assert transition_scores([], [], 2).tolist() == np.full((2, 2), np.log(0.5), np.float32).tolist()
    for kw, why in ((dict(prior=0.0), "prior"), (dict(prior=-1.0), "prior"), (dict(prior=float("nan")), "prior"), (dict(scale=0.0), "scale"),
                    (dict(scale=float("inf")), "scale")):
        with pytest.raises(ValueError, match=why):
            transition_scores(labels, start, 3, **kw)
    with pytest.raises(ValueError, match="start flags"):
        transition_scores(labels, start[:-1], 3)
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        transition_scores(labels, start, 2)


def test_transition_flags_and_refusals(tmp_path):
    from tennis_amd import evaluate as ev
    from tennis_amd.events import check_save_events
    parse = ev.build_parser().parse_args
    flags = parse([])
    assert flags.event_transitions is None and flags.event_transition_prior is None and flags.event_transition_scale is None
    assert parse(["--save_events", "--event_transitions", "train"]).event_transitions == "train"
    for bad, why in ((["--event_transitions", "train"], "give --save_events too"),
                     (["--save_events", "--event_transitions", "train", "--event_smooth", "3"], "not together with --event_smooth 3"),
                     (["--save_events", "--event_transitions", "train", "--event_switch_cost", "2"], "not together with --event_switch_cost"),
                     (["--save_events", "--event_transition_prior", "2"], "give --event_transitions too"),
                     (["--save_events", "--event_transition_scale", "2"], "give --event_transitions too"),
                     (["--event_transition_scale", "2"], "give --event_transitions too"),
                     (["--save_events", "--event_transitions", "train", "--event_transition_prior", "0"], "finite and > 0"),
                     (["--save_events", "--event_transitions", "train", "--event_transition_scale", "-1"], "finite and > 0"),
                     (["--save_events", "--event_transitions", "train", "--num_gpus", "2"], "--num_gpus 1"),
                     (["--save_events", "--event_transitions", "train", "--save_feats"], "--save_feats")):
        with pytest.raises(SystemExit, match=why):
            ev.main(["--root", "/nonexistent"] + bad)                            # refused before anything is opened or built
    for good in (["--save_events", "--event_transitions", "train"], ["--save_events", "--event_transitions", "train", "--event_smooth", "1"],
                 ["--save_events", "--event_transitions", "t.npy", "--window", "4", "--temp_pool", "gru"],
                 ["--save_events", "--event_transitions", "train", "--event_transition_prior", "0.5", "--event_transition_scale", "2"]):
        check_save_events(parse(good))

    class Old:                                                                   # flags built by hand, without the newer switches
        save_events, save_feats, corpus_frames, num_gpus = True, False, 0, 1
    check_save_events(Old())
    # a matrix file: -inf off the diagonal is kept, anything else the decoder refuses is refused on loading
    class Three:
        classes = ["A", "B", "C"]
    good = np.zeros((3, 3), np.float32)
    good[0, 1] = -np.inf
    np.save(str(tmp_path / "good.npy"), good)
    got, source = ev.event_transitions(parse(["--save_events", "--event_transitions", str(tmp_path / "good.npy")]), Three(), 1)
    assert np.array_equal(got, good) and got.dtype == np.float32 and source.endswith("good.npy")
    np.save(str(tmp_path / "bad.npy"), np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match=r"\(3, 3\)"):
        ev.event_transitions(parse(["--save_events", "--event_transitions", str(tmp_path / "bad.npy")]), Three(), 1)


def _cols():
    return dict(video=["V1", "V1"], first_frame=[0, 10], last_frame=[9, 12], cls=[0, 2], score=np.asarray([0.5, 0.9], np.float32),
                peak=np.asarray([0.7, 0.99], np.float32), first_sample=[4, 0], last_sample=[5, 1], gt_video=["V1"], gt_first_frame=[0],
                gt_last_frame=[12], gt_cls=[0], smooth=1, tiou=[0.1, 0.3, 0.5], precision=np.full((3, 3), 0.5),
                recall=np.full((3, 3), 0.25), f1=np.full((3, 3), 1 / 3))


def test_the_transitions_column_is_written_only_when_given(tmp_path):
    from tennis_amd import events as E
    plain, path = str(tmp_path / "plain.npz"), str(tmp_path / "path.npz")
    trans = TR.cyclic(3)
    E.save_events(plain, **_cols())
    E.save_events(path, **_cols(), transitions=trans)
    with np.load(plain, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS)                              # exactly the columns it had
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS) | {"transitions"}
        assert z["transitions"].dtype == np.float32 and np.array_equal(z["transitions"], trans)
    d = E.load_events(path)
    assert np.array_equal(d["transitions"], trans) and "transitions" not in E.load_events(plain) and "transitions" not in E.EVENT_COLUMNS
    assert "transition matrix" in E.event_table(d, ["OTH", "SERVE", "HIT"]) and "smooth 1" in E.event_table(E.load_events(plain), ["OTH", "SERVE", "HIT"])
    with pytest.raises(ValueError, match=r"\(3, 3\)"):
        E.save_events(path, **_cols(), transitions=np.zeros((2, 2)))


def test_abi_surface_of_the_transition_entry():
    from tennis_amd import _lib
    pub = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    declared = _lib.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"^int tn_event_decoder_run_transitions\(", pub, re.M)
    assert re.search(r"const float \*transitions", pub) and "tn_event_decoder_run_transitions" in declared
    name = "tn_dbg_event_decoder_transition_geometry"
    assert re.search(r"^int %s\(" % name, dbg, re.M) and name not in pub and name in declared
    for sym in ("tn_event_decoder_run_transitions", name):
        assert getattr(lib, sym) is not None, sym
    for words in ("staying wins a tie", "the smallest p that attains it", "label[t-1] = b_t[label[t]]", "HOST pointer", "TN_ERR_NOMEM"):
        assert words in pub, words
    # the existing entries keep their signatures
    assert re.search(r"int tn_event_decoder_run_switch\(tn_event_decoder \*d, const float \*logits, int N, int C, const int32_t \*rows, "
                     r"const int32_t \*start,\s+int M, float switch_cost,", pub)
    from tennis_amd.engine import event_decoder_switch_geometry, event_decoder_transition_geometry
    tile, p16, p64 = event_decoder_transition_geometry()                         # touches no device
    assert tile == event_decoder_switch_geometry() and p16 >= 16 and p64 >= 64 and p16 % 16 == 0 and p64 % 16 == 0
    L = _lib.load()
    one = ctypes.c_int()
    assert L.tn_dbg_event_decoder_transition_geometry(None, ctypes.byref(one), ctypes.byref(one)) != 0 and b"tile" in L.tn_last_error()
    assert L.tn_event_decoder_run_transitions(None, None, 1, 1, None, None, 1, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"tn_event_decoder_run_transitions" in L.tn_last_error() and b"handle" in L.tn_last_error()
    doc = open(os.path.join(ROOT, "docs", "kernels.md")).read()
    assert "Event decoding with a transition matrix" in doc and "viterbi_trans_forward_kernel" in doc and "viterbi_trans_backtrack_kernel" in doc
