"""No GPU: ``events.viterbi_labels`` (the host restatement of the switch-cost path decoder) against the brute-force optimum
(tests/tools/viterbi_ref.py), its float32 run against its float64 run on dyadic inputs, cost 0 against the per-frame arg-max, the
refusals of ``--event_switch_cost``, the ``switch_cost`` column and the ABI surface."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import viterbi_ref as VR

COSTS = [0.0, 0.3, 1.5, 50.0]


def _tiny_cases():
    rng = np.random.default_rng(0)
    for i in range(300):
        t, c = int(rng.integers(1, 7)), int(rng.integers(1, 4))
        logits = rng.normal(0, 1.5, (t, c)).astype(np.float32)
        if i % 3 == 0:
            logits = np.round(logits * 2) / 2                                    # a coarse grid: ties between paths
        start = (rng.random(t) < 0.25).astype(np.int32)
        yield logits, start


def test_viterbi_labels_is_the_brute_force_optimum():
    from tennis_amd.events import viterbi_labels
    worst = 0.0
    for logits, start in _tiny_cases():
        t, c = logits.shape
        rows = np.arange(t)
        e = VR.emissions(logits, rows)
        for cost in COSTS:
            lab = viterbi_labels(logits, rows, start, cost)
            assert lab.shape == (t,) and lab.dtype == np.int64 and lab.min() >= 0 and lab.max() < c
            best = VR.brute_force(e, start, cost)
            got = VR.path_score(e, lab, start, cost)
            worst = max(worst, best - got)
            assert got <= best + 1e-12 and best - got <= 1e-12 * (1 + abs(best)), (logits, start, cost, lab)
            assert abs(VR.optimum(e, start, cost) - best) <= 1e-12 * (1 + abs(best))     # the textbook recursion agrees as well
    print("viterbi_labels against brute force: largest shortfall %.3g" % worst)


def test_float32_and_float64_agree_exactly_on_dyadic_inputs():
    from tennis_amd.events import viterbi_labels
    rng = np.random.default_rng(1)
    for c, cost in ((1, 0.25), (2, 0.0), (2, 1.0), (3, 0.25), (11, 3.5), (64, 1000.0), (11, 0.25)):
        m = 400
        logits = (rng.integers(-8, 9, (m + 20, c)) / 4.0).astype(np.float32)      # multiples of 2^-2: every operation is exact in fp32
        rows = rng.permutation(m + 20)[:m]
        start = (rng.random(m) < 0.03).astype(np.int32)
        a = viterbi_labels(logits, rows, start, cost, dtype=np.float32)
        b = viterbi_labels(logits, rows, start, cost, dtype=np.float64)
        assert np.array_equal(a, b), (c, cost)
        _, amax_tie, stay_tie = VR.forward_values(VR.emissions(logits, rows), start, cost)
        if c > 1:
            assert amax_tie.any() and (stay_tie.any() or cost > 3.5)             # the ties the two runs had to agree on


def test_cost_zero_is_the_first_arg_max_and_a_large_cost_is_one_label_per_video():
    from tennis_amd.events import label_runs, viterbi_labels
    rng = np.random.default_rng(2)
    m, c = 500, 11
    logits = rng.normal(0, 2, (m, c)).astype(np.float32)                         # (continuous values: no row has a tied maximum)
    rows = rng.permutation(m)
    start = (rng.random(m) < 0.02).astype(np.int32)
    assert np.array_equal(viterbi_labels(logits, rows, start, 0.0), logits[rows].argmax(1))
    assert np.array_equal(viterbi_labels(logits, rows, start, 0.0, dtype=np.float32), logits[rows].argmax(1))
    runs = [len(label_runs(viterbi_labels(logits, rows, start, cost), start)[0]) for cost in (0.0, 0.5, 2.0, 8.0, 1e6)]
    assert runs == sorted(runs, reverse=True) and runs[0] > runs[2] > runs[-1]   # a larger cost never adds runs
    assert runs[-1] == len(VR.videos(start))
    # rows are clipped, position 0 begins a video whatever its flag says
    assert np.array_equal(viterbi_labels(logits, [-5, 10 ** 6], [0, 0], 1.0), viterbi_labels(logits, [0, m - 1], [1, 0], 1.0))
    assert len(viterbi_labels(logits, [], [], 1.0)) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="switch_cost"):
            viterbi_labels(logits, rows, start, bad)
    with pytest.raises(ValueError, match="start flags"):
        viterbi_labels(logits, [0, 1], [1], 1.0)


def test_a_glitch_is_absorbed_and_a_boundary_stays():
    from tennis_amd.events import viterbi_labels
    x = np.zeros((12, 3), np.float32)
    truth = np.array([0] * 5 + [2] * 7)
    x[np.arange(12), truth] = 4.0
    x[2, 1] = 5.0                                                                # one position where a wrong class leads by 1
    x[8, 0] = 5.0
    assert list(viterbi_labels(x, np.arange(12), np.zeros(12), 1.0)) == list(truth)
    glitched = truth.copy()
    glitched[2], glitched[8] = 1, 0
    assert list(viterbi_labels(x, np.arange(12), np.zeros(12), 0.0)) == list(glitched)
    assert list(viterbi_labels(x, np.arange(12), np.zeros(12), 0.5)) == list(truth)        # a lead of 1 = 2 x 0.5: the tie stays
    assert list(viterbi_labels(x, np.arange(12), np.zeros(12), 0.49)) == list(glitched)


def test_switch_cost_flag_and_refusals():
    from tennis_amd import evaluate as ev
    from tennis_amd.events import check_save_events
    parse = ev.build_parser().parse_args
    assert parse([]).event_switch_cost is None
    assert parse(["--save_events", "--event_switch_cost", "2.5"]).event_switch_cost == 2.5
    for bad, why in ((["--event_switch_cost", "2"], "give --save_events too"),
                     (["--save_events", "--event_switch_cost", "2", "--event_smooth", "3"], "not together with --event_smooth 3"),
                     (["--save_events", "--event_switch_cost", "-0.5"], "finite and >= 0"),
                     (["--save_events", "--event_switch_cost", "nan"], "finite and >= 0"),
                     (["--save_events", "--event_switch_cost", "inf"], "finite and >= 0"),
                     (["--save_events", "--event_switch_cost", "2", "--num_gpus", "2"], "--num_gpus 1"),
                     (["--save_events", "--event_switch_cost", "2", "--save_feats"], "--save_feats")):
        with pytest.raises(SystemExit, match=why):
            ev.main(["--root", "/nonexistent"] + bad)                            # refused before anything is opened or built
    for good in (["--save_events", "--event_switch_cost", "0"], ["--save_events", "--event_switch_cost", "2", "--event_smooth", "1"],
                 ["--save_events", "--event_switch_cost", "1000", "--window", "4", "--temp_pool", "gru"]):
        check_save_events(parse(good))


def _cols():
    return dict(video=["V1", "V1"], first_frame=[0, 10], last_frame=[9, 12], cls=[0, 2], score=np.asarray([0.5, 0.9], np.float32),
                peak=np.asarray([0.7, 0.99], np.float32), first_sample=[4, 0], last_sample=[5, 1], gt_video=["V1"], gt_first_frame=[0],
                gt_last_frame=[12], gt_cls=[0], smooth=1, tiou=[0.1, 0.3, 0.5], precision=np.full((3, 3), 0.5),
                recall=np.full((3, 3), 0.25), f1=np.full((3, 3), 1 / 3))


def test_the_switch_cost_column_is_written_only_when_given(tmp_path):
    from tennis_amd import events as E
    plain, path = str(tmp_path / "plain.npz"), str(tmp_path / "path.npz")
    E.save_events(plain, **_cols())
    E.save_events(path, **_cols(), switch_cost=2)
    with np.load(plain, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS)                              # exactly the columns it had
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS) | {"switch_cost"}
    d = E.load_events(path)
    assert d["switch_cost"].dtype == np.float64 and float(d["switch_cost"]) == 2.0 and int(d["smooth"]) == 1
    assert "switch_cost" not in E.load_events(plain)
    assert "switch cost 2" in E.event_table(d, ["OTH", "SERVE", "HIT"]) and "smooth 1" in E.event_table(E.load_events(plain), ["OTH", "SERVE", "HIT"])


def test_abi_surface_of_the_switch_cost_entry():
    from tennis_amd import _lib
    pub = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    declared = _lib.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"^int tn_event_decoder_run_switch\(", pub, re.M)
    assert re.search(r"float switch_cost", pub) and "tn_event_decoder_run_switch" in declared
    for name in ("tn_dbg_event_decoder_switch_geometry", "tn_dbg_event_decoder_workspace_bytes"):
        assert re.search(r"^int %s\(" % name, dbg, re.M) and name not in pub and name in declared, name
    for name in ("tn_event_decoder_run_switch", "tn_dbg_event_decoder_switch_geometry", "tn_dbg_event_decoder_workspace_bytes"):
        assert getattr(lib, name) is not None, name
    for words in ("stay_t[c] = (v_{t-1}[c] >= -switch_cost)", "first arg-max of v_t", "TN_ERR_NOMEM", "A tie between staying and switching stays"):
        assert words in pub, words
    # the existing entry keeps its signature
    assert re.search(r"int tn_event_decoder_run\(tn_event_decoder \*d, const float \*logits, int N, int C, const int32_t \*rows, "
                     r"const int32_t \*start, int M,\s+int width,", pub)
    # the geometry hook touches no device
    from tennis_amd.engine import event_decoder_switch_geometry
    tile = event_decoder_switch_geometry()
    assert tile >= 2 and tile <= 4096
    assert _lib.load().tn_dbg_event_decoder_switch_geometry(None) != 0 and b"tile" in _lib.load().tn_last_error()
    assert _lib.load().tn_dbg_event_decoder_workspace_bytes(None, None) != 0 and b"handle" in _lib.load().tn_last_error()
    doc = open(os.path.join(ROOT, "docs", "kernels.md")).read()
    assert "Event decoding with a switch cost" in doc and "viterbi_forward_kernel" in doc
