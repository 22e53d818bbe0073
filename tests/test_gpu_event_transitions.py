"""-m gpu: the transition-matrix path decoder (csrc/event_runs.hip: viterbi_forward_kernel<ONE_ROW, true>, viterbi_trans_backtrack_kernel;
tn_event_decoder_run_transitions, engine.EventDecoder.decode(transitions=...)) against its definition in float64
(events.viterbi_labels(transitions=...), tests/tools/transitions_ref.py).  Shapes are placed from the decoder's own geometry: G
positions of a video per step of the chain kernels (tn_dbg_event_decoder_transition_geometry); layouts and row modes are those of
tests/test_gpu_event_viterbi.py.  Both instantiations run: a handle of up to 16 classes keeps 16-byte back-pointer rows and reduces
over one row of lanes, a handle of up to 64 keeps 64-byte rows; up to 16 classes every case runs on both.

Exactness: logits that are multiples of 2^-6 in [-16, 16] and matrices that are multiples of 2^-2 in [-8, 0] (or -inf) make every
fp32 operation of the recurrence exact (all values are multiples of 2^-6 below 2^13: a class the grammar cuts off falls by at most 32
a step over at most 2 G + 3 steps), so the labels must equal the float64 reference at every position, ties included.  For general fp32
logits the returned path's float64 score is held against the optimum (transitions_ref.path_bound)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tools import events_ref as ER
from tools import transitions_ref as TR
from tools.event_paths import Spy as _Spy
from tools.event_paths import check_events_of_own_frames as _check_events_of_own_frames
from tools.event_paths import layout as _layout
from tools.event_paths import rows_of as _rows
from tools.event_paths import to_numpy as _np

pytestmark = pytest.mark.gpu


def _geometry():
    from tennis_amd.engine import event_decoder_transition_geometry
    return event_decoder_transition_geometry()


G, PITCH16, PITCH64 = _geometry()
SIZES = [1, 2, G - 1, G, G + 1, 2 * G + 3]
CLASSES = [1, 2, 11, 16, 17, 64]
KINDS = ["potts0", "potts0.25", "potts1", "potts3.5", "random", "cyclic", "zero"]
MAXPOS = 4 * G + 64


@pytest.fixture(scope="module")
def decs():
    """max_classes -> handle: 16 runs the one-row instantiation, 64 the other"""
    from tennis_amd.engine import EventDecoder
    return {16: EventDecoder(MAXPOS, 16), 64: EventDecoder(MAXPOS, 64)}


def _handles(decs, c):
    return [decs[k] for k in (16, 64) if c <= k]


def _decode(dec, logits, rows, start, trans=None, frames=True, **kw):
    if trans is not None:
        kw["transitions"] = trans
    return _np(dec.decode(torch.tensor(np.asarray(logits, np.float32), device="cuda"), np.array(rows), np.array(start),
                          return_frames=frames, **kw))


def _matrix(rng, c, kind):
    if kind.startswith("potts"):
        return TR.potts(c, float(kind[5:]))
    if kind == "cyclic":
        return TR.cyclic(c)
    if kind == "zero":
        return np.zeros((c, c), np.float32)
    return (-rng.integers(0, 33, (c, c)) / 4.0).astype(np.float32)                # multiples of 1/4 in [-8, 0], asymmetric


@functools.lru_cache(maxsize=None)
def _exact_case(m, c, kind, coarse):
    """dyadic logits and matrix with their float64 reference, computed once.  ``coarse``: logits from the matrix's own grid
    (multiples of 1/4 in [-1, 1]), so that arg-maxima and predecessors tie; otherwise any multiple of 2^-6 in [-16, 16]."""
    from tennis_amd.events import viterbi_labels
    i_m, i_c, i_k = SIZES.index(m), CLASSES.index(c), KINDS.index(kind)
    seed = (i_m * 7 + i_c) * 11 + i_k * 2 + int(coarse)
    rng = np.random.default_rng(seed)
    n, rows = _rows(rng, m, seed % 3)
    start = _layout(m, (i_m + i_c + i_k) % 3)
    logits = (rng.integers(-4, 5, (n, c)) / 4.0 if coarse else rng.integers(-1024, 1025, (n, c)) / 64.0).astype(np.float32)
    trans = _matrix(rng, c, kind)
    if kind == "random" and coarse and c > 1:
        trans = np.maximum(trans, -1.0)                                          # as coarse as the logits: predecessors tie
    if kind == "random" and c >= 11:
        assert not np.array_equal(trans, trans.T)
    assert np.all(logits * 64 == np.round(logits * 64)) and np.abs(logits).max() <= 16
    finite = trans[np.isfinite(trans)]
    assert np.all(finite * 4 == np.round(finite * 4)) and finite.min() >= -8 and finite.max() <= 0
    label = viterbi_labels(logits, rows, start, transitions=trans)
    _, amax_tie, stay_tie, pred_tie = TR.forward_values(TR.emissions(logits, rows), start, trans)
    x = logits[np.clip(rows, 0, n - 1)].astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    for arr in (logits, rows, start, trans, label, p):
        arr.setflags(write=False)
    return logits, rows, start, trans, label, p, (int(amax_tie.sum()), int(stay_tie.sum()), int(pred_tie.sum()))


def expected_ties(c, kind):
    """which ties the inputs of a class count and matrix kind must hold (over the sizes): a tied arg-max takes two classes; staying
    can tie with another predecessor from two classes on; two predecessors other than the class itself take three classes, and a
    column with more than one of them finite, which the cyclic grammar does not have"""
    return c >= 2, c >= 2, c >= 3 and kind != "cyclic"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("m", SIZES)
def test_labels_equal_float64_exactly_ties_included(decs, report, m, c, kind):
    ties = np.sum([_exact_case(mm, c, kind, True)[6] for mm in SIZES], 0)
    for have, want, what in zip(ties, expected_ties(c, kind), ("tied arg-max", "stay tie", "tie between two other predecessors")):
        assert have > 0 or not want, "no %s among the inputs" % what
    for coarse in (True, False):
        logits, rows, start, trans, label, p, _ = _exact_case(m, c, kind, coarse)
        for dec in _handles(decs, c):
            got = _decode(dec, logits, rows, start, trans)
            assert got["label"].dtype == np.int32 and got["label"].shape == (m,)
            assert np.array_equal(got["label"], label), np.flatnonzero(got["label"] != label)[:8]
            if kind.startswith("potts"):
                same = _decode(dec, logits, rows, start, switch_cost=float(kind[5:]))
                assert all(np.array_equal(got[k], same[k]) for k in same)
            assert TR.forbidden_pairs(got["label"], start, trans) == 0
            err = np.abs(got["conf"].astype(np.float64) - p[np.arange(m), got["label"]])
            bound = ER.score_bound(c, 1)
            key = "event_transitions_m%d_c%d_%s_%s_h%d_conf_err_over_bound" % (m, c, kind, "coarse" if coarse else "fine", dec.classes)
            report[key] = float(err.max() / bound)
            assert np.all(err <= bound), report[key]
            _check_events_of_own_frames(got, start)


def test_the_cyclic_grammar_binds():
    """(a condition on the inputs of the test above: the per-frame arg-max of the same logits does take forbidden transitions)"""
    taken = 0
    for c in CLASSES[2:]:
        logits, rows, start, trans, label, _, _ = _exact_case(2 * G + 3, c, "cyclic", False)
        taken += TR.forbidden_pairs(logits[np.clip(rows, 0, len(logits) - 1)].argmax(1), start, trans)
        assert len(set(label.tolist())) > 1
    assert taken > 50


def test_a_planted_grammar_absorbs_the_forbidden_glitch_and_keeps_the_boundary(decs):
    A, B, Cc = 0, 1, 2
    trans = np.array([[0.0, -np.inf, -0.5],
                      [-0.5, 0.0, -0.5],
                      [-0.5, -0.5, 0.0]], np.float32)
    m, cut = 2 * G + 3, G + 5
    glitches = [7, G - 1, G + 2]                                                 # one frame each, on both sides of a tile edge
    logits = np.zeros((m, 3), np.float32)
    logits[:cut, A] = 4.0
    logits[cut:, Cc] = 4.0
    logits[glitches, B] = 7.0                                                    # B leads A by 3 > 2 x 0.5
    want = np.array([A] * cut + [Cc] * (m - cut))                                # A -> B is forbidden: no glitch comes through,
    start = np.zeros(m, np.int32)                                                # and A -> C stays at the frame the scores put it
    from tennis_amd.events import label_runs, viterbi_labels
    assert np.array_equal(viterbi_labels(logits, np.arange(m), start, transitions=trans), want)
    through = want.copy()
    through[glitches] = B                                                        # a uniform cost of 0.5 lets every one of them through
    for dec in _handles(decs, 3):
        got = _decode(dec, logits, np.arange(m), start, trans)
        assert np.array_equal(got["label"], want)
        assert list(got["first"]) == [0, cut] and list(got["last"]) == [cut - 1, m - 1] and list(got["cls"]) == [A, Cc]
        uniform = _decode(dec, logits, np.arange(m), start, TR.potts(3, 0.5))
        assert np.array_equal(uniform["label"], through)
        first, _, cls = label_runs(through, start)
        assert np.array_equal(uniform["first"], first) and np.array_equal(uniform["cls"], cls) and len(first) == 2 + 2 * len(glitches)


PATH_CASES = [(m, c) for m in (G + 1, 2 * G + 3) for c in (2, 11, 16, 17, 64)] + [(1, 11), (2, 11), (G - 1, 1), (G, 11)]


@pytest.mark.parametrize("m,c", PATH_CASES)
def test_the_path_of_general_logits_is_optimal_within_the_rounding_bound(decs, report, m, c):
    """Gaussian logits of scale 3, a finite random matrix in [-6, 0].  The float64 score of the returned path against the float64
    optimum; the bound is transitions_ref.path_bound's, 2 M 4 2^-24 (max|e| + max|T|), derived there; every case is held to it."""
    from tennis_amd.events import viterbi_labels
    seed = m * 1009 + c * 13
    rng = np.random.default_rng(seed)
    n, rows = _rows(rng, m, seed % 3)
    start = _layout(m, seed % 3 if m > 2 else 2)
    logits = (rng.normal(0, 1, (n, c)) * 3).astype(np.float32)
    trans = (-6.0 * rng.random((c, c))).astype(np.float32)
    e = TR.emissions(logits, rows)
    best = TR.optimum(e, start, trans)
    assert abs(TR.path_score(e, viterbi_labels(logits, rows, start, transitions=trans), start, trans) - best) <= 1e-9 * (1 + abs(best))
    bound = TR.path_bound(m, np.abs(trans).max(), np.abs(e).max())
    x = logits[np.clip(rows, 0, n - 1)].astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    for dec in _handles(decs, c):
        got = _decode(dec, logits, rows, start, trans)
        mine = TR.path_score(e, got["label"], start, trans)
        ratio = (best - mine) / bound
        key = "event_transitions_path_m%d_c%d_h%d_shortfall_over_bound" % (m, c, dec.classes)
        print("%s: %.3g (optimum %.6f, returned path %.6f, bound %.3g)" % (key, ratio, best, mine, bound))
        report[key] = float(ratio)
        assert mine <= best + 1e-9 * (1 + abs(best))
        assert best - mine <= bound, ratio
        assert got["label"].min() >= 0 and got["label"].max() < c
        assert np.all(np.abs(got["conf"] - p[np.arange(m), got["label"]]) <= ER.score_bound(c, 1))
        _check_events_of_own_frames(got, start)
        # the kernel is the definition in fp32: the float32 run of the host restatement gives the same labels
        assert np.array_equal(got["label"], viterbi_labels(logits, rows, start, dtype=np.float32, transitions=trans))


def test_a_video_alone_gives_the_bits_of_the_joint_call():
    from tennis_amd.engine import EventDecoder
    rng = np.random.default_rng(5)
    c = 11
    lengths = [1, 2, G, G + 3, 5, 2 * G + 1, G - 1]
    m = sum(lengths)
    bounds = np.cumsum([0] + lengths)
    start = np.zeros(m, np.int32)
    start[bounds[:-1]] = 1
    n = m + 100
    logits = (rng.normal(0, 1, (n, c)) * 2).astype(np.float32)
    trans = (-3.0 * rng.random((c, c))).astype(np.float32)
    trans[rng.random((c, c)) < 0.2] = -np.inf
    trans[np.arange(c), np.arange(c)] = -0.125
    rows = rng.permutation(n)[:m]
    big, small = EventDecoder(m + 3 * G, 64), EventDecoder(m, 11)                # another max_positions, and the other instantiation
    whole = _decode(big, logits, rows, start, trans)
    again = _decode(big, logits, rows, start, trans)
    other = _decode(small, logits, rows, start, trans)
    assert all(np.array_equal(whole[k], again[k]) and np.array_equal(whole[k], other[k]) for k in whole)
    assert len(set(whole["label"].tolist())) > 3 and len(whole["first"]) > len(lengths)
    assert TR.forbidden_pairs(whole["label"], start, trans) == 0
    for dec in (big, small):
        for a, b in zip(bounds[:-1], bounds[1:]):
            alone = _decode(dec, logits, rows[a:b], start[a:b], trans)
            assert np.array_equal(alone["label"], whole["label"][a:b]) and np.array_equal(alone["conf"], whole["conf"][a:b])
            sel = (whole["first"] >= a) & (whole["first"] < b)
            assert np.array_equal(alone["first"], whole["first"][sel] - a) and np.array_equal(alone["last"], whole["last"][sel] - a)
            for k in ("cls", "score", "peak"):
                assert np.array_equal(alone[k], whole[k][sel]), k


@pytest.mark.parametrize("classes,pitch", [(16, PITCH16), (64, PITCH64)])
def test_nothing_changes_without_the_keyword(classes, pitch):
    from tennis_amd.engine import EventDecoder
    rng = np.random.default_rng(6)
    m, c = 2 * G + 3, 11
    dec = EventDecoder(MAXPOS, classes)
    logits = (rng.normal(0, 1, (m, c)) * 2).astype(np.float32)
    trans = (-2.0 * rng.random((c, c))).astype(np.float32)
    start = _layout(m, 1)
    calls = {"smooth1": dict(smooth=1), "smooth9": dict(smooth=9), "switch2": dict(switch_cost=2.0)}
    before = {k: _decode(dec, logits, np.arange(m), start, **kw) for k, kw in calls.items()}
    held = dec.workspace_bytes()
    first = _decode(dec, logits, np.arange(m), start, trans)
    grown = dec.workspace_bytes()
    mp = (MAXPOS + 3) // 4 * 4
    assert grown == held + mp * (pitch + 5) + 4 * classes * classes + 4          # the documented amount (docs/kernels.md)
    second = _decode(dec, logits, np.arange(m), start, trans)
    assert dec.workspace_bytes() == grown                                        # only the first call allocates
    assert all(np.array_equal(first[k], second[k]) for k in first)
    for k, kw in calls.items():
        after = _decode(dec, logits, np.arange(m), start, **kw)
        assert set(after) == set(before[k]) and all(np.array_equal(before[k][key], after[key]) for key in after), k
    assert dec.workspace_bytes() == grown
    quiet = _decode(dec, logits, np.arange(m), start, trans, frames=False)       # label_out / conf_out NULL: the handle's own buffers
    assert set(quiet) == {"first", "last", "cls", "score", "peak"} and all(np.array_equal(quiet[k], first[k]) for k in quiet)


@pytest.mark.parametrize("classes", [16, 64])
def test_the_paths_interleaved_on_one_handle_give_the_bits_of_a_fresh_handle(classes):
    """The two chains keep their bookkeeping (the videos' bounds, a_t) in workspaces of their own inside one handle.  ONE handle runs
    transitions first, then the switch cost, smooth = 9, transitions and the switch cost again, over every shape; each result must be
    the bits of the same call on a handle that has run nothing else, and the handle grows exactly twice."""
    from tennis_amd.engine import EventDecoder
    dec = EventDecoder(MAXPOS, classes)
    held = [dec.workspace_bytes()]
    for m in (1, G, G + 1, 2 * G + 3):
        for c in (k for k in (3, 16, 17, 64) if k <= classes):
            rng = np.random.default_rng(m * 67 + c)
            n, rows = _rows(rng, m, (m + c) % 3)
            start = np.zeros(m, np.int32)
            start[m // 3 + 1:m // 3 + 2] = 1                                     # two videos from two positions on
            logits = (rng.normal(0, 1, (n, c)) * 2).astype(np.float32)
            trans = (-3.0 * rng.random((c, c))).astype(np.float32)
            calls = {"transitions": dict(transitions=trans), "switch": dict(switch_cost=1.5), "smooth9": dict(smooth=9)}
            fresh = {k: _decode(EventDecoder(MAXPOS, classes), logits, rows, start, **kw) for k, kw in calls.items()}
            for k in ("transitions", "switch", "smooth9", "transitions", "switch"):
                got = _decode(dec, logits, rows, start, **calls[k])
                held.append(dec.workspace_bytes())
                assert set(got) == set(fresh[k]) == {"label", "conf", "first", "last", "cls", "score", "peak"}
                for key in got:
                    assert got[key].dtype == fresh[k][key].dtype and np.array_equal(got[key], fresh[k][key]), (m, c, k, key)
            if m >= 2:
                assert {0, m // 3 + 1} <= set(fresh["smooth9"]["first"].tolist())
    assert sum(b != a for a, b in zip(held, held[1:])) == 2 and held[0] < held[1] < held[2] == held[-1]


def test_a_nan_among_the_logits_leaves_every_label_in_range(decs):
    rng = np.random.default_rng(8)
    m, c = 2 * G + 3, 11
    logits = rng.normal(0, 2, (m, c)).astype(np.float32)
    logits[[3, G, G + 7], [0, 5, 10]] = np.nan
    logits[G + 20] = np.nan
    trans = (-2.0 * rng.random((c, c))).astype(np.float32)
    for dec in _handles(decs, c):
        got = _decode(dec, logits, np.arange(m), _layout(m, 1), trans)
        assert got["label"].min() >= 0 and got["label"].max() < c and got["cls"].min() >= 0 and got["cls"].max() < c
        assert 1 <= len(got["first"]) <= m


def test_refusals(decs):
    from tennis_amd import _lib
    dec = decs[64]
    lib = _lib.load()
    P = _lib.ptr
    m, n, c = 16, 16, 11
    lg = torch.zeros((n, c), device="cuda")
    iv = torch.zeros(m, dtype=torch.int32, device="cuda")
    ev = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.zeros(m, device="cuda") for _ in range(2)]
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    good = np.zeros((c, c), np.float32)

    def matrix(p, q, value):
        t = good.copy()
        t[p, q] = value
        return t

    def run(**k):
        a = dict(h=dec.handle, logits=P(lg), N=n, C=c, rows=P(iv), start=P(iv), M=m, trans=good, first=P(ev[0]), last=P(ev[1]), cls=P(ev[2]),
                 score=P(ev[3]), peak=P(ev[4]), count=P(cnt))
        a.update(k)
        t = None if a["trans"] is None else np.ascontiguousarray(a["trans"], np.float32).ctypes.data_as(C.c_void_p)
        return lib.tn_event_decoder_run_transitions(a["h"], a["logits"], a["N"], a["C"], a["rows"], a["start"], a["M"], t, None, None,
                                                    a["first"], a["last"], a["cls"], a["score"], a["peak"], a["count"], None)
    for bad, word in ((dict(trans=matrix(2, 3, np.nan)), b"transitions[2][3] is NaN"), (dict(trans=matrix(4, 1, 0.5)), b"transitions[4][1] is positive"),
                      (dict(trans=matrix(0, 10, np.inf)), b"transitions[0][10] is positive"),
                      (dict(trans=matrix(7, 7, -np.inf)), b"transitions[7][7] is not finite"), (dict(trans=None), b"transitions is null"),
                      (dict(h=None), b"handle"), (dict(logits=None), b"logits"), (dict(rows=None), b"rows"), (dict(start=None), b"start"),
                      (dict(first=None), b"ev_first"), (dict(count=None), b"count"), (dict(C=65), b"C "), (dict(C=0), b"C "),
                      (dict(M=dec.max_positions + 1), b"max_positions"), (dict(M=0), b"M "), (dict(N=0), b"N ")):
        assert run(**bad) == -1, bad
        assert word in lib.tn_last_error() and b"tn_event_decoder_run_transitions" in lib.tn_last_error(), (bad, lib.tn_last_error())
    first_bad = good.copy()
    first_bad[5, 5], first_bad[3, 8] = np.nan, 1.0                               # the first offending entry in row-major order is named
    assert run(trans=first_bad) == -1 and b"transitions[3][8] is positive" in lib.tn_last_error()
    torch.cuda.synchronize()
    assert int(cnt.item()) == -7                                                 # nothing was launched
    assert run(trans=matrix(2, 3, -np.inf)) == 0                                 # -inf off the diagonal forbids, it is not refused
    torch.cuda.synchronize()
    assert int(cnt.item()) == 1                                                  # all-zero logits, one video: one event
    x = torch.zeros((n, c), device="cuda")
    calls = []
    with pytest.MonkeyPatch.context() as mp:                                     # refused in front of every entry of the library
        mp.setattr(dec, "lib", _Spy(dec.lib, calls))
        for bad, why in ((matrix(2, 3, np.nan), r"\[2\]\[3\] is NaN"), (matrix(4, 1, 0.5), r"\[4\]\[1\] is positive"),
                         (matrix(0, 10, np.inf), r"\[0\]\[10\] is positive"), (matrix(7, 7, -np.inf), r"\[7\]\[7\] is not finite"),
                         (np.zeros((c, c + 1), np.float32), r"\(11, 11\)"), (np.zeros((c - 1, c - 1), np.float32), r"\(11, 11\)"),
                         (np.zeros(c * c, np.float32), r"\(11, 11\)")):
            with pytest.raises(ValueError, match=why):
                dec.decode(x, np.arange(m), np.zeros(m), transitions=bad)
        with pytest.raises(ValueError, match="smooth=3"):
            dec.decode(x, np.arange(m), np.zeros(m), smooth=3, transitions=good)
        with pytest.raises(ValueError, match="switch_cost=1"):
            dec.decode(x, np.arange(m), np.zeros(m), switch_cost=1.0, transitions=good)
    assert calls == []
    ok = dec.decode(x, np.arange(m), np.zeros(m), transitions=torch.zeros((c, c)))   # a CPU tensor is taken as well
    assert len(ok["first"]) == 1
    from tennis_amd.engine import EventDecoder
    small = EventDecoder(8, 4)                                                   # C above the handle's
    created = small.workspace_bytes()
    with pytest.raises(RuntimeError, match="max_classes"):
        small.decode(x, np.arange(8), np.zeros(8), transitions=good)
    assert small.workspace_bytes() == created                                    # and nothing was allocated for it
    torch.cuda.synchronize()
