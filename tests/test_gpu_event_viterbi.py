"""-m gpu: the switch-cost path decoder (csrc/event_runs.hip: viterbi_forward_kernel<ONE_ROW, false>, viterbi_backtrack_kernel, event_flag_kernel;
tn_event_decoder_run_switch, engine.EventDecoder.decode(switch_cost=...)) against its definition in float64
(events.viterbi_labels, tests/tools/viterbi_ref.py).  Shapes are placed from the decoder's own geometry: G positions of a video per
step of the chain kernels (tn_dbg_event_decoder_switch_geometry).  A video's tiles are counted from the video's own first position,
so "a boundary on a tile edge" is a video of exactly G positions, and a video of G + 3 or 2 G + 3 positions crosses one or two.

Exactness: logits that are multiples of 2^-6 in [-16, 16] and costs that are multiples of 2^-2 make every fp32 operation of the
recurrence exact (all values are multiples of 2^-6 below 2^11), so the labels must equal the float64 reference at every position,
ties included.  For general fp32 logits the returned path's float64 score is held against the optimum (viterbi_ref.path_bound)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tools import events_ref as ER
from tools import viterbi_ref as VR
from tools.event_paths import Spy as _Spy
from tools.event_paths import check_events_of_own_frames as _check_events_of_own_frames
from tools.event_paths import layout as _layout
from tools.event_paths import rows_of as _rows
from tools.event_paths import to_numpy as _np

pytestmark = pytest.mark.gpu


def _geometry():
    from tennis_amd.engine import event_decoder_switch_geometry
    return event_decoder_switch_geometry()


G = _geometry()
SIZES = [1, 2, G - 1, G, G + 1, 2 * G + 3]
CLASSES = [1, 2, 11, 16, 17, 64]           # (16 / 17: the forward kernel reduces over one row of lanes up to 16 classes)
COSTS = [0.0, 0.25, 1.0, 3.5, 1000.0]
MAXPOS = 4 * G + 64


@pytest.fixture(scope="module")
def dec():
    from tennis_amd.engine import EventDecoder
    return EventDecoder(MAXPOS, 64)


def _decode(dec, logits, rows, start, cost=None, smooth=1, frames=True):
    kw = {} if cost is None else {"switch_cost": cost}
    return _np(dec.decode(torch.tensor(np.asarray(logits, np.float32), device="cuda"), np.array(rows), np.array(start), smooth=smooth,
                          return_frames=frames, **kw))


@functools.lru_cache(maxsize=None)
def _exact_case(m, c, cost, coarse):
    """dyadic logits with their float64 reference, computed once.  ``coarse``: values from a grid as wide as the cost's own (0.25; 8
    at cost 1000), so that arg-maxima tie and classes sit at exactly -cost; otherwise any multiple of 2^-6 in [-16, 16]."""
    from tennis_amd.events import viterbi_labels
    i_m, i_c, i_k = SIZES.index(m), CLASSES.index(c), COSTS.index(cost)
    seed = (i_m * 7 + i_c) * 11 + i_k * 2 + int(coarse)
    rng = np.random.default_rng(seed)
    n, rows = _rows(rng, m, seed % 3)
    start = _layout(m, (i_m + i_c + i_k) % 3)
    if not coarse:
        logits = rng.integers(-1024, 1025, (n, c)) / 64.0
    elif cost == 1000.0:
        logits = rng.integers(-2, 3, (n, c)) * 8.0
        a, b = max(VR.videos(start), key=lambda v: v[1] - v[0])
        if c > 1 and b - a >= 34:                                                # the last class loses 31 x 32 + 8 = 1000 against class 0
            at = np.clip(rows[a:a + 34], 0, n - 1)
            if len(set(at.tolist())) == 34:                                      # (clamped rows may repeat: then nothing is planted)
                logits[at] = np.minimum(logits[at], 8.0)
                logits[at, 0] = 16.0
                logits[at, c - 1] = -16.0
                logits[at[31], c - 1] = 8.0
    else:
        logits = rng.integers(-4, 5, (n, c)) / 4.0
    logits = logits.astype(np.float32)
    assert np.all(logits * 64 == np.round(logits * 64)) and np.abs(logits).max() <= 16
    label = viterbi_labels(logits, rows, start, cost)
    e = VR.emissions(logits, rows)
    _, amax_tie, stay_tie = VR.forward_values(e, start, cost)
    x = logits[np.clip(rows, 0, n - 1)].astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    for arr in (logits, rows, start, label, p):
        arr.setflags(write=False)
    return logits, rows, start, label, p, int(amax_tie.sum()), int(stay_tie.sum())


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("m", SIZES)
def test_labels_equal_float64_exactly_ties_included(dec, report, m, c, cost):
    # the inputs of this class count and cost hold both kinds of ties (over the sizes: a single position cannot hold a stay / switch
    # decision, and 1000 = 31 x 32 + 8 below the best class takes 32 positions of one video).  One class has no arg-max to tie, and
    # its only value, 0, equals -cost at cost 0 alone.
    ties = [_exact_case(mm, c, cost, True)[5:] for mm in SIZES]
    if c > 1:
        assert sum(t[0] for t in ties) > 0, "no tied arg-max among the inputs"
    if c > 1 or cost == 0.0:
        assert sum(t[1] for t in ties) > 0, "no class at exactly -cost among the inputs"
    for coarse in (True, False):
        logits, rows, start, label, p, _, _ = _exact_case(m, c, cost, coarse)
        got = _decode(dec, logits, rows, start, cost)
        assert got["label"].dtype == np.int32 and got["label"].shape == (m,)
        assert np.array_equal(got["label"], label), np.flatnonzero(got["label"] != label)[:8]
        err = np.abs(got["conf"].astype(np.float64) - p[np.arange(m), got["label"]])
        bound = ER.score_bound(c, 1)
        key = "event_viterbi_m%d_c%d_cost%g_%s_conf_err_over_bound" % (m, c, cost, "coarse" if coarse else "fine")
        report[key] = float(err.max() / bound)
        assert np.all(err <= bound), report[key]
        _check_events_of_own_frames(got, start)


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("m", SIZES)
def test_cost_zero_is_the_width_one_decode_bit_for_bit(dec, m, c):
    rng = np.random.default_rng(m * 131 + c)
    n, rows = _rows(rng, m, (m + c) % 3)
    start = _layout(m, (m + c) % 3)
    # a random order of distinct multiples of 2^-6 per row: the maximum leads by at least 2^-6
    logits = (np.argsort(rng.random((n, max(c, 2))), 1)[:, :c] * (rng.integers(1, 9, (n, 1)) / 64.0) - 1.0).astype(np.float32)
    if c > 1:
        top = np.sort(logits.astype(np.float64), 1)
        assert (top[:, -1] - top[:, -2]).min() >= 2.0 ** -6
    path = _decode(dec, logits, rows, start, 0.0)
    plain = _decode(dec, logits, rows, start, None, smooth=1)
    assert set(path) == set(plain) == {"first", "last", "cls", "score", "peak", "label", "conf"}
    for k in plain:
        assert path[k].dtype == plain[k].dtype and np.array_equal(path[k], plain[k]), k
    assert np.array_equal(path["label"], logits[np.clip(rows, 0, n - 1)].argmax(1))
    quiet = _decode(dec, logits, rows, start, 0.0, frames=False)                 # label_out / conf_out NULL: the handle's own buffers
    assert set(quiet) == {"first", "last", "cls", "score", "peak"} and all(np.array_equal(quiet[k], plain[k]) for k in quiet)


def test_planted_glitches_are_absorbed_and_boundaries_stay(dec):
    rng = np.random.default_rng(9)
    c = 11
    m = 2 * G + 3
    start = _layout(m, 1)                                                        # videos [0, 1) [1, 3) [3, G) [G, m)
    cuts = sorted({0, 1, 3, 7, 20, G - 5, G, G + 1, G + 9, 2 * G - 1, 2 * G, 2 * G + 1})      # segment starts, tile edges among them
    truth = np.zeros(m, np.int64)
    for i, (a, b) in enumerate(zip(cuts, cuts[1:] + [m])):
        truth[a:b] = (i * 4 + 1) % c
    assert np.all(truth[np.asarray(cuts[1:])] != truth[np.asarray(cuts[1:]) - 1])
    logits = np.zeros((m, c), np.float32)
    logits[np.arange(m), truth] = 4.0
    # isolated glitches: a wrong class leads by 1, never next to a boundary or another glitch
    glitches = [p for p in (10, 14, 30, G - 9, G + 4, G + 20, G + 40, 2 * G - 4) if all(abs(p - q) >= 2 for q in cuts + [m])]
    assert len(glitches) >= 6
    wrong = np.asarray([(truth[p] + 1 + int(rng.integers(0, c - 1))) % c for p in glitches])
    assert np.all(wrong != truth[glitches])
    logits[glitches, wrong] = 5.0
    from tennis_amd.events import label_runs
    for cost, want in ((1.0, truth), (0.0, None)):
        if want is None:
            want = truth.copy()
            want[glitches] = wrong
        got = _decode(dec, logits, np.arange(m), start, cost)
        first, last, cls = label_runs(want, start)
        assert np.array_equal(got["label"], want)
        assert np.array_equal(got["first"], first) and np.array_equal(got["last"], last) and np.array_equal(got["cls"], cls)
        if cost == 0.0:
            for p, w in zip(glitches, wrong):                                    # every glitch an event of its own
                i = int(np.searchsorted(got["first"], p))
                assert got["first"][i] == p and got["last"][i] == p and got["cls"][i] == w
        else:
            assert len(first) == len(cuts) and list(first) == cuts


PATH_CASES = [(m, c, cost) for m in (G + 1, 2 * G + 3) for c in (2, 11, 17, 64) for cost in (0.25, 2.0, 30.0)] + [(1, 11, 2.0), (2, 11, 2.0),
                                                                                                                   (G - 1, 1, 2.0), (G, 11, 2.0)]


@pytest.mark.parametrize("m,c,cost", PATH_CASES)
def test_the_path_of_general_logits_is_optimal_within_the_rounding_bound(dec, report, m, c, cost):
    """Random normal x 2 logits.  The float64 score of the returned path - the sum of exact emissions minus cost per switch - against
    the float64 optimum.  Bound (viterbi_ref.path_bound): every fp32 step rounds one emission, one addition and one normalisation,
    each on a value of at most cost + max|e|, so each off by at most 2^-24 (cost + max|e|); the fp32 run is an exact run on emissions
    moved by at most three such roundings, for which its path is optimal; any path's score moves by at most M times that, and two
    paths are compared: 2 M 3 2^-24 (cost + max|e|).  The returned path can never score above the optimum (beyond float64 noise)."""
    from tennis_amd.events import viterbi_labels
    seed = m * 1009 + c * 13 + int(cost * 4)
    rng = np.random.default_rng(seed)
    n, rows = _rows(rng, m, seed % 3)
    start = _layout(m, seed % 3 if m > 2 else 2)
    logits = (rng.normal(0, 1, (n, c)) * 2).astype(np.float32)
    got = _decode(dec, logits, rows, start, cost)
    e = VR.emissions(logits, rows)
    best = VR.optimum(e, start, cost)
    assert abs(VR.path_score(e, viterbi_labels(logits, rows, start, cost), start, cost) - best) <= 1e-9 * (1 + abs(best))
    mine = VR.path_score(e, got["label"], start, cost)
    bound = VR.path_bound(m, cost, np.abs(e).max())
    ratio = (best - mine) / bound
    key = "event_viterbi_path_m%d_c%d_cost%g_shortfall_over_bound" % (m, c, cost)
    print("%s: %.3g (optimum %.6f, returned path %.6f, bound %.3g)" % (key, ratio, best, mine, bound))
    report[key] = float(ratio)
    assert mine <= best + 1e-9 * (1 + abs(best))
    assert best - mine <= bound, ratio
    assert got["label"].min() >= 0 and got["label"].max() < c
    x = logits[np.clip(rows, 0, n - 1)].astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    assert np.all(np.abs(got["conf"] - p[np.arange(m), got["label"]]) <= ER.score_bound(c, 1))
    _check_events_of_own_frames(got, start)


def test_a_video_alone_gives_the_bits_of_the_joint_call():
    from tennis_amd.engine import EventDecoder
    rng = np.random.default_rng(5)
    c, cost = 11, 1.5
    lengths = [1, 2, G, G + 3, 5, 2 * G + 1, G - 1]
    m = sum(lengths)
    bounds = np.cumsum([0] + lengths)
    start = np.zeros(m, np.int32)
    start[bounds[:-1]] = 1
    n = m + 100
    logits = (rng.normal(0, 1, (n, c)) * 2).astype(np.float32)
    rows = rng.permutation(n)[:m]
    big, small = EventDecoder(m + 3 * G, 64), EventDecoder(m, 11)
    whole = _decode(big, logits, rows, start, cost)
    again = _decode(big, logits, rows, start, cost)
    other = _decode(small, logits, rows, start, cost)                            # a handle of another max_positions
    assert all(np.array_equal(whole[k], again[k]) and np.array_equal(whole[k], other[k]) for k in whole)
    assert len(set(whole["label"].tolist())) > 3 and len(whole["first"]) > len(lengths)
    for dec in (big, small):
        for a, b in zip(bounds[:-1], bounds[1:]):
            alone = _decode(dec, logits, rows[a:b], start[a:b], cost)
            assert np.array_equal(alone["label"], whole["label"][a:b]) and np.array_equal(alone["conf"], whole["conf"][a:b])
            sel = (whole["first"] >= a) & (whole["first"] < b)
            assert np.array_equal(alone["first"], whole["first"][sel] - a) and np.array_equal(alone["last"], whole["last"][sel] - a)
            for k in ("cls", "score", "peak"):
                assert np.array_equal(alone[k], whole[k][sel]), k


def test_nothing_changes_without_the_keyword():
    from tennis_amd.engine import EventDecoder
    rng = np.random.default_rng(6)
    m, c = 2 * G + 3, 11
    dec = EventDecoder(MAXPOS, 64)
    logits = (rng.normal(0, 1, (m, c)) * 2).astype(np.float32)
    start = _layout(m, 1)
    created = dec.workspace_bytes()
    assert created >= 9 * MAXPOS
    before = {w: _decode(dec, logits, np.arange(m), start, None, smooth=w) for w in (1, 9)}
    assert dec.workspace_bytes() == created                                      # decode(smooth=...) allocates nothing in the handle
    _decode(dec, logits, np.arange(m), start, 2.0)
    grown = dec.workspace_bytes()
    assert grown >= created + 9 * MAXPOS                                         # 8 bytes of stay mask and 1 of a_t per position, the bounds
    _decode(dec, logits, np.arange(m), start, 0.5)
    assert dec.workspace_bytes() == grown                                        # only the first call allocates
    for w in (1, 9):
        after = _decode(dec, logits, np.arange(m), start, None, smooth=w)
        assert all(np.array_equal(before[w][k], after[k]) for k in after)
    assert dec.workspace_bytes() == grown


def test_refusals(dec):
    from tennis_amd import _lib
    lib = _lib.load()
    P = _lib.ptr
    m, n, c = 16, 16, 11
    lg = torch.zeros((n, c), device="cuda")
    iv = torch.zeros(m, dtype=torch.int32, device="cuda")
    ev = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.zeros(m, device="cuda") for _ in range(2)]
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")

    def run(**k):
        a = dict(h=dec.handle, logits=P(lg), N=n, C=c, rows=P(iv), start=P(iv), M=m, cost=1.0, first=P(ev[0]), last=P(ev[1]), cls=P(ev[2]),
                 score=P(ev[3]), peak=P(ev[4]), count=P(cnt))
        a.update(k)
        return lib.tn_event_decoder_run_switch(a["h"], a["logits"], a["N"], a["C"], a["rows"], a["start"], a["M"], a["cost"], None, None,
                                               a["first"], a["last"], a["cls"], a["score"], a["peak"], a["count"], None)
    for bad, word in ((dict(cost=-0.5), b"switch_cost"), (dict(cost=float("nan")), b"switch_cost"), (dict(cost=float("inf")), b"switch_cost"),
                      (dict(cost=float("-inf")), b"switch_cost"), (dict(h=None), b"handle"), (dict(logits=None), b"logits"),
                      (dict(rows=None), b"rows"), (dict(start=None), b"start"), (dict(first=None), b"ev_first"), (dict(count=None), b"count"),
                      (dict(C=65), b"C "), (dict(C=0), b"C "), (dict(M=dec.max_positions + 1), b"max_positions"), (dict(M=0), b"M "),
                      (dict(N=0), b"N ")):
        assert run(**bad) == -1, bad
        assert word in lib.tn_last_error() and b"tn_event_decoder_run_switch" in lib.tn_last_error(), (bad, lib.tn_last_error())
    torch.cuda.synchronize()
    assert int(cnt.item()) == -7                                                 # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == 1                                                  # all-zero logits, one video: one event
    x = torch.zeros((n, c), device="cuda")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="switch_cost"):
            dec.decode(x, np.arange(m), np.zeros(m), switch_cost=bad)
    calls = []
    with pytest.MonkeyPatch.context() as mp:                                     # refused in front of every entry of the library
        mp.setattr(dec, "lib", _Spy(dec.lib, calls))
        with pytest.raises(ValueError, match="smooth=3"):
            dec.decode(x, np.arange(m), np.zeros(m), smooth=3, switch_cost=1.0)
        with pytest.raises(ValueError, match="switch_cost"):
            dec.decode(x, np.arange(m), np.zeros(m), switch_cost=-2.0)
    assert calls == []
    small = C.c_void_p()
    assert lib.tn_event_decoder_create(dec.ctx.handle, 8, 4, C.byref(small)) == 0
    try:
        size = C.c_size_t()
        assert lib.tn_dbg_event_decoder_workspace_bytes(small, C.byref(size)) == 0 and size.value >= 72
        assert lib.tn_event_decoder_run_switch(small, P(lg), n, c, P(iv), P(iv), 8, 1.0, None, None, P(ev[0]), P(ev[1]), P(ev[2]), P(ev[3]),
                                               P(ev[4]), P(cnt), None) == -1 and b"max_classes" in lib.tn_last_error()
    finally:
        assert lib.tn_event_decoder_destroy(small) == 0
    torch.cuda.synchronize()
