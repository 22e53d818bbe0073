"""-m gpu: event scores from HMM posteriors (csrc/event_runs.hip: hmm_chain_kernel, hmm_posterior_kernel; tn_event_decoder_run_posteriors,
engine.EventDecoder.decode(posteriors=True)) against their definition in float64 (events.hmm_posteriors, held to brute force by
tests/test_cpu_event_posteriors.py).

The bar on max |posterior - float64| is not fixed in advance: BAR = 8 x the largest error of the definition's own float32 run
(hmm_posteriors(dtype=float32)) against its float64 run over EVERY input of this file, the extreme ones included - measured on the
host, from the oracle alone (the kernel uses the hardware's exp2 / log2 where numpy has its own, and may sum the last softmax in
another order).  Every test prints its own figures next to it; docs/numerics.md holds both.
Rows of the posterior sum to 1 within (C + 1) 2^-23 in float64: one rounded division per entry over a fixed-order fp32 sum of C
terms."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tools.event_paths import Spy as _Spy
from tools.event_paths import check_events_of_own_frames as _check_events_of_own_frames
from tools.event_paths import rows_of as _rows

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 129, 200]                                           # tile (64) and chunk (8) edges, in one call
CLASSES = [1, 2, 11, 16, 17, 64]                                                 # both instantiations and their edges
KINDS = ["planted", "potts", "holes"]
EXTREME = [3, 17]
MANY = 1100
MAXPOS = 3 * MANY


def _starts(lengths):
    bounds = np.cumsum([0] + list(lengths))
    start = np.zeros(bounds[-1], np.int32)
    start[bounds[:-1]] = 1
    return start, bounds


def _matrix(rng, c, kind, start):
    from tennis_amd.events import transition_scores
    if kind == "potts":
        return (-2.0 * (1 - np.eye(c))).astype(np.float32)
    if kind == "holes":
        t = (-3.0 * rng.random((c, c))).astype(np.float32)
        t[(rng.random((c, c)) < 0.25) & ~np.eye(c, dtype=bool)] = -np.inf
        t[np.arange(c), np.arange(c)] = -0.125
        return t
    planted = np.repeat(rng.integers(0, c, len(start) // 7 + 1), 7)[:len(start)]   # runs of seven positions
    return transition_scores(planted, start, c)


def _finish(logits, rows, start, trans):
    """the inputs with their float64 posteriors and the float32 oracle's error against them, computed once and left unchanged"""
    from tennis_amd.events import hmm_posteriors
    g64 = hmm_posteriors(logits, rows, start, trans)
    g32 = hmm_posteriors(logits, rows, start, trans, dtype=np.float32)
    assert g32.dtype == np.float32 and np.all(np.isfinite(g64)) and np.all(np.isfinite(g32))
    err32 = float(np.abs(g32.astype(np.float64) - g64).max())
    for arr in (logits, rows, start, trans, g64):
        arr.setflags(write=False)
    return logits, rows, start, trans, g64, err32


@functools.lru_cache(maxsize=None)
def _case(c, kind):
    seed = CLASSES.index(c) * 5 + KINDS.index(kind)
    rng = np.random.default_rng(seed)
    start, _ = _starts(LENGTHS)
    n, rows = _rows(rng, len(start), 2)                                          # permuted, every fifth outside [0, N): clamped
    logits = (rng.normal(0, 1, (n, c)) * 3).astype(np.float32)
    return _finish(logits, rows, start, _matrix(rng, c, kind, start))


@functools.lru_cache(maxsize=None)
def _extreme(c):
    """gaps of 200 between the logits, and the frames ask for 0 -> 1, which the matrix forbids; also 1 -> 0 -> 1 glitches"""
    lengths = [131, 1, 2, 66]
    start, bounds = _starts(lengths)
    m = len(start)
    trans = np.full((c, c), -0.5, np.float32)
    trans[np.arange(c), np.arange(c)] = 0.0
    trans[0, 1] = -np.inf
    if c > 3:
        trans[1, 3:] = -np.inf
    logits = np.zeros((m, c), np.float32)
    for a, b in zip(bounds[:-1], bounds[1:]):
        cut = a + (b - a) // 2
        logits[a:cut, 0] = 200.0
        logits[cut:b, 1] = 200.0
    logits[[7, 62, 63, 100], 2] = 400.0
    logits[70, 0] = -200.0
    return _finish(logits, np.arange(m), start, trans)


@functools.lru_cache(maxsize=None)
def _many():
    """more chains than the chain kernel's grid: it loops"""
    rng = np.random.default_rng(77)
    c = 11
    start, _ = _starts(rng.integers(1, 4, MANY))
    m = len(start)
    logits = (rng.normal(0, 1, (m, c)) * 3).astype(np.float32)
    return _finish(logits, rng.permutation(m).astype(np.int64), start, _matrix(rng, c, "holes", start))


@functools.lru_cache(maxsize=None)
def _bar():
    """(8 x the float32 oracle's largest error over every input of this file, that error)"""
    errs = [_case(c, k)[5] for c in CLASSES for k in KINDS] + [_extreme(c)[5] for c in EXTREME] + [_many()[5]]
    worst = max(errs)
    assert worst > 0
    return 8 * worst, worst


@pytest.fixture(scope="module")
def decs():
    """max_classes -> handle: 16 runs the one-row instantiation, 64 the other"""
    from tennis_amd.engine import EventDecoder
    return {16: EventDecoder(MAXPOS, 16), 64: EventDecoder(MAXPOS, 64)}


def _handles(decs, c):
    return [decs[k] for k in (16, 64) if c <= k]


def _decode(dec, logits, rows, start, **kw):
    return dec.decode(torch.tensor(np.asarray(logits, np.float32), device="cuda"), np.array(rows), np.array(start), return_frames=True, **kw)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _check(dec, case, report, key):
    """assertions 1, 2 and 5 of one call on one handle -> its output"""
    logits, rows, start, trans, g64, err32 = case
    m, c = g64.shape
    bar, worst32 = _bar()
    got = _np(_decode(dec, logits, rows, start, transitions=trans, return_posteriors=True))
    post = got["posterior"]
    assert post.shape == (m, c) and post.dtype == np.float32 and np.all(np.isfinite(post)) and np.all(np.isfinite(got["conf"]))
    assert post.min() >= 0 and post.max() <= 1
    err = float(np.abs(post.astype(np.float64) - g64).max())
    rowsum = float(np.abs(post.astype(np.float64).sum(1) - 1).max())
    print("%s: kernel max|err| %.3g, float32 oracle on these inputs %.3g, bar %.3g (8 x %.3g); rows sum to 1 within %.3g (bound %.3g)"
          % (key, err, err32, bar, worst32, rowsum, (c + 1) * 2.0 ** -23))
    report[key + "_err"] = err
    report[key + "_oracle32_err"] = err32
    assert err <= bar, (err, bar)
    assert rowsum <= (c + 1) * 2.0 ** -23, rowsum
    # the path does not move, and the events are scored with gamma
    plain = _np(_decode(dec, logits, rows, start, transitions=trans))
    for k in ("label", "first", "last", "cls"):
        assert got[k].dtype == plain[k].dtype and np.array_equal(got[k], plain[k]), k
    assert np.array_equal(got["conf"], post[np.arange(m), got["label"]])
    _check_events_of_own_frames(got, start)                                      # peak the exact maximum, score within mean_bound
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", CLASSES)
def test_posteriors_against_float64(decs, report, c, kind):
    case = _case(c, kind)
    assert list(np.diff(np.append(np.flatnonzero(case[2]), len(case[2])))) == LENGTHS
    assert (case[1] < 0).any() and (case[1] >= len(case[0])).any()
    if kind == "holes" and c > 2:
        assert np.isneginf(case[3]).any()
    for dec in _handles(decs, c):
        got = _check(dec, case, report, "event_posteriors_c%d_%s_h%d" % (c, kind, dec.classes))
        if c > 1 and kind != "potts":
            assert np.abs(got["conf"] - _np(_decode(dec, *case[:3], transitions=case[3]))["conf"]).max() > 1e-3      # not the frame's softmax


@pytest.mark.parametrize("c", EXTREME)
def test_extreme_logits_against_a_forbidding_matrix(decs, report, c):
    case = _extreme(c)
    logits, _, start, trans = case[:4]
    q = logits.argmax(1)
    assert ((q[:-1] == 0) & (q[1:] == 1) & (start[1:] == 0)).sum() >= 3 and np.isneginf(trans[0, 1])      # the frames ask for 0 -> 1
    top = np.sort(logits, 1)
    assert (top[:, -1] - top[:, -2]).min() >= 200
    for dec in _handles(decs, c):
        got = _check(dec, case, report, "event_posteriors_extreme_c%d_h%d" % (c, dec.classes))
        assert np.all(np.isfinite(got["score"])) and np.all(np.isfinite(got["peak"]))
        lab = got["label"]
        assert not ((lab[:-1] == 0) & (lab[1:] == 1) & (start[1:] == 0)).any()


def test_more_chains_than_the_grid(decs, report):
    case = _many()
    assert int(case[2].sum()) == MANY and 2 * MANY > 1024
    for dec in _handles(decs, 11):
        _check(dec, case, report, "event_posteriors_many_h%d" % dec.classes)


def test_a_video_alone_gives_the_bits_of_the_joint_call():
    from tennis_amd.engine import EventDecoder
    logits, rows, start, trans, _, _ = _case(11, "holes")
    bounds = np.append(np.flatnonzero(start), len(start))
    for classes in (16, 64):
        big, small = EventDecoder(len(start) + 200, classes), EventDecoder(200, classes)      # posteriors are the handles' first call
        whole = _decode(big, logits, rows, start, transitions=trans, return_posteriors=True)
        again = _decode(big, logits, rows, start, transitions=trans, return_posteriors=True)
        assert all(torch.equal(whole[k], again[k]) for k in whole)
        for a, b in zip(bounds[:-1], bounds[1:]):
            alone = _decode(small, logits, rows[a:b], start[a:b], transitions=trans, return_posteriors=True)
            assert torch.equal(alone["posterior"], whole["posterior"][a:b]) and torch.equal(alone["conf"], whole["conf"][a:b])
            assert torch.equal(alone["label"], whole["label"][a:b])
    quiet = big.decode(torch.tensor(logits, device="cuda"), np.array(rows), np.array(start), transitions=trans, posteriors=True)      # posterior NULL, own frames
    assert set(quiet) == {"first", "last", "cls", "score", "peak"} and all(torch.equal(quiet[k], whole[k]) for k in quiet)


@pytest.mark.parametrize("c", [2, 11, 17])
def test_the_switch_cost_goes_through_its_matrix(decs, c):
    """dyadic logits (multiples of 2^-6 in [-16, 16]) and a dyadic cost: the recurrence of the path is exact in fp32, so the path under
    -cost (1 - I) is the switch-cost decoder's at every position, ties included"""
    rng = np.random.default_rng(c)
    cost = 1.75
    start, _ = _starts(LENGTHS)
    m = len(start)
    logits = (rng.integers(-1024, 1025, (m, c)) / 64.0).astype(np.float32)
    potts = (-cost * (1 - np.eye(c))).astype(np.float32)
    for dec in _handles(decs, c):
        got = _decode(dec, logits, np.arange(m), start, switch_cost=cost, return_posteriors=True)
        plain = _decode(dec, logits, np.arange(m), start, switch_cost=cost)
        for k in ("label", "first", "last", "cls"):
            assert torch.equal(got[k], plain[k]), k
        same = _decode(dec, logits, np.arange(m), start, transitions=potts, return_posteriors=True)
        assert set(same) == set(got) and all(torch.equal(got[k], same[k]) for k in got)
        assert torch.equal(got["conf"], got["posterior"][torch.arange(m), got["label"].long()])


@pytest.mark.parametrize("classes", [16, 64])
def test_nothing_changes_without_the_keyword(classes):
    from tennis_amd.engine import EventDecoder, event_decoder_transition_geometry
    _, p16, p64 = event_decoder_transition_geometry()
    pitch = p16 if classes <= 16 else p64
    logits, rows, start, trans, _, _ = _case(11, "planted")
    maxpos = len(start) + 3                                                      # (no multiple of 4)
    dec = EventDecoder(maxpos, classes)
    calls = {"smooth1": dict(smooth=1), "smooth9": dict(smooth=9), "switch2": dict(switch_cost=2.0), "transitions": dict(transitions=trans)}
    before = {k: _decode(dec, logits, rows, start, **kw) for k, kw in calls.items()}
    held = dec.workspace_bytes()
    assert _decode(dec, logits, rows, start, transitions=trans) and dec.workspace_bytes() == held
    first = _decode(dec, logits, rows, start, transitions=trans, return_posteriors=True)
    grown = dec.workspace_bytes()
    assert grown == held + 2 * maxpos * pitch * 4
    second = _decode(dec, logits, rows, start, transitions=trans, posteriors=True)
    assert dec.workspace_bytes() == grown                                        # only the first call allocates
    assert "posterior" not in second and all(torch.equal(first[k], second[k]) for k in second)
    for k, kw in calls.items():
        after = _decode(dec, logits, rows, start, **kw)
        assert set(after) == set(before[k]) and all(torch.equal(before[k][key], after[key]) for key in after), k
    assert dec.workspace_bytes() == grown


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

    def run(trans, h=dec.handle):
        t = None if trans is None else np.ascontiguousarray(trans, np.float32).ctypes.data_as(C.c_void_p)
        return lib.tn_event_decoder_run_posteriors(h, P(lg), n, c, P(iv), P(iv), m, t, None, None, None, P(ev[0]), P(ev[1]), P(ev[2]), P(ev[3]),
                                                   P(ev[4]), P(cnt), None)
    bad = good.copy()
    bad[4, 1] = 0.5
    for args, word in (((None,), b"transitions is null"), ((bad,), b"transitions[4][1] is positive"), ((good, None), b"handle")):
        assert run(*args) == -1
        assert word in lib.tn_last_error() and b"tn_event_decoder_run_posteriors" in lib.tn_last_error(), lib.tn_last_error()
    torch.cuda.synchronize()
    assert int(cnt.item()) == -7                                                 # nothing was launched
    assert run(good) == 0                                                        # posterior, label_out and conf_out NULL
    torch.cuda.synchronize()
    assert int(cnt.item()) == 1                                                  # all-zero logits, one video: one event
    assert float(ev[3][0]) == pytest.approx(1 / c, abs=1e-6)                     # ... whose every class is as likely as another
    x = torch.zeros((n, c), device="cuda")
    calls = []
    with pytest.MonkeyPatch.context() as mp:                                     # refused in front of every entry of the library
        mp.setattr(dec, "lib", _Spy(dec.lib, calls))
        for kw in (dict(posteriors=True), dict(return_posteriors=True)):
            with pytest.raises(ValueError, match="give transitions or switch_cost"):
                dec.decode(x, np.arange(m), np.zeros(m), **kw)
            with pytest.raises(ValueError, match="smooth=3"):
                dec.decode(x, np.arange(m), np.zeros(m), smooth=3, **kw)
            with pytest.raises(ValueError, match="smooth=3"):
                dec.decode(x, np.arange(m), np.zeros(m), smooth=3, transitions=good, **kw)
            with pytest.raises(ValueError, match="smooth=3"):
                dec.decode(x, np.arange(m), np.zeros(m), smooth=3, switch_cost=1.0, **kw)
    assert calls == []
