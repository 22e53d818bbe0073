"""-m gpu: the event decoder (csrc/event_runs.hip, tn_event_decoder_*, engine.EventDecoder) against its definitions restated in
float64 (tests/tools/events_ref.py).  Shapes are placed from the decoder's own geometry (tn_dbg_event_decoder_geometry): R positions
per workgroup of the score kernel, S tile counts per step of the scan workgroup.

Bounds, derived (u = 2^-24, every probability and score is at most 1, so the bounds are absolute):
  score  (C + width + 8) u : the softmax costs the subtraction of the maximum (1), expf (2 ulp assumed), the C - 1 additions of the
         denominator and the division (1); the window adds width - 1 additions and a division; two spare.
  mean   (ceil(len / 64) + 7) u on top of the confs' own error: ceil(len / 64) - 1 additions per lane, six tree levels, the division,
         one spare.  The peak is a maximum: exact given the confs.
Labels are compared where the reference's margin between its best and second score exceeds twice the score bound; the share of
positions left out is asserted on the reference first (at most 1 %: a condition on the inputs, not a tolerance)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tools import events_ref as ER

pytestmark = pytest.mark.gpu


def _geometry():
    from tennis_amd.engine import event_decoder_geometry
    return event_decoder_geometry()


R, S = _geometry()
BIG = (S + 1) * R + 5                  # more than S tiles of flags: the scan workgroup takes a second step
SIZES = [1, 2, R - 1, R, R + 1, 2 * R + 3]
CLASSES = [1, 2, 11, 64]
WIDTHS = [1, 3, 9, 63]


@pytest.fixture(scope="module")
def dec():
    from tennis_amd.engine import EventDecoder
    return EventDecoder(BIG, 64)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _decode(dec, logits, rows, start, width, frames=True):
    return _np(dec.decode(torch.tensor(np.asarray(logits, np.float32), device="cuda"), np.array(rows), np.array(start), smooth=width,
                          return_frames=frames))


def _starts(rng, m, width):
    """video boundaries: lengths 1 and 2 in front, then one shorter than the window, then random ones"""
    start = (rng.random(m) < 0.08).astype(np.int32)
    start[0] = 0                                                                 # (position 0 begins a video whatever its flag says)
    for at in (1, 3, 3 + max(width - 1, 1)):
        if at < m:
            start[at] = 1
    return start


@functools.lru_cache(maxsize=None)
def _random_case(m, c, width):
    """random logits (standard normal x 2, x 4 at 64 classes), rows by turns the identity, a permutation of a larger N, and with
    entries outside [0, N); the float64 reference, computed once and shared"""
    seed = m * 10007 + c * 101 + width
    rng = np.random.default_rng(seed)
    mode = seed % 3
    n = m if mode == 0 else m + 37
    logits = (rng.normal(0, 1, (n, c)) * (4.0 if c == 64 else 2.0)).astype(np.float32)
    rows = np.arange(m) if mode == 0 else rng.permutation(n)[:m]
    if mode == 2:
        rows = rows.copy()
        rows[::5] = rng.choice([-3, -1, n, n + 9, 2 ** 31 - 1, -2 ** 31], len(rows[::5]))
    start = _starts(rng, m, width)
    ref = ER.decode_ref(logits, rows, start, width)
    for a in (logits, rows, start, *ref.values()):
        a.setflags(write=False)
    return logits, rows.astype(np.int64), start, ref


def _check_against_ref(got, ref, start, c, width, report=None, key=None):
    """scores within the bound, labels where the margin allows, and the events of the decoder's OWN labels and confs exactly"""
    m = len(ref["label"])
    bound = ER.score_bound(c, width)
    safe = ref["margin"] > 2 * bound
    assert (~safe).sum() <= 0.01 * m, "the inputs leave more than 1 %% of the positions too close to call: %d of %d" % ((~safe).sum(), m)
    assert got["label"].shape == (m,) and got["conf"].shape == (m,)
    assert got["label"].min() >= 0 and got["label"].max() < c
    err = np.abs(got["conf"].astype(np.float64) - ref["score"][np.arange(m), got["label"]])
    ratio = float(err.max() / bound)
    if key:
        print("%s: measured / bound = %.3f (max err %.3g, bound %.3g)" % (key, ratio, err.max(), bound))
        report[key] = ratio
    assert np.all(err <= bound), ratio
    assert np.array_equal(got["label"][safe], ref["label"][safe])
    # the events are the runs of the decoder's own labels, with the peak and mean of its own confs
    from tennis_amd.events import label_runs
    first, last, cls = label_runs(got["label"], start)
    assert np.array_equal(got["first"], first) and np.array_equal(got["last"], last) and np.array_equal(got["cls"], cls)
    conf64 = got["conf"].astype(np.float64)
    for a, b, sc, pk in zip(first, last, got["score"], got["peak"]):
        assert pk == got["conf"][a:b + 1].max()
        assert abs(float(sc) - conf64[a:b + 1].mean()) <= ER.mean_bound(b - a + 1)
    return ratio


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("m", SIZES)
def test_scores_labels_and_runs_against_float64(dec, report, m, c, width):
    logits, rows, start, ref = _random_case(m, c, width)
    got = _decode(dec, logits, rows, start, width)
    _check_against_ref(got, ref, start, c, width, report, "event_runs_m%d_c%d_w%d_err_over_bound" % (m, c, width))
    assert 0.5 ** 0.5 > 100 * ER.score_bound(c, width)                          # (the bound discriminates: scores are of order 1 / C .. 1)


@pytest.mark.parametrize("mode", ["identity", "permutation", "out_of_range"])
def test_rows_select_permute_and_clamp(dec, mode):
    rng = np.random.default_rng(7)
    m, c, width = 2 * R + 3, 11, 9
    n = m if mode == "identity" else 3 * m
    logits = (rng.normal(0, 1, (n, c)) * 2).astype(np.float32)
    rows = np.arange(m) if mode == "identity" else rng.permutation(n)[:m]
    if mode == "out_of_range":
        rows[::3] = rng.choice([-7, -1, n, n + 1, 2 ** 31 - 1, -2 ** 31], len(rows[::3]))
    start = _starts(rng, m, width)
    got = _decode(dec, logits, rows, start, width)
    _check_against_ref(got, ER.decode_ref(logits, rows, start, width), start, c, width)
    # the same list spelled with clamped rows, and gathered on the host, gives the same bits
    clamped = np.clip(rows, 0, n - 1)
    for other in (_decode(dec, logits, clamped, start, width), _decode(dec, logits[clamped], np.arange(m), start, width)):
        assert all(np.array_equal(got[k], other[k]) for k in got)


def test_video_layouts(dec):
    """videos of length 1, of length 2, shorter than the window, ending exactly on a tile edge, and one video over everything"""
    rng = np.random.default_rng(11)
    c, width = 11, 9
    m = 3 * R
    logits = (rng.normal(0, 1, (m, c)) * 2).astype(np.float32)
    start = np.zeros(m, np.int32)
    start[[0, 1, 3, 3 + width - 2, R, 2 * R - 1, 2 * R]] = 1                     # lengths 1, 2, width - 2, ..., up to the edges R and 2 R
    for st in (start, np.zeros(m, np.int32)):
        got = _decode(dec, logits, np.arange(m), st, width)
        _check_against_ref(got, ER.decode_ref(logits, np.arange(m), st, width), st, c, width)


def _planted(name, m, c):
    lab, start = np.zeros(m, np.int64), np.zeros(m, np.int32)
    if name == "every_position_its_own_run":
        lab = (np.arange(m) % 2) * min(3, c - 1)
    elif name == "one_run":
        lab[:] = c - 1
    elif name == "runs_on_tile_edges":
        lab = (np.arange(m) // R) % c
    elif name == "same_label_across_videos":
        lab[:] = 1 % c
        start[[R, R + 5]] = 1
    elif name == "run_across_tiles":
        lab[10:2 * R + 50] = 1 % c
    elif name == "short_runs":
        lab = (np.arange(m) // 7) % 2
    return lab, start


PLANTED = [("every_position_its_own_run", 2 * R + 3, 11, 1), ("every_position_its_own_run", 2 * R + 3, 2, 1), ("one_run", 2 * R + 3, 11, 9),
           ("one_run", BIG, 2, 3), ("short_runs", BIG, 2, 3), ("runs_on_tile_edges", 3 * R, 11, 1), ("runs_on_tile_edges", 3 * R, 11, 9),
           ("same_label_across_videos", 3 * R, 11, 9), ("run_across_tiles", 3 * R, 11, 1), ("run_across_tiles", 3 * R, 64, 63)]


@pytest.mark.parametrize("name,m,c,width", PLANTED, ids=["%s_m%d_c%d_w%d" % p for p in PLANTED])
def test_planted_events_exactly(dec, report, name, m, c, width):
    rng = np.random.default_rng(len(name) + m + c + width)
    lab, start = _planted(name, m, c)
    logits = np.zeros((m, c), np.float32)
    logits[np.arange(m), lab] = 8.0
    logits += rng.normal(0, 0.1, (m, c)).astype(np.float32)
    rows = np.arange(m)
    ref = ER.decode_ref(logits, rows, start, width)
    assert ref["margin"].min() > 1e-2                                            # no close calls
    if width == 1:
        assert np.array_equal(ref["label"], lab)
    got = _decode(dec, logits, rows, start, width, frames=False)
    assert set(got) == {"first", "last", "cls", "score", "peak"}
    k = len(ref["first"])
    assert len(got["first"]) == k and got["first"].dtype == np.int32 and got["score"].dtype == np.float32
    assert np.array_equal(got["first"], ref["first"]) and np.array_equal(got["last"], ref["last"]) and np.array_equal(got["cls"], ref["cls"])
    if name == "every_position_its_own_run" and width == 1:
        assert k == m
    if name == "one_run":
        assert k == 1 and got["last"][0] == m - 1
    if name == "same_label_across_videos":
        assert k == 3 and list(got["first"]) == [0, R, R + 5] and len(set(got["cls"])) == 1
    length = ref["last"] - ref["first"] + 1
    sb = ER.score_bound(c, width)
    e_peak = np.abs(got["peak"].astype(np.float64) - ref["ev_peak"])
    e_score = np.abs(got["score"].astype(np.float64) - ref["ev_score"])
    mb = np.asarray([ER.mean_bound(int(n)) for n in length])
    key = "event_runs_planted_%s_m%d_c%d_w%d" % (name, m, c, width)
    report[key + "_peak_err_over_bound"] = float(e_peak.max() / sb)
    report[key + "_score_err_over_bound"] = float((e_score / (sb + mb)).max())
    print("%s: peak %.3f, score %.3f of their bounds" % (key, report[key + "_peak_err_over_bound"], report[key + "_score_err_over_bound"]))
    assert np.all(e_peak <= sb) and np.all(e_score <= sb + mb)


def test_ties_are_exact(dec):
    rng = np.random.default_rng(3)
    m, c = 2 * R + 3, 11
    rows = np.arange(m)
    start = np.zeros(m, np.int32)
    start[[5, 6, R, R + 40]] = 1
    videos = [0, 5, 6, R, R + 40]
    for width in (1, 3, 63):
        # all-zero logits: class 0 everywhere, one event per video
        got = _decode(dec, np.zeros((m, c)), rows, start, width)
        assert not got["label"].any() and list(got["first"]) == videos and not got["cls"].any()
        assert np.all(np.abs(got["conf"] - 1 / c) <= ER.score_bound(c, width))
        # two classes with identical logit columns: the smaller index
        x = (rng.normal(0, 1, (m, c)) * 2).astype(np.float32)
        x[:, 2] = x[:, 7] = 10.0
        got = _decode(dec, x, rows, start, width)
        assert np.all(got["label"] == 2) and list(got["first"]) == videos
        # identical rows: the labels of width 1 under any width
        row = (rng.normal(0, 1, c) * 2).astype(np.float32)
        got = _decode(dec, np.tile(row, (m, 1)), rows, start, width)
        one = _decode(dec, np.tile(row, (m, 1)), rows, start, 1)
        assert np.array_equal(got["label"], one["label"]) and np.all(got["label"] == int(np.argmax(row)))


def test_bit_identity(dec):
    rng = np.random.default_rng(5)
    c, width = 11, 9
    lengths = [1, 2, 200, R + 77, 50, R]
    m = sum(lengths)
    bounds = np.cumsum([0] + lengths)
    start = np.zeros(m, np.int32)
    start[bounds[:-1]] = 1
    n = m + 100
    logits = (rng.normal(0, 1, (n, c)) * 2).astype(np.float32)
    rows = rng.permutation(n)[:m]
    whole = _decode(dec, logits, rows, start, width)
    again = _decode(dec, logits, rows, start, width)
    assert all(np.array_equal(whole[k], again[k]) for k in whole)                # two calls on one input
    quiet = _decode(dec, logits, rows, start, width, frames=False)               # label_out / conf_out NULL: the handle's own buffers
    assert all(np.array_equal(whole[k], quiet[k]) for k in quiet)
    for a, b in zip(bounds[:-1], bounds[1:]):                                    # a video decoded alone = its slice of the whole call
        alone = _decode(dec, logits, rows[a:b], start[a:b], width)
        assert np.array_equal(alone["label"], whole["label"][a:b]) and np.array_equal(alone["conf"], whole["conf"][a:b])
        sel = (whole["first"] >= a) & (whole["first"] < b)
        assert np.array_equal(alone["first"], whole["first"][sel] - a) and np.array_equal(alone["last"], whole["last"][sel] - a)
        for k in ("cls", "score", "peak"):
            assert np.array_equal(alone[k], whole[k][sel]), k
    # width 1 is the softmax's bits with no division: a window cut down to one position (every position a video of its own) under
    # any width gives the same conf, and so does the maximum of the probabilities themselves, read out through a one-hot follow-up
    one = _decode(dec, logits, rows, start, 1)
    cut = _decode(dec, logits, rows, np.ones(m, np.int32), 63)
    assert np.array_equal(one["conf"], cut["conf"]) and np.array_equal(one["label"], cut["label"])
    x64 = logits[rows].astype(np.float64)
    p64 = np.exp(x64 - x64.max(1, keepdims=True))
    p64 /= p64.sum(1, keepdims=True)
    assert np.array_equal(one["label"], p64.argmax(1)) or (np.sort(p64, 1)[:, -1] - np.sort(p64, 1)[:, -2]).min() < 2 * ER.score_bound(c, 1)
    assert np.all(np.abs(one["conf"] - p64.max(1)) <= ER.score_bound(c, 1))


def test_refusals_name_the_argument(dec):
    from tennis_amd import _lib
    lib = _lib.load()
    P = _lib.ptr
    m, n, c = 16, 16, 11
    lg = torch.zeros((n, c), device="cuda")
    iv = torch.zeros(m, dtype=torch.int32, device="cuda")
    ev = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.zeros(m, device="cuda") for _ in range(2)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(**k):
        a = dict(h=dec.handle, logits=P(lg), N=n, C=c, rows=P(iv), start=P(iv), M=m, width=3, first=P(ev[0]), last=P(ev[1]), cls=P(ev[2]),
                 score=P(ev[3]), peak=P(ev[4]), count=P(cnt))
        a.update(k)
        return lib.tn_event_decoder_run(a["h"], a["logits"], a["N"], a["C"], a["rows"], a["start"], a["M"], a["width"], None, None, a["first"],
                                        a["last"], a["cls"], a["score"], a["peak"], a["count"], None)
    assert run() == 0
    for bad, word in ((dict(h=None), b"handle"), (dict(logits=None), b"logits"), (dict(rows=None), b"rows"), (dict(start=None), b"start"),
                      (dict(first=None), b"ev_first"), (dict(last=None), b"ev_last"), (dict(cls=None), b"ev_cls"),
                      (dict(score=None), b"ev_score"), (dict(peak=None), b"ev_peak"), (dict(count=None), b"count"), (dict(C=65), b"C "),
                      (dict(C=0), b"C "), (dict(width=4), b"width"), (dict(width=65), b"width"), (dict(width=0), b"width"),
                      (dict(width=-1), b"width"), (dict(M=dec.max_positions + 1), b"max_positions"), (dict(M=0), b"M "), (dict(N=0), b"N "),
                      (dict(N=-4), b"N ")):
        assert run(**bad) == -1, bad
        assert word in lib.tn_last_error(), (bad, lib.tn_last_error())
    assert b"odd" in (run(width=4), lib.tn_last_error())[1]
    small = C.c_void_p()
    assert lib.tn_event_decoder_create(dec.ctx.handle, 8, 4, C.byref(small)) == 0
    try:
        assert lib.tn_event_decoder_run(small, P(lg), n, c, P(iv), P(iv), 8, 3, None, None, P(ev[0]), P(ev[1]), P(ev[2]), P(ev[3]), P(ev[4]),
                                        P(cnt), None) == -1 and b"max_classes" in lib.tn_last_error()
    finally:
        assert lib.tn_event_decoder_destroy(small) == 0
    for args, word in (((None, 8, 4, C.byref(small)), b"ctx"), ((dec.ctx.handle, 0, 4, C.byref(small)), b"max_positions"),
                       ((dec.ctx.handle, 8, 65, C.byref(small)), b"max_classes"), ((dec.ctx.handle, 8, 4, None), b"out")):
        assert lib.tn_event_decoder_create(*args) == -1 and word in lib.tn_last_error(), word
    torch.cuda.synchronize()
