"""No GPU: ``events.hmm_posteriors`` (the host restatement of the posteriors behind ``EventDecoder.decode(..., posteriors=True)``)
against the brute-force marginals over every label path, its two closed forms, the order of its sums, the refusals of
``--event_posteriors``, ``decode_split`` and ``save_events``, the ``posteriors`` column and the ABI surface."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _emissions(logits, rows):
    q = np.asarray(logits, np.float64)[np.clip(rows, 0, len(logits) - 1)]
    return q - q.max(1, keepdims=True)


def _softmax(x):
    x = np.asarray(x, np.float64)
    p = np.exp(x - x.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def _brute_force(e, trans):
    """the marginals of one video from all C^L paths, weight exp(sum_t e[t, l_t] + sum_{t > 0} T[l_{t-1}, l_t]), in float64"""
    n, c = e.shape
    trans = np.asarray(trans, np.float64)
    paths = list(itertools.product(range(c), repeat=n))
    score = np.asarray([sum(e[t, l] for t, l in enumerate(p)) + sum(trans[a, b] for a, b in zip(p, p[1:])) for p in paths])
    w = np.exp(score - score.max())
    gamma = np.zeros((n, c))
    for p, x in zip(paths, w):
        for t, l in enumerate(p):
            gamma[t, l] += x
    return gamma / w.sum()


def _matrices(rng):
    holes = (-3.0 * rng.random((3, 3))).astype(np.float32)
    holes[0, 1] = holes[2, 0] = -np.inf
    chain = np.full((3, 3), -np.inf, np.float32)                                 # 0 -> 1 -> 2 only, no way back
    chain[np.arange(3), np.arange(3)] = -0.25
    chain[0, 1] = chain[1, 2] = -1.0
    return {"finite": (-3.0 * rng.random((3, 3))).astype(np.float32), "holes": holes, "chain": chain, "zero": np.zeros((3, 3), np.float32)}


def test_float64_equals_the_brute_force_marginals():
    from tennis_amd.events import hmm_posteriors
    rng = np.random.default_rng(0)
    worst = 0.0
    for name, trans in _matrices(rng).items():
        for lengths in ([1], [2], [6], [3, 1, 5], [1, 1], [4, 6]):                # one call: several videos, videos of length 1
            m = sum(lengths)
            n = m + 5
            logits = (rng.normal(0, 2.0, (n, 3))).astype(np.float32)
            rows = rng.permutation(n)[:m]
            rows[0] = n + 7                                                      # clipped to the last row
            start = np.zeros(m, np.int32)
            bounds = np.cumsum([0] + lengths)
            start[bounds[1:-1]] = 1                                              # (position 0 begins a video whatever its flag says)
            got = hmm_posteriors(logits, rows, start, trans)
            assert got.shape == (m, 3) and got.dtype == np.float64
            e = _emissions(logits, rows)
            for a, b in zip(bounds[:-1], bounds[1:]):
                want = _brute_force(e[a:b], trans)
                worst = max(worst, float(np.abs(got[a:b] - want).max()))
                assert np.abs(got[a:b] - want).max() <= 1e-12, (name, lengths, a)
            assert np.abs(got.sum(1) - 1).max() <= 1e-12
    print("hmm_posteriors(float64) against brute force: largest error %.3g" % worst)


def test_closed_form_identical_rows():
    """T[p, c] = r[c]: the label of a position does not depend on its predecessor, so the positions are independent"""
    from tennis_amd.events import hmm_posteriors
    rng = np.random.default_rng(1)
    for c in (1, 2, 5, 11):
        m = 40
        r = (-2.0 * rng.random(c)).astype(np.float32)
        trans = np.tile(r, (c, 1))
        logits = rng.normal(0, 3, (m, c)).astype(np.float32)
        start = np.zeros(m, np.int32)
        start[[0, 17, 18]] = 1
        e = _emissions(logits, np.arange(m))
        want = _softmax(e + r.astype(np.float64))
        want[start != 0] = _softmax(e[start != 0])
        assert np.abs(hmm_posteriors(logits, np.arange(m), start, trans) - want).max() <= 1e-12


def test_closed_form_no_switch_possible():
    """every off-diagonal entry -inf: a video keeps one label, whose probability every position shares"""
    from tennis_amd.events import hmm_posteriors
    rng = np.random.default_rng(2)
    for c in (1, 3, 11):
        lengths = [1, 2, 30]
        m = sum(lengths)
        trans = np.full((c, c), -np.inf, np.float32)
        trans[np.arange(c), np.arange(c)] = (-rng.random(c)).astype(np.float32)
        logits = rng.normal(0, 1, (m, c)).astype(np.float32)
        start = np.zeros(m, np.int32)
        bounds = np.cumsum([0] + lengths)
        start[bounds[:-1]] = 1
        got = hmm_posteriors(logits, np.arange(m), start, trans)
        e = _emissions(logits, np.arange(m))
        for a, b in zip(bounds[:-1], bounds[1:]):
            want = _softmax(e[a:b].sum(0) + (b - a - 1) * np.diagonal(trans).astype(np.float64))
            assert np.abs(got[a:b] - want[None]).max() <= 1e-12, (c, a)


def test_the_sums_run_in_ascending_order():
    """the float32 run against the definition written out with explicit loops (every sum in ascending index): the same bits"""
    from tennis_amd.events import hmm_posteriors
    rng = np.random.default_rng(3)
    f = np.float32
    for c in (3, 11, 17):
        m = 25
        logits = rng.normal(0, 3, (m, c)).astype(f)
        trans = (-3.0 * rng.random((c, c))).astype(f)
        trans[(rng.random((c, c)) < 0.2) & ~np.eye(c, dtype=bool)] = -np.inf
        e = logits - logits.max(1, keepdims=True)

        def lse(x):
            mx = max(x)
            if mx == -np.inf:
                return f(-np.inf)
            s = f(0)
            for v in x:
                s = f(s + np.exp(f(v - mx)))
            return f(mx + np.log(s))
        ah, bh = np.zeros((m, c), f), np.zeros((m, c), f)
        ah[0] = e[0]
        for t in range(1, m):
            a = np.asarray([f(e[t, k] + lse([f(ah[t - 1, p] + trans[p, k]) for p in range(c)])) for k in range(c)], f)
            ah[t] = a - a.max()
        for t in range(m - 2, -1, -1):
            b = np.asarray([lse([f(trans[p, k] + f(e[t + 1, k] + bh[t + 1, k])) for k in range(c)]) for p in range(c)], f)
            bh[t] = b - b.max()
        want = np.zeros((m, c), f)
        for t in range(m):
            g = ah[t] + bh[t]
            x = np.exp(g - g.max())
            s = f(0)
            for v in x:
                s = f(s + v)
            want[t] = x / s
        got = hmm_posteriors(logits, np.arange(m), np.zeros(m), trans, dtype=np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want), c


def test_extreme_logits_against_a_forbidding_matrix_stay_finite():
    from tennis_amd.events import hmm_posteriors
    trans = np.array([[0.0, -np.inf, -0.5], [-0.5, 0.0, -0.5], [-0.5, -0.5, 0.0]], np.float32)
    m = 12
    logits = np.zeros((m, 3), np.float32)
    logits[:6, 0] = 200.0
    logits[6:, 1] = 200.0                                                        # the frames ask for 0 -> 1, which is forbidden
    for dtype in (np.float32, np.float64):
        g = hmm_posteriors(logits, np.arange(m), np.zeros(m), trans, dtype=dtype)
        assert np.all(np.isfinite(g)) and np.abs(g.astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -23
    six = hmm_posteriors(logits[3:9], np.arange(6), np.zeros(6), trans)
    assert np.abs(six - _brute_force(_emissions(logits[3:9], np.arange(6)), trans)).max() <= 1e-12


def test_hmm_posteriors_refusals_and_edges():
    from tennis_amd.events import hmm_posteriors
    x = np.zeros((4, 3), np.float32)
    assert hmm_posteriors(x, [], [], np.zeros((3, 3))).shape == (0, 3)
    assert np.allclose(hmm_posteriors(x, np.arange(4), np.zeros(4), np.zeros((3, 3))), 1 / 3, atol=1e-15)
    for bad, why in ((np.zeros((2, 2)), r"\(3, 3\)"), (np.full((3, 3), np.nan), r"\[0\]\[0\] is NaN"),
                     (np.array([[0, 0, 0], [0, 0, 0.5], [0, 0, 0]]), r"\[1\]\[2\] is positive"),
                     (np.array([[0, 0, 0], [0, 0, 0], [0, 0, -np.inf]]), r"\[2\]\[2\] is not finite")):
        with pytest.raises(ValueError, match=why):
            hmm_posteriors(x, np.arange(4), np.zeros(4), bad)
    with pytest.raises(ValueError, match="start flags"):
        hmm_posteriors(x, [0, 1], [1], np.zeros((3, 3)))


def test_posterior_flag_and_refusals():
    from tennis_amd import evaluate as ev
    from tennis_amd.events import check_save_events
    parse = ev.build_parser().parse_args
    assert parse([]).event_posteriors is False
    assert parse(["--save_events", "--event_transitions", "train", "--event_posteriors"]).event_posteriors is True
    for bad, why in ((["--event_posteriors"], "give --save_events too"),
                     (["--event_posteriors", "--event_transitions", "train"], "give --save_events too"),
                     (["--save_events", "--event_posteriors"], "give --event_transitions or --event_switch_cost too"),
                     (["--save_events", "--event_posteriors", "--event_smooth", "5"], "give --event_transitions or --event_switch_cost too"),
                     (["--save_events", "--event_posteriors", "--event_transitions", "train", "--event_smooth", "3"], "not together with --event_smooth 3"),
                     (["--save_events", "--event_posteriors", "--event_switch_cost", "1", "--num_gpus", "2"], "--num_gpus 1")):
        with pytest.raises(SystemExit, match=why):
            ev.main(["--root", "/nonexistent"] + bad)                            # refused before anything is opened or built
    for good in (["--save_events", "--event_transitions", "train", "--event_posteriors"],
                 ["--save_events", "--event_switch_cost", "2", "--event_posteriors"],
                 ["--save_events", "--event_transitions", "t.npy", "--event_posteriors", "--event_smooth", "1"]):
        check_save_events(parse(good))

    class Old:                                                                   # flags built by hand, without the newer switches
        save_events, save_feats, corpus_frames, num_gpus = True, False, 0, 1
    check_save_events(Old())


def test_decode_split_refuses_posteriors_without_a_path():
    from tennis_amd.events import decode_split
    with pytest.raises(ValueError, match="give switch_cost or transitions"):     # before the dataset or the logits are touched
        decode_split(None, None, posteriors=True)
    with pytest.raises(ValueError, match="smooth=3"):
        decode_split(None, None, smooth=3, switch_cost=1.0, posteriors=True)


def _cols():
    return dict(video=["V1", "V1"], first_frame=[0, 10], last_frame=[9, 12], cls=[0, 2], score=np.asarray([0.5, 0.9], np.float32),
                peak=np.asarray([0.7, 0.99], np.float32), first_sample=[4, 0], last_sample=[5, 1], gt_video=["V1"], gt_first_frame=[0],
                gt_last_frame=[12], gt_cls=[0], smooth=1, tiou=[0.1, 0.3, 0.5], precision=np.full((3, 3), 0.5),
                recall=np.full((3, 3), 0.25), f1=np.full((3, 3), 1 / 3))


def test_the_posteriors_column_is_written_only_when_given(tmp_path):
    from tennis_amd import events as E
    plain, path, post = (str(tmp_path / n) for n in ("plain.npz", "path.npz", "post.npz"))
    trans = np.zeros((3, 3), np.float32)
    E.save_events(plain, **_cols())
    E.save_events(path, **_cols(), transitions=trans)
    E.save_events(post, **_cols(), transitions=trans, posteriors=True)
    with np.load(plain, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS)                              # exactly the columns it had
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS) | {"transitions"}
    with np.load(post, allow_pickle=False) as z:
        assert set(z.files) == set(E.EVENT_COLUMNS) | {"transitions", "posteriors"}
        assert z["posteriors"].shape == () and z["posteriors"].dtype == np.bool_ and bool(z["posteriors"])
    E.save_events(post, **_cols(), switch_cost=2.0, posteriors=True)
    d = E.load_events(post)
    assert bool(d["posteriors"]) and float(d["switch_cost"]) == 2.0 and "posteriors" not in E.EVENT_COLUMNS
    assert "posterior scores" in E.event_table(d, ["OTH", "SERVE", "HIT"])
    assert "posterior" not in E.event_table(E.load_events(path), ["OTH", "SERVE", "HIT"])
    with pytest.raises(ValueError, match="give switch_cost or transitions"):
        E.save_events(post, **_cols(), posteriors=True)


def test_abi_surface_of_the_posterior_entry():
    from tennis_amd import _lib
    pub = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    name = "tn_event_decoder_run_posteriors"
    assert re.search(r"^int %s\(" % name, pub, re.M) and name not in dbg.replace("first " + name, "") and name in _lib.declared_symbols()
    assert re.search(r"const float \*transitions, int32_t \*label_out, float \*conf_out, float \*posterior,", pub)
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None
    for words in ("forward-backward", "may be NULL", "gamma_m[label[m]]", "TN_ERR_NOMEM", "2 * max_positions * pitch * 4"):
        assert words in pub, words
    L = _lib.load()
    assert L.tn_event_decoder_run_posteriors(None, None, 1, 1, None, None, 1, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"tn_event_decoder_run_posteriors" in L.tn_last_error() and b"handle" in L.tn_last_error()
    doc = open(os.path.join(ROOT, "docs", "kernels.md")).read()
    assert "Event scores from posteriors" in doc and "hmm_chain_kernel" in doc and "hmm_posterior_kernel" in doc
