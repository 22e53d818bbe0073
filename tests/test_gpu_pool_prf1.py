"""-m gpu: tn_temporal_pool / tn_temporal_pool_arg and tn_prf1_update (csrc/rnn.hip) past the one shape each had: fewer outputs than
a workgroup, exactly one, one more; one step and many; infinities and ties; the confusion matrix added into, labels out of range.
No tolerance anywhere: the max is the input's own element, the mean is held bitwise to the float32 restatement of the kernel's
definition (its float64 error is reported beside it), the confusion counts are integers.  NaN inputs are out of scope: fmaxf and
`>` skip them, numpy does not (docs/numerics.md)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POOL_SHAPES = [(1, 1, 1), (1, 1, 255), (1, 3, 256), (1, 3, 257), (3, 1, 300), (2, 17, 256), (5, 64, 257), (1, 200, 64), (4, 9, 37)]


@pytest.fixture(scope="module")
def ctx():
    from tennis_amd import _lib
    return _lib.default_context(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pool_input(B, T, F):
    """Normal values (no zero, no NaN) with, where there are columns for them: a column that is -inf at every step, one with a +inf,
    one whose largest value stands at two steps, one whose steps are all equal - in the first and the last batch row"""
    x = np.random.default_rng(B * 10007 + T * 101 + F).normal(0, 1, (B, T, F)).astype(np.float32)
    assert (x != 0).all()
    for b in {0, B - 1}:
        cols = [F - 1 - k for k in range(4) if F - 1 - k >= 0]           # the last columns: the last threads of the last workgroup
        if len(cols) >= 1:
            x[b, :, cols[0]] = -np.inf
        if len(cols) >= 2:
            x[b, T // 2, cols[1]] = np.inf
        if len(cols) >= 3:
            x[b, [0, T - 1], cols[2]] = 7.5
        if len(cols) >= 4:
            x[b, :, cols[3]] = -1.25
    return x


def _mean_f32(x):
    """The kernel's definition: acc = acc + x[:, t] in float32, t ascending from 0.f, then one float32 division by T"""
    acc = np.zeros((x.shape[0], x.shape[2]), np.float32)
    for t in range(x.shape[1]):
        acc = acc + x[:, t]
    assert acc.dtype == np.float32
    return acc / np.float32(x.shape[1])


@pytest.mark.parametrize("B,T,F", POOL_SHAPES)
def test_temporal_pool_max_and_mean(ctx, report, B, T, F):
    from tennis_amd.engine import temporal_pool
    x = _pool_input(B, T, F)
    xd = torch.from_numpy(x).cuda()
    got = temporal_pool(xd, "max", ctx).cpu().numpy()
    assert got.shape == (B, F) and np.array_equal(_bits(got), _bits(x.max(1)))
    if F >= 2:
        assert got[0, F - 1] == -np.inf and got[B - 1, F - 2] == np.inf
    with np.errstate(invalid="ignore"):
        want = _mean_f32(x)
    assert not np.isnan(want).any()                     # -inf and +inf never share a column
    got = temporal_pool(xd, "mean", ctx).cpu().numpy()
    assert got.shape == (B, F) and np.array_equal(_bits(got), _bits(want))
    fin = np.isfinite(want)
    report[f"temporal_pool_mean_maxabs_err_vs_f64_{B}x{T}x{F}"] = (
        float(np.abs(got[fin].astype(np.float64) - x.astype(np.float64).mean(1)[fin]).max()) if fin.any() else 0.0)


@pytest.mark.parametrize("v", [-np.inf, np.inf, -3.5])
def test_temporal_pool_of_a_single_value(ctx, v):
    from tennis_amd.engine import temporal_pool
    xd = torch.full((1, 1, 1), float(v), device="cuda")
    for kind in ("max", "mean"):
        got = temporal_pool(xd, kind, ctx).cpu().numpy()
        assert got.shape == (1, 1) and got[0, 0] == np.float32(v)


def test_temporal_pool_arg_returns_the_max_pools_bits(ctx):
    from tennis_amd.engine import temporal_pool
    x = _pool_input(5, 64, 257)
    xd = torch.from_numpy(x).cuda()
    y, arg = temporal_pool(xd, "max", ctx, return_steps=True)
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(temporal_pool(xd, "max", ctx).cpu().numpy()))
    arg = arg.cpu().numpy()
    assert np.array_equal(arg, x.argmax(1))                # the first step that holds the maximum; step 0 for a column of -inf
    assert arg[0, 257 - 3] == 0 and arg[0, 257 - 2] == 32 and arg[0, 257 - 1] == 0      # the tie, the +inf, the -inf column


def _prf1_data(rows, classes, seed):
    """Logits with ties at every class position (row 3 k: classes c, c + 2, c + 4 ... tied at the top, c = k mod classes), all-equal
    rows, rows of -inf, +inf once and twice; labels in range with -1 and `classes` among them"""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 1, (rows, classes)).astype(np.float32)
    for i in range(rows):
        c = (i // 3) % classes
        if i % 3 == 0:
            logits[i, c::2] = 9.0
        elif i % 12 == 1:
            logits[i] = 1.25
        elif i % 12 == 4:
            logits[i] = -np.inf
        elif i % 12 == 7:
            logits[i, c] = np.inf
        elif i % 12 == 10:
            logits[i, c] = logits[i, classes - 1] = np.inf
    labels = rng.integers(0, classes, rows).astype(np.int32)
    labels[rng.random(rows) < 0.1] = -1
    labels[rng.random(rows) < 0.1] = classes
    if rows >= 2:
        labels[0], labels[rows - 1] = classes, -1
    return logits, labels


def _prf1_ref(logits, labels, classes):
    m = np.zeros((classes, classes), np.int64)
    ok = (labels >= 0) & (labels < classes)
    np.add.at(m, (labels[ok], logits.argmax(1)[ok]), 1)
    return m, int(ok.sum())


def test_prf1_data_has_what_it_says():
    logits, labels = _prf1_data(513, 11, 0)
    am = logits.argmax(1)
    assert set(am[0::3][:33].tolist()) == set(range(11))                         # a tie won by every class position
    assert (logits[4] == -np.inf).all() and am[4] == 0 and am[1] == 0 and (logits[1] == 1.25).all()
    assert (labels == -1).any() and (labels == 11).any() and ((labels >= 0) & (labels < 11)).sum() > 300
    last = 10 - logits[:, ::-1].argmax(1)                                        # what `>=` in place of `>` would pick
    ok = (labels >= 0) & (labels < 11)
    assert (last != am)[ok].sum() > 100
    m, _ = _prf1_ref(logits, labels, 11)
    assert m.max() > 1                                                           # what `=` in place of `+=` could not count


@pytest.mark.parametrize("classes", [1, 2, 11, 64])
def test_prf1_update_adds_first_maxima_of_in_range_rows(ctx, classes):
    from tennis_amd import _lib
    for rows in (1, 255, 256, 257, 513):
        start = (np.arange(classes * classes, dtype=np.int64) * 7 % 5).reshape(classes, classes) + 1      # non-zero everywhere
        mat = torch.from_numpy(start.copy()).cuda()
        want, kept_so_far = start.copy(), 0
        for call in range(2):                                    # the second call adds to what the first left
            logits, labels = _prf1_data(rows, classes, 1000 * classes + 10 * rows + call)
            ld, lab = torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()
            _lib.check(ctx.lib.tn_prf1_update(ctx.handle, _lib.ptr(ld), _lib.ptr(lab), rows, classes, _lib.ptr(mat)), "tn_prf1_update")
            torch.cuda.synchronize()
            m, kept = _prf1_ref(logits, labels, classes)
            want += m
            kept_so_far += kept
            got = mat.cpu().numpy()
            assert np.array_equal(got, want), (classes, rows, call)
            assert int(got.sum() - start.sum()) == kept_so_far            # out-of-range rows are dropped ...
            assert kept < rows or rows == 1                               # ... and there are some


def test_prf1_metric_device_and_host_routes_agree(ctx):
    from tennis_amd.metrics.vision import PRF1
    names = [f"c{i}" for i in range(11)]
    logits, _ = _prf1_data(513, 11, 42)
    labels = np.random.default_rng(43).integers(0, 11, 513).astype(np.int32)      # the host route has no out-of-range rule: in range only
    dev, host = PRF1(label_names=names), PRF1(label_names=names)
    for lo, hi in ((0, 256), (256, 513)):                                          # two updates: the metric accumulates too
        dev.update(torch.from_numpy(labels[lo:hi]).cuda(), torch.from_numpy(logits[lo:hi]).cuda())
        host.update(labels[lo:hi], logits[lo:hi])
    assert np.array_equal(dev.mat, host.mat) and dev.mat.sum() == 513
    a, b = dev.get(), host.get()
    assert len(a) == len(b) == 39
    for (na, va), (nb, vb) in zip(a, b):
        assert na == nb and va == vb, (na, va, nb, vb)
