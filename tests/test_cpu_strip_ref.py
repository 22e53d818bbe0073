"""-m "not gpu": the float64 reference, the derived bound and the input generators of tests/tools/strip_ref.py, checked on their own -
they are what tests/test_gpu_strip_instantiations.py holds every dense_strip_kernel<W, KS> to.

  * an fp32 model of the kernel's arithmetic (float32 accumulation k-step by k-step, the two fp16 roundings, three column
    accumulators summed last) stays inside the bound on the `noisy` inputs, at one geometry per map width;
  * the same model with one defect at a time leaves it: one (tap, channel) product missing from one output channel, one input
    channel of the 1x1 missing, the bottleneck row above a chunk seam taken from the row below it, one padding column not zero -
    so the bound can fail, and fails for the mistakes the planted seams are there for;
  * on the `integer` inputs the float64 result consists of integers fp16 holds exactly, for all 35 supported (W, K), and the
    generator keeps the structure it promises.

Outside the bound's reach, listed and not worked around: the low half of the shift dropped (at most 2^-11 |t2|, below the rounding of
a2 the bound has to allow), and any other perturbation of that size."""
import numpy as np
import pytest

from tools import strip_ref as SR

MODEL_CASES = [(28, 96), (56, 320), (64, 64), (128, 288)]
_cache = {}


def _case(w, k):
    """inputs, reference and bound of a `noisy` case, computed once and left unchanged"""
    if (w, k) not in _cache:
        inp = SR.noisy(w, k, 1, 0)
        y, bound = SR.reference(inp)
        for a in (y, bound, *inp.values()):
            a.setflags(write=False)
        _cache[(w, k)] = (inp, y, bound)
    return _cache[(w, k)]


@pytest.mark.parametrize("w,k", MODEL_CASES)
def test_fp32_model_stays_inside_the_bound(w, k):
    """Worst ratios of the model (recorded in docs/numerics.md): 0.20 at (28, 96), 0.14 at (56, 320), 0.24 at (64, 64), 0.18 at
    (128, 288)"""
    inp, y, bound = _case(w, k)
    r = SR.ratio(SR.model(inp), y, bound)
    print("fp32 model at %d x %d, K = %d: max |err| / E = %.3f, |y| max %.3g, E median %.3g" % (w, w, k, r, np.abs(y).max(), np.median(bound)))
    assert r <= 1.0
    assert r > 0.05          # a bound the model does not come near would not be a bound on anything


@pytest.mark.parametrize("w,k", MODEL_CASES)
def test_every_listed_defect_leaves_the_bound(w, k):
    inp, y, bound = _case(w, k)
    rows = SR.rows_per_wave(w)
    # the product of output channel 5's largest weight: E sums |w3| u a2 over all 1152 products of an output, so one product of an
    # average weight (a 1152th of that sum, times 1 / u) is about as large as E - on real-valued inputs the bound sees a missing
    # product only where its weight is well above average.  The `integer` inputs see every one of them.
    tap = (5, *(int(i) for i in np.unravel_index(np.abs(inp["w3"][5]).argmax(), (128, 3, 3))))
    defects = {
        "one (tap, channel) product missing from one output channel": dict(drop_tap=tap),
        "input channel k of the 1x1 missing": dict(drop_k=k - 3),
        "bottleneck row above a chunk seam taken from the row below it": dict(seam_row=rows),
        "padding column not zero": dict(pad_col=True),
    }
    for name, kw in defects.items():
        err = np.abs(SR.model(inp, **kw).astype(np.float64) - y) / bound
        print("%d x %d, K = %d, %s: max |err| / E = %.3g at %s" % (w, w, k, name, err.max(), np.unravel_index(err.argmax(), err.shape)))
        assert err.max() > 1.0, name
    # each defect is seen where it is: the missing tap in its output channel only, the seam in its row only, the padding column in
    # column 0 only
    e = np.abs(SR.model(inp, drop_tap=tap).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 1, 2)).nonzero()[0].tolist() == [5]
    e = np.abs(SR.model(inp, seam_row=rows).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 2, 3)).nonzero()[0].tolist() == [rows]
    e = np.abs(SR.model(inp, pad_col=True).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 1, 3)).nonzero()[0].tolist() == [0]


def test_noisy_inputs_plant_both_sides_of_every_seam():
    assert SR.seam_lines(56) == ([0, 27, 28, 55], [0, 13, 14, 27, 28, 41, 42, 55])
    assert SR.seam_lines(28) == ([0, 6, 7, 13, 14, 20, 21, 27], [0, 13, 14, 27])
    rows, cols = SR.seam_lines(64)
    assert rows == [0, 15, 16, 31, 32, 47, 48, 63] and cols == [0, 13, 14, 27, 28, 41, 42, 55] + list(range(56, 64))
    rows, cols = SR.seam_lines(128)
    assert rows == [0, 31, 32, 63, 64, 95, 96, 127]
    assert cols == sorted({0, 127} | {c for s in range(14, 128, 14) for c in (s - 1, s)} | set(range(112, 128)))
    x = SR.noisy(28, 64, 2, 3)["x"].astype(np.float32)
    rows, cols = SR.seam_lines(28)
    planted = np.zeros((28, 28), bool)
    planted[rows, :] = True
    planted[:, cols] = True
    assert np.all((np.abs(x[:, planted]) >= 20) & (np.abs(x[:, planted]) <= 60))
    assert np.abs(x[:, ~planted]).max() < 12 and (x[:, planted] > 0).any() and (x[:, planted] < 0).any()


@pytest.mark.parametrize("w,k", SR.SUPPORTED, ids=["%d-%d" % c for c in SR.SUPPORTED])
def test_integer_inputs_are_exact_in_float64(w, k):
    """What makes the GPU test's bit comparison legitimate: every intermediate of the `integer` case is an integer small enough for
    the format that holds it (|bott| <= 24 in fp32 and fp16, |y| <= 864 < 2048 in fp32 and fp16), and the weights have the structure
    that makes a dropped, doubled or mis-permuted product change an integer."""
    inp = SR.integer(w, k, 1, 0)
    assert set(np.unique(inp["x"].astype(np.float32))) == {0.0, 1.0}
    w1, w3, t2 = inp["w1"], inp["w3"], inp["t2"]
    assert np.all(np.isin(w1, (-1, 0, 1))) and np.all((w1 != 0).sum(axis=1) == 16) and np.all((w1 != 0).sum(axis=0) >= 2)
    assert len({tuple(np.flatnonzero(r)) for r in w1}) > 32                      # rotated, not one pattern
    assert np.all(t2 == np.round(t2)) and np.abs(t2).max() <= 8
    assert np.all(np.isin(w3, (-1, 0, 1))) and np.all((w3 != 0).sum(axis=0) == 1) and np.all((w3 != 0).sum(axis=(1, 2, 3)) == 36)
    assert np.array_equal(SR.folded_weights(w1, inp["s2"]), w1.astype(np.float64))
    hi, lo = SR.shift_halves(t2)
    assert np.array_equal(hi, t2.astype(np.float64)) and not lo.any()
    y, bound = SR.reference(inp)
    assert np.array_equal(y, np.round(y)) and np.abs(y).max() <= 864 and np.abs(y).max() > 30
    assert np.array_equal(y.astype(np.float16).astype(np.float64), y)
    assert len(np.unique(y)) > 40                                               # not a degenerate map
    if (w, k) in MODEL_CASES:                                                   # and the kernel's arithmetic reproduces it exactly
        assert np.array_equal(SR.model(inp).astype(np.float64), y)
