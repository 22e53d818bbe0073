"""-m "not gpu": the float64 reference, the derived bound, the input generators and the shape lists of tests/tools/block_ref.py, checked
on their own - they are what tests/test_gpu_block_instantiations.py holds dense_block7.hip, dense_block14.hip and dense_block28.hip to.

  * an fp32 model of each kernel's arithmetic (float32 accumulation k-step by k-step in the kernel's split - four K ranges summed last at
    7 x 7, super-steps then the permuted tail then the shift at 14 x 14, the shift first at 28 x 28 -, the two fp16 roundings, three column
    accumulators or four per-wave partial sums added last) stays inside the bound on `noisy` and returns `chain_integer` exactly;
  * the same model with one defect at a time leaves the bound on `noisy` (ratios: docs/numerics.md) and changes an integer;
  * the shape lists cover every tail variant / super-step flavour / ring-slot residue in every role, computed with the formulas restated
    from the packers and held equal to their source text; a list with any one row deleted fails;
  * the refusal rule restated, against the lists and the refusal cases."""
import os
import re

import numpy as np
import pytest

from tools import block_ref as BR

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tennis_amd", "csrc")
MODEL_CASES = {7: (448, 2), 14: (320, 2), 28: (160, 2)}          # the smallest K0 whose second layer has a clipped last super-step (14, 28)
_cache = {}


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _case(h):
    """a `noisy` block of one frame through the model, computed once and left unchanged"""
    if h not in _cache:
        k0, nl = MODEL_CASES[h]
        x, layers = BR.noisy(h, k0, nl, 1, 0)
        buf = BR.model_block(x, layers, h)
        for a in (x, buf, *[v for p in layers for v in p.values()]):
            a.setflags(write=False)
        _cache[h] = (k0, nl, x, layers, buf)
    return _cache[h]


@pytest.mark.parametrize("h", BR.SIZES)
def test_fp32_model_stays_inside_the_bound_and_returns_the_integers(h):
    """Worst ratios of the model (docs/numerics.md): 0.06 - 0.3 as for the strip and tile kernels"""
    k0, nl, x, layers, buf = _case(h)
    rs = BR.block_ratios(buf, k0, layers, h)
    print("fp32 model at %d x %d, K0 = %d: max |err| / E per layer = %s" % (h, h, k0, ["%.3f" % r for r in rs]))
    assert max(rs) <= 1.0
    assert min(rs) > 0.03          # a bound the model does not come near would not be a bound on anything
    xi, li = BR.integer_block(h, k0, nl, BR.BATCH[h], 0)
    want = BR.chain_reference(xi, li, h)
    assert np.array_equal(want, np.round(want)) and np.abs(want).max() < 2048 and len(np.unique(want[..., k0:])) > 40
    assert np.array_equal(BR.model_block(xi, li, h).astype(np.float64), want)
    _integers_are_alive(h, k0, xi, li, want)


def _integers_are_alive(h, k0, xi, li, want):
    """every layer sees {0, 1} again; no input channel is constant and no bottleneck channel is dead, so a product dropped, doubled or
    taken from the wrong place anywhere changes some output"""
    for l, p in enumerate(li):
        k = k0 + 32 * l
        a1 = np.clip(want[..., :k], p["lo"], p["hi"])
        assert set(np.unique(a1)) <= {0.0, 1.0} and np.all(a1.min(axis=(0, 1, 2)) == 0) and np.all(a1.max(axis=(0, 1, 2)) == 1), l
        assert np.all(p["t2"] >= -2) and np.all(p["t2"] == np.round(p["t2"])) and np.all(p["s2"] == 1)
        w1, w3 = p["w1"], p["w3"]
        assert np.all(np.isin(w1, (-1, 0, 1))) and np.all((w1 != 0).sum(axis=1) == 16) and np.all(w1.sum(axis=1) == 0) and np.all((w1 != 0).sum(axis=0) >= 1)
        assert np.all(np.isin(w3, (-1, 0, 1))) and np.all((w3 != 0).sum(axis=0) == 1) and np.all((w3 != 0).sum(axis=(1, 2, 3)) == 36) and np.all(w3.sum(axis=(1, 2, 3)) == 0)
        a2 = np.maximum(a1 @ w1.T.astype(np.float64) + p["t2"], 0.0)
        assert np.all(a2.max(axis=(0, 1, 2)) >= 1) and a2.max() <= 24, l


@pytest.mark.parametrize("h,k0,nl", [(7, 512, 16), (14, 256, 24), (28, 128, 13)])
def test_integers_stay_alive_through_the_longest_blocks(h, k0, nl):
    xi, li = BR.integer_block(h, k0, nl, BR.BATCH[h], 0)       # as the GPU test runs it: a bottleneck channel with t2 = -2 needs some hundred pixels to show
    want = BR.chain_reference(xi, li, h)
    assert np.array_equal(want, np.round(want)) and np.abs(want).max() <= 864
    _integers_are_alive(h, k0, xi, li, want)


def _defects(h, k0, layers, prev_a2):
    p = layers[1]
    k = k0 + 32
    tap = (5, *(int(i) for i in np.unravel_index(np.abs(p["w3"][5]).argmax(), (128, 3, 3))))
    d = {"the largest 3x3 product of one output missing": dict(drop_tap=tap),
         "one input channel of the 1x1 missing": dict(drop_k=k0 // 2 + 1),
         "left padding column not zero": dict(pad_col=0),
         "right padding column not zero": dict(pad_col=1),
         "the row below the frame not zero": dict(ghost_row=True)}
    if h == 7:
        d["wave 2's K-range partial sum missing"] = dict(drop_wave=2)
    if h == 14:
        d["the row above the wave seam 7 | 8 taken from below it"] = dict(seam_row=8)
        d["the forwarded 32 channels consumed in plain order"] = dict(plain_forward=True)
    if h == 28:
        d["row -1 of pass 2 (row 15) taken from the previous layer's tile"] = dict(stale_row=(15, prev_a2))
    return d, k


@pytest.mark.parametrize("h", BR.SIZES)
def test_every_listed_defect_leaves_the_bound_and_changes_an_integer(h):
    k0, nl, x, layers, buf = _case(h)
    _, prev = BR.model(dict(x=buf[..., :k0].astype(np.float16), **layers[0]), h, want_a2=True)
    defects, k = _defects(h, k0, layers, prev)
    inp = dict(x=buf[..., :k].astype(np.float16), **layers[1])
    y, bound = BR.reference(inp, h)
    for name, kw in defects.items():
        err = np.abs(BR.model(inp, h, **kw).astype(np.float64) - y) / bound
        print("%d x %d, K = %d, %s: max |err| / E = %.3g at %s" % (h, h, k, name, err.max(), np.unravel_index(err.argmax(), err.shape)))
        assert err.max() > 1.0, name
    # each defect is seen where it is
    e = lambda **kw: np.abs(BR.model(inp, h, **kw).astype(np.float64) - y) / bound
    assert (e(pad_col=0) > 1.0).any(axis=(0, 1, 3)).nonzero()[0].tolist() == [0]
    assert (e(pad_col=1) > 1.0).any(axis=(0, 1, 3)).nonzero()[0].tolist() == [h - 1]
    assert (e(ghost_row=True) > 1.0).any(axis=(0, 2, 3)).nonzero()[0].tolist() == [h - 1]
    if h == 14:
        assert (e(seam_row=8) > 1.0).any(axis=(0, 2, 3)).nonzero()[0].tolist() == [8]
    if h == 28:
        assert (e(stale_row=(15, prev)) > 1.0).any(axis=(0, 2, 3)).nonzero()[0].tolist() == [15, 16]
    # the integers: every defect, and a single missing product at arbitrary positions
    xi, li = BR.integer_block(h, k0, nl, 1, 0)
    want = BR.chain_reference(xi, li, h)
    inpi = dict(x=want[..., :k].astype(np.float16), **li[1])
    _, previ = BR.model(dict(x=xi, **li[0]), h, want_a2=True)
    di, _ = _defects(h, k0, li, previ)
    di.pop("the largest 3x3 product of one output missing")
    rng = np.random.default_rng([h, 9])
    for _ in range(6):
        c, dy, dx = int(rng.integers(128)), int(rng.integers(3)), int(rng.integers(3))
        o = int(np.flatnonzero(li[1]["w3"][:, c, dy, dx])[0])
        di["product (%d, %d, %d, %d) missing" % (o, c, dy, dx)] = dict(drop_tap=(o, c, dy, dx))
    di["the newest input channel missing"] = dict(drop_k=k - 1)
    for name, kw in di.items():
        assert not np.array_equal(BR.model(inpi, h, **kw).astype(np.float64), want[..., k:k + 32]), name


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", BR.SIZES)
def test_shape_lists_cover_every_loop_variant(h):
    assert BR.coverage_problems(h, BR.SHAPES[h]) == []
    assert sorted((r[0], r[1]) for r in BR.SHAPES[h]) == sorted(r[:2] for r in BR.required_rows(h))
    assert len(BR.SHAPES[h]) == {7: 20, 14: 27, 28: 15}[h] and all(len(r) == 3 and r[2] for r in BR.SHAPES[h])
    for k0, nl, _ in BR.SHAPES[h]:
        assert BR.launchable(h, k0, nl, BR.case_ldc(h, k0, nl), BR.BATCH[h]) and BR.launchable(h, k0, nl, BR.smallest_ldc(h, k0, nl), 1)
    assert {BR.case_ldc(h, k0, nl) == BR.smallest_ldc(h, k0, nl) for k0, nl, _ in BR.SHAPES[h]} == {True, False}


@pytest.mark.parametrize("h", BR.SIZES)
def test_deleting_any_row_of_a_shape_list_fails_a_check(h):
    for i, row in enumerate(BR.SHAPES[h]):
        rest = BR.SHAPES[h][:i] + BR.SHAPES[h][i + 1:]
        problems = BR.coverage_problems(h, rest)
        assert problems, row
        assert any("K0 = %d, nl = %d" % row[:2] in p for p in problems), (row, problems)


def test_what_a_thinner_list_would_miss():
    """the variant checks, not only the row checks, bite: without the long chains no tail variant runs as an inner layer; the first
    layers alone do not reach every ring-slot residue"""
    short7 = [r for r in BR.SHAPES[7] if r[1] <= 2]
    assert any("inner layer" in p for p in BR.coverage_problems(7, short7))
    for h in (14, 28):
        first = [r for r in BR.SHAPES[h] if r[1] == 1]
        assert any("mod 5" in p for p in BR.coverage_problems(h, first))
        only_even = [r for r in BR.SHAPES[h] if r[1] <= 2 and (r[0] // 64) % 2 == 0 and r[0] % 64 == 0]
        assert any("super-step count" in p for p in BR.coverage_problems(h, only_even))


def test_restated_formulas_equal_the_source():
    b7, b14, b28, ds = _src("dense_block7.hip"), _src("dense_block14.hip"), _src("dense_block28.hip"), _src("dense_stream.h")
    assert int(re.search(r"constexpr int kRingDepth = (\d+);", b7).group(1)) == BR.RING7
    assert int(re.search(r"constexpr int kNR = (\d+);", ds).group(1)) == BR.NR
    pack7 = b7[b7.index("Block7Image pack_block7("):b7.index("int launch_dense_block7(")]
    assert "G = K / 16, gbase = G / 4, grem = G % 4;" in pack7
    assert "const int nA = gbase + (w < grem ? 1 : 0), g0 = w * gbase + (w < grem ? w : grem);" in pack7
    assert "const int M = (w + m) & 3, g = g0 + sidx;" in pack7
    assert "while (b + 2 * D + 1 <= nA) {" in b7 and "const int r = nA - 1 - b - D;" in b7
    for k in range(448, 993, 32):                                       # the loop restated: r = (nA - 1) mod 6 for every nA that occurs
        for g0, na in BR.wave_ranges7(k):
            assert na >= BR.RING7 + 1 and BR.tail_variant7(na) == (na - 1) % BR.RING7
        rs = BR.wave_ranges7(k)
        assert rs[0][0] == 0 and all(rs[w][0] + rs[w][1] == (rs[w + 1][0] if w < 3 else k // 16) for w in range(4))
    u14 = b14[b14.index("int dense_block14_units("):b14.index("size_t dense_block14_scratch_halfs(")]
    assert "int n = 4;" in u14 and "n += (K0 + 32 * l - 32 + 63) / 64 + 1 + 6;" in u14
    assert "G = K - 32, nsu = (G + 63) / 64;" in b14 and "const int c = G + 16 * (ln >> 5) + 8 * ks + j;" in b14
    u28 = b28[b28.index("int dense_block28_units("):b28.index("size_t dense_block28_scratch_halfs(")]
    assert "int n = 1 + 4;" in u28 and "n += 4 * ((K0 + 32 * l + 63) / 64 + 6);" in u28
    assert BR.units(14, 256, 24) == 4 + sum((256 + 32 * l - 32 + 63) // 64 + 7 for l in range(24)) and BR.units(28, 128, 1) == 5 + 4 * 8
    assert BR.tail_order14(288)[:16] == list(range(256, 264)) + list(range(272, 280)) and sorted(BR.tail_order14(288)) == list(range(256, 288))
    # the predicates
    assert "return H == 7 && W == 7 && K0 % 32 == 0 && K0 >= 64 * (kRingDepth + 1) && nl >= 1 && K0 + 32 * nl <= 1024;" in b7
    assert "return H == 14 && W == 14 && K0 % 32 == 0 && K0 >= 256 && nl >= 1 && K0 + 32 * nl <= kScrChannels;" in b14
    assert "constexpr int kScrPlanes = 64;" in b14 and "constexpr int kScrChannels = 16 * kScrPlanes;" in b14 and "constexpr int kFrameScrB = kScrPlanes * kPlaneB;" in b14
    assert "return H == 28 && W == 28 && K0 % 32 == 0 && K0 >= 128 && nl >= 1 && K0 + 32 * (nl - 1) <= 512;" in b28
    assert "constexpr int kPlanes = 36;" in b28
    # the highest scratch plane a ring refill names (plane = 4 super-step + k-step) lies inside what a frame has
    assert max(4 * BR.nsu(14, k) - 1 for k in range(256, 993, 32)) == 59 < 64
    assert max(4 * BR.nsu(28, k) - 1 for k in range(128, 513, 32)) == 31 and max(k // 16 + 1 for k in range(128, 513, 32)) == 33 < 36


def test_refusal_rule():
    assert BR.accepted_k0(7) == list(range(448, 993, 32)) and BR.accepted_k0(14) == list(range(256, 993, 32)) and BR.accepted_k0(28) == list(range(128, 513, 32))
    assert BR.supported(14, 256, 24) and BR.supported(14, 512, 16) and not BR.supported(14, 256, 25) and not BR.supported(14, 1024, 1)
    assert BR.supported(28, 128, 13) and not BR.supported(28, 128, 14) and BR.supported(7, 448, 18) and not BR.supported(7, 448, 19)
    for h in BR.SIZES:
        rows = BR.refusals(h)
        assert len(rows) == (8 if h == 14 else 7)
        for k0, nl, ldc, b, names in rows:
            assert not BR.launchable(h, k0, nl, ldc, b), (h, k0, nl, ldc, b)
            assert "%d x %d" % (h, h) in names
        assert [BR.supported(h, *r[:2]) for r in rows] == [False] * (len(rows) - 3) + [True] * 3
        assert rows[0][0] == {7: 416, 14: 224, 28: 96}[h]
        assert rows[3][0] + 32 * rows[3][1] == (1056 if h != 28 else 576) and (h != 28 or rows[3][0] + 32 * (rows[3][1] - 1) == 544)
    assert BR.refusals(14)[4][0] + 32 * BR.refusals(14)[4][1] == 2048


def test_seams_are_planted_in_every_input_channel():
    assert np.argwhere(BR.seam_mask(7)[1:6, 1:6]).tolist() == [[3, 2], [3, 3]]            # pixels 31 | 32 (pixel 48 is a corner)
    assert BR.seam_mask(14)[:, 5].nonzero()[0].tolist() == [0, 3, 4, 7, 8, 11, 12, 13]
    assert BR.seam_mask(28, False)[:, 5].nonzero()[0].tolist() == [0, 7, 8, 15, 16, 23, 24, 26, 27] and BR.seam_mask(28).all()
    assert BR.channel_seams(7, 448, 1) == [111, 112, 223, 224, 335, 336]                  # G = 28: seven k-steps per wave
    assert BR.channel_seams(7, 480, 1) == [127, 128, 255, 256, 367, 368]                  # G = 30: 8, 8, 7, 7
    assert BR.channel_seams(14, 256, 1) == [63, 64, 127, 128, 191, 192, 223, 224]
    assert BR.channel_seams(28, 160, 1) == [63, 64, 127, 128]
    for h in BR.SIZES:
        k0 = BR.MIN_K0[h]
        x, layers = BR.noisy(h, k0, 2, 2, 1)
        x = np.abs(x.astype(np.float32))
        m, cs = BR.seam_mask(h, wave_seams=False), BR.channel_seams(h, k0, 2)
        assert np.all((x[:, m] >= 20) & (x[:, m] <= 60)) and np.all((x[..., cs] >= 20) & (x[..., cs] <= 60))
        rest = np.ones(k0, bool)
        rest[cs] = False
        assert x[1][~m][:, rest].max() < 12 and len(layers) == 2
    d = BR.dirty(14, 256, 2, 0).astype(np.float32)
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (np.abs(d[np.isfinite(d)]) > 5e4).any()
