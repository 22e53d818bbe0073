"""-m "not gpu": the float64 reference, the derived bound, the input generators and the instantiation table of tests/tools/tile_ref.py,
checked on their own - they are what tests/test_gpu_tile_instantiations.py holds every dense_layer_kernel<W, ROUT, BM, BK, PP, CHAIN, EX>
to.

  * an fp32 model of the kernel's arithmetic (float32 accumulation over 32 channels per step, the fp32 fma of BN2, the two fp16
    roundings, one accumulator per output; exact mode: hi pass then lo pass, 18 taps) stays inside the bound on the `noisy` inputs - one
    case per k-tile size, one exact case, K % 64 == 32 at BK = 64 with and without exact weights;
  * the same model with one defect at a time leaves it: a 3x3 product missing, an input channel of the 1x1 missing, the halo row above a
    row-tile seam taken from the wrong side, either padding column not zero, either tile row past the image edge not zero, and - exact
    mode - the lo pass reading its activations from channel Kp onward instead of wrapping to channel 0;
  * the `integer` and `chain_integer` cases are exact in float64 and in the model and change under every defect, a single missing
    product at an arbitrary position and the missing wrap included;
  * `seam_lines` and the restated geometry constants agree with csrc/dense_layer_big.hip, and the set of template argument lists at its
    launch_geom<...> / TN_GEOM(...) call sites, parsed as text, is the set in INSTANTIATIONS: an instantiation added later fails here
    until it is listed, and thereby run.

Outside the bound's reach on real-valued inputs, listed and not worked around: see tools/tile_ref.py.  The missing wrap is one of them
where nothing large sits behind the layer's channels (the lo halves are 2^-11 of the weights): on the `noisy` inputs it leaves the bound
through the SENTINEL the GPU test's buffer holds there, at the tightest row pitch (where it finds the next pixel's activations) it may
not; the `integer` inputs see it at every pitch."""
import os
import re

import numpy as np
import pytest

from tools import tile_ref as TR

MODEL_CASES = [(28, 96, False), (14, 160, True), (7, 544, False), (16, 64, True)]      # (H, K, exact)
IDS = ["%d-%d%s" % (h, k, "-exact" if e else "") for h, k, e in MODEL_CASES]
HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tennis_amd", "csrc", "dense_layer_big.hip")
_cache = {}


def _case(h, k, exact):
    """inputs, reference and bound of a `noisy` case, computed once and left unchanged"""
    key = (h, k, exact)
    if key not in _cache:
        inp = TR.noisy(h, k, 1, 0, exact)
        y, bound = TR.reference(inp)
        for a in (y, bound, *inp.values()):
            a.setflags(write=False)
        _cache[key] = (inp, y, bound)
    return _cache[key]


def _wide_behind(inp, h, k):
    """what sits behind channel Kp in the buffer of the GPU test at a pitch with room behind the output (SENTINEL)"""
    return TR.behind(TR.buffer(inp["x"], TR.smallest_ldc(k) + 64), TR.kp_of(h, k), k)


@pytest.mark.parametrize("h,k,exact", MODEL_CASES, ids=IDS)
def test_fp32_model_stays_inside_the_bound(h, k, exact):
    """Worst ratios of the model (recorded in docs/numerics.md): 0.26 at (28, 96), 0.17 at (14, 160, exact), 0.07 at (7, 544), 0.20 at
    (16, 64, exact)"""
    inp, y, bound = _case(h, k, exact)
    r = TR.ratio(TR.model(inp), y, bound)
    print("fp32 model at %d x %d, K = %d%s: max |err| / E = %.3f, |y| max %.3g, E median %.3g" % (h, h, k, ", exact" if exact else "", r, np.abs(y).max(),
                                                                                              np.median(bound)))
    assert r <= 1.0
    assert r > 0.05          # a bound the model does not come near would not be a bound on anything


def _defects(inp, h, k, exact):
    # the product of output channel 5's largest weight (see tools/tile_ref.py on what a bound on real-valued inputs can see of one product)
    tap = (5, *(int(i) for i in np.unravel_index(np.abs(inp["w3"][5]).argmax(), (128, 3, 3))))
    seam = TR.rout(h) if TR.rout(h) < h else h // 2
    d = {"one 3x3 product missing from one output channel": dict(drop_tap=tap),
         "input channel k of the 1x1 missing": dict(drop_k=k - 3),
         "halo row above a row-tile seam taken from the wrong side": dict(seam_row=seam),
         "padding slot 0 of a tile row not zero": dict(pad_col=0),
         "padding slot W + 1 of a tile row not zero": dict(pad_col=1),
         "tile row above the image (top_pad) not zero": dict(edge_row=0),
         "tile row below the image (last tile) not zero": dict(edge_row=1)}
    if exact:
        d["lo pass reads from channel Kp onward instead of wrapping"] = dict(no_wrap=_wide_behind(inp, h, k))
    return d


@pytest.mark.parametrize("h,k,exact", MODEL_CASES, ids=IDS)
def test_every_listed_defect_leaves_the_bound(h, k, exact):
    inp, y, bound = _case(h, k, exact)
    for name, kw in _defects(inp, h, k, exact).items():
        err = np.abs(TR.model(inp, **kw).astype(np.float64) - y) / bound
        print("%d x %d, K = %d%s, %s: max |err| / E = %.3g at %s" % (h, h, k, ", exact" if exact else "", name, err.max(), np.unravel_index(err.argmax(), err.shape)))
        assert err.max() > 1.0, name
    # each defect is seen where it is
    e = np.abs(TR.model(inp, drop_tap=_defects(inp, h, k, exact)["one 3x3 product missing from one output channel"]["drop_tap"]).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 1, 2)).nonzero()[0].tolist() == [5]
    seam = TR.rout(h) if TR.rout(h) < h else h // 2
    e = np.abs(TR.model(inp, seam_row=seam).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 2, 3)).nonzero()[0].tolist() == [seam]
    e = np.abs(TR.model(inp, pad_col=0).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 1, 3)).nonzero()[0].tolist() == [0]
    e = np.abs(TR.model(inp, pad_col=1).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 1, 3)).nonzero()[0].tolist() == [h - 1]
    e = np.abs(TR.model(inp, edge_row=0).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 2, 3)).nonzero()[0].tolist() == [0]
    e = np.abs(TR.model(inp, edge_row=1).astype(np.float64) - y) / bound
    assert (e > 1.0).any(axis=(0, 2, 3)).nonzero()[0].tolist() == [h - 1]


def _integer_is_exact(inp, y, exact):
    assert set(np.unique(inp["x"].astype(np.float32))) <= {0.0, 1.0}
    w1, w3, t2 = inp["w1"], inp["w3"], inp["t2"]
    assert np.all(np.isin(w1, (-1, 0, 1))) and np.all((w1 != 0).sum(axis=1) == 16) and np.all((w1 != 0).sum(axis=0) >= 1)
    assert np.all(np.isin(w3, (-1, 0, 1))) and np.all((w3 != 0).sum(axis=0) == 1) and np.all((w3 != 0).sum(axis=(1, 2, 3)) == 36)
    assert np.all(t2 == np.round(t2)) and np.abs(t2).max() <= (4 if exact else 8) and np.all(inp["s2"] == 1)
    if exact:
        l1, l3 = inp["w1_lo"], inp["w3_lo"]
        assert np.all(np.isin(l1, (-1, 0, 1))) and np.all((l1 != 0).sum(axis=1) == 8)
        assert np.all(np.isin(l3, (-1, 0, 1))) and np.all((l3 != 0).sum(axis=0) == 1) and np.all((l3 != 0).sum(axis=(1, 2, 3)) == 36)
        assert not np.array_equal(l1 != 0, w1 != 0) and not np.array_equal(l3 != 0, w3 != 0)        # independent patterns
    assert np.array_equal(y, np.round(y)) and np.abs(y).max() <= (2016 if exact else 864) and np.abs(y).max() > 30
    assert np.array_equal(y.astype(np.float16).astype(np.float64), y)
    assert len(np.unique(y)) > 40                                               # not a degenerate map


@pytest.mark.parametrize("h,k,exact", MODEL_CASES + [(56, 32, False), (64, 1024, True), (32, 544, True), (14, 1024, False), (7, 32, True)],
                         ids=lambda v: str(int(v)))
def test_integer_inputs_are_exact_in_float64(h, k, exact):
    """What makes the GPU test's bit comparison legitimate: every intermediate of the `integer` case is an integer small enough for the
    format that holds it (|bott| <= 24 / 28, |y| <= 864 / 2016 < 2048)."""
    inp = TR.integer(h, k, 1, 0, exact)
    y, _ = TR.reference(inp)
    _integer_is_exact(inp, y, exact)


@pytest.mark.parametrize("h,k,exact", MODEL_CASES, ids=IDS)
def test_integer_inputs_change_under_every_defect(h, k, exact):
    inp = TR.integer(h, k, 1, 0, exact)
    y, _ = TR.reference(inp)
    assert np.array_equal(TR.model(inp).astype(np.float64), y)                  # the kernel's arithmetic reproduces the integers exactly
    rng = np.random.default_rng([h, k, 9])
    defects = dict(_defects(inp, h, k, exact))
    defects.pop("one 3x3 product missing from one output channel")
    for i in range(6):                                                          # a single missing product at an arbitrary position
        c, dy, dx = int(rng.integers(128)), int(rng.integers(3)), int(rng.integers(3))
        half = i % 2 if exact else 0
        o = int(np.flatnonzero(inp["w3_lo" if half else "w3"][:, c, dy, dx])[0])
        defects["product (%d, %d, %d, %d) of image half %d missing" % (o, c, dy, dx, half)] = dict(drop_tap=(o, c, dy, dx, half))
    defects["input channel %d of the 1x1 missing" % (k // 2 + 1)] = dict(drop_k=k // 2 + 1)
    if exact:                                                                   # the missing wrap, at the tightest pitch and a wide one
        defects["no wrap, tightest pitch"] = dict(no_wrap=TR.behind(TR.buffer(inp["x"], TR.smallest_ldc(k)), TR.kp_of(h, k), k))
    for name, kw in defects.items():
        assert not np.array_equal(TR.model(inp, **kw).astype(np.float64), y), name


@pytest.mark.parametrize("h,k0,n,exact", [(7, 64, 4, False), (16, 64, 3, True), (14, 128, 3, True)])
def test_chain_integer_is_exact(h, k0, n, exact):
    x, layers = TR.chain_integer(h, k0, n, 2, 0, exact)
    buf = TR.chain_reference(x, layers)
    assert buf.shape[-1] == k0 + 32 * n and np.array_equal(buf, np.round(buf)) and np.abs(buf).max() < 2048
    for l, p in enumerate(layers):
        k = k0 + 32 * l
        assert np.all(p["lo"] == 0) and np.all(p["hi"][:k0] == 65504) and np.all(p["hi"][k0:] == 1)
        inp = dict(x=np.clip(buf[..., :k], 0, None).astype(np.float16), **p)    # what the layer reads: the stored outputs
        y = buf[..., k:k + 32]
        assert np.array_equal(TR.model(dict(x=buf[..., :k].astype(np.float16), **p)).astype(np.float64), y)
        assert len(np.unique(y)) > 20 and inp["x"].shape[-1] == k
        a1 = np.clip(buf[..., :k], p["lo"], p["hi"])
        assert set(np.unique(a1)) <= {0.0, 1.0} and (l == 0 or 0.2 < a1[..., k0:].mean() < 0.8)      # each layer sees {0, 1} again


# ---- the geometry restated in the tool against the kernel's source ------------------------------------------------------------------
def _dispatch():
    """the template argument lists at the launch_geom<...>(a, s) / TN_GEOM(...) call sites of dense_layer_big.hip -> set of 7-tuples"""
    src = open(HIP).read()
    body = src[src.index("int launch_dense_layer_big("):]
    found = set()
    for m in re.finditer(r"launch_geom<([^>]*)>\(a, s\)", body):
        args = [a.strip() for a in m.group(1).split(",")]
        if not args[0].isdigit():
            continue                                                             # the macro's own definition
        vals = [int(a) if a.isdigit() else a == "true" for a in args]
        assert len(vals) >= 5
        vals += [False] * (7 - len(vals))
        found.add(tuple(vals))
    for m in re.finditer(r"TN_GEOM\(\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", body):
        g = tuple(int(v) for v in m.groups())
        found |= {g + (0, False, False), g + (2, False, False)}
    return found


def test_instantiation_table_equals_the_dispatch():
    found = _dispatch()
    table = {r["targs"] for r in TR.INSTANTIATIONS}
    assert len(TR.INSTANTIATIONS) == 30 and len(table) == 30
    assert found == table, (sorted(found - table), sorted(table - found))
    for r in TR.INSTANTIATIONS:
        w, ro, bm, bk, pp, chain, ex = r["targs"]
        assert w == r["h"] and chain == r["chained"] and ex == r["exact"]
        assert (ro, bk) == TR.GEOM[w][:2] and bm in TR.BMS[w]
        assert r["ks"] and all((k if not chain else k[0] + 32 * (k[1] - 1)) <= TR.kmax(w) for k in r["ks"])
    src = open(HIP).read()
    assert "KMAX = W == 56 ? 256 : W == 28 ? 512 : 1024" in src and [TR.kmax(w) for w in (56, 28, 14, 7, 64, 32, 16)] == [256, 512, 1024, 1024, 1024, 1024, 1024]
    assert "REBAL ? (wid < 4 ? wid * 64 : 256 + (wid - 4) * 48) : wid * (BM / 8)" in src and "G::NSPLIT ? (wid & 3) * 16" in src


def test_single_layer_k_sets():
    for h in TR.GEOM:
        for exact in (False, True):
            ks, bk, km = TR.single_ks(h, exact), TR.bk_of(h), TR.kmax(h)
            tiles = {(k + bk - 1) // bk for k in ks}
            assert {1, 2, 3, 4} <= tiles and km in ks and km - 32 in ks and all(k % 32 == 0 and 32 <= k <= km for k in ks)
            mid = [k for k in ks if 4 * bk < k < km - 32]
            assert any(k % 64 == 0 for k in mid) and any(k % 64 == 32 for k in mid)
    assert TR.single_ks(14, True) == [32, 64, 96, 128, 160, 192, 224, 256, 576, 608, 992, 1024]
    # chains: the smallest K0 the launcher accepts
    assert [TR.chain_min_k0(h, v, e) for h, v, e in ((14, 0, False), (16, 0, False), (7, 0, False), (7, 512, False), (7, 32, False), (14, 0, True), (16, 0, True),
                                                     (7, 0, True))] == [128, 64, 192, 128, 128, 128, 64, 128]


def test_seam_lines_follow_the_geometry():
    rows, cols, px = TR.seam_lines(56)
    assert rows == sorted({0, 55} | {r for s in range(7, 56, 7) for r in (s - 1, s)}) and cols == [0, 55]
    assert TR.seam_lines(28)[0] == [0, 13, 14, 27] and TR.seam_lines(64)[0] == sorted({0, 63} | {r for s in range(4, 64, 4) for r in (s - 1, s)})
    assert TR.seam_lines(32)[0] == [0, 7, 8, 15, 16, 23, 24, 31]
    for h in (16, 14, 7):
        assert TR.seam_lines(h)[0] == [0, h - 1]                                # whole-frame tiles: no seam inside
    # 56 x 56, first tile (image rows 0 ... 7 flattened): 64 rows per wave -> (1, 7) | (1, 8); second tile starts at image row 6
    assert {(1, 7), (1, 8), (7, 7), (7, 8)} <= set(px)
    # 28 x 28, first tile: waves 4 ... 7 start at flattened rows 256, 304, 352, 400 (REBAL)
    px28 = set(TR.seam_lines(28)[2])
    assert {divmod(m, 28) for m0 in (64, 128, 192, 256, 304, 352, 400) for m in (m0 - 1, m0)} <= px28
    # 7 x 7: 16-row groups of both wave splits, and phase B's fragments: srel = 9 row + column + 1 = 15 | 16 -> (1, 5) | (1, 6)
    px7 = set(TR.seam_lines(7)[2])
    assert {divmod(m, 7) for m0 in (16, 32, 48) for m in (m0 - 1, m0)} <= px7 and {(1, 5), (1, 6)} <= px7
    # 14 x 14: 32 rows per wave; fragments of 16 slots in rows of 16 slots: slot 15 is padding, slot 16 padding - nothing to plant
    px14 = set(TR.seam_lines(14)[2])
    assert px14 == {divmod(m, 14) for m0 in range(32, 196, 32) for m in (m0 - 1, m0)}
    x = TR.noisy(28, 64, 2, 3)["x"].astype(np.float32)
    m = TR.seam_mask(28)
    assert np.all((np.abs(x[:, m]) >= 20) & (np.abs(x[:, m]) <= 60))
    assert np.abs(x[:, ~m]).max() < 12 and (x[:, m] > 0).any() and (x[:, m] < 0).any()
