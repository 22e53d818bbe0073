"""-m "not gpu": the float64 reference, the derived bound, the input generators, the instantiation table and the case list of
tests/tools/layerwise_ref.py, checked on their own - they are what tests/test_gpu_layerwise_instantiations.py holds every
conv1x1_kernel<MI, POOL, NB, EX, ONCE>, trans_ws_kernel<NK, BM, NB> and conv3x3_kernel<V, EX> to.

  * INSTANTIATIONS is the set of template argument lists at the hipLaunchKernelGGL / launch_tws<...> sites of csrc/conv1x1.hip,
    csrc/trans_ws.hip and csrc/conv3x3.hip, parsed as text: an instantiation added later fails here until it is listed, and thereby run;
  * every GPU case reaches, by the restated dispatch rules, the instantiation it names, and every instantiation has a `noisy` and an
    `integer` case;
  * an fp32 model of the arithmetic stays inside the bound on `noisy` inputs and reproduces the `integer` ones bit for bit;
  * the same model with one defect at a time leaves the bound on `noisy` inputs or changes the `integer` result (the figures:
    docs/numerics.md "The transition and layer-wise kernels, every instantiation");
  * the conditions that make the pooled `integer` inputs see the lo operand hold for every pooled case;
  * tn_dbg_pack_trans_frags (the host packer tn_densenet121_create calls; no device) against a numpy restatement of the fragment order.

Near the bound's reach on real-valued inputs, listed and not worked around: the lo operand of the pooled mean missing (|lo| <= u a is
what the rounding of y allows; the planted channels carry it outside, by 1.3 at the least) and the bias added behind the rounding (a
double rounding: outside in the cases with thousands of outputs, inside at M = 1); the `integer` inputs see the first in every case and
the second in the pooled case."""
import os
import re

import numpy as np
import pytest

from tools import layerwise_ref as LR

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tennis_amd", "csrc")
SMALL = [c for c in LR.ALL_CASES if c["M"] <= 1200]
_cache = {}


def _ref(c):
    """inputs and reference of a case, computed once and left unchanged"""
    if c["id"] not in _cache:
        inp = LR.make(c)
        out = LR.reference(inp)
        for a in (*out, *(v for v in inp.values() if isinstance(v, np.ndarray))):
            a.setflags(write=False)
        _cache[c["id"]] = (inp, out)
    return _cache[c["id"]]


def _targs(text, n):
    vals = [int(a) if a.strip().isdigit() else a.strip() == "true" for a in text.split(",")]
    return tuple(vals + [False] * (n - len(vals)))


def test_instantiation_table_equals_the_sources():
    found = []
    src = open(os.path.join(CSRC, "conv1x1.hip")).read()
    found += [("conv1x1_kernel", _targs(m, 5)) for m in re.findall(r"hipLaunchKernelGGL\(\(?conv1x1_kernel<([^>]*)>", src)]
    src = open(os.path.join(CSRC, "trans_ws.hip")).read()
    found += [("trans_ws_kernel", _targs(m, 3)) for m in re.findall(r"launch_tws<([\d, ]*)>\(a, s\)", src)]
    src = open(os.path.join(CSRC, "conv3x3.hip")).read()
    found += [("conv3x3_kernel", _targs(m, 2)) for m in re.findall(r"hipLaunchKernelGGL\(\(?conv3x3_kernel<([^>]*)>", src)]
    assert len(found) == len(set(found)) == 12 + 4 + 3, found
    assert set(found) == set(LR.INSTANTIATIONS), (sorted(set(found) - set(LR.INSTANTIATIONS)), sorted(set(LR.INSTANTIATIONS) - set(found)))


def test_the_dispatch_rules_are_the_sources():
    """the constants ``instantiation_of`` restates, as they stand in the launchers"""
    c1 = open(os.path.join(CSRC, "conv1x1.hip")).read()
    for text in ("a.M >= 128 * 512", "a.M >= 64 * 512", "a.N % 256 == 0", "NT == 1 && !no_nt && (size_t)a.M * 4 * a.ldx * sizeof(f16) > (nt_mb << 20)",
                 "(size_t)atoi(getenv(\"TN_TRANS_NT_MB\")) : 128", "a.wfrag && !no_ws && trans_ws_supported(a)"):
        assert text in c1, text
    ws = open(os.path.join(CSRC, "trans_ws.hip")).read()
    for text in ("a.K == 16 * BK ? launch_tws<16, 64, 512>", "a.K == 8 * BK ? launch_tws<8, 128, 256>", "if (a.N == 512)", "constexpr int BK = 64;",
                 "a.pool && !a.exact && !a.bias && (a.N == 512 || a.N == 256) && a.K % (2 * BK) == 0 && a.H % 2 == 0 && a.W % 2 == 0"):
        assert text in ws, text
    c3 = open(os.path.join(CSRC, "conv3x3.hip")).read()
    assert "if (a.exact)" in c3 and "else if (a.variant == 9)" in c3


def test_every_case_reaches_the_instantiation_it_names():
    for c in LR.ALL_CASES:
        assert LR.instantiation_of(LR.launch_args(c), c["nt_mb"]) == c["inst"], c["id"]
        assert c["inst"] in LR.INSTANTIATIONS
    for c in LR.ONCE_CASES:                                     # ... and in a process with the default threshold they are the plain ones
        assert LR.instantiation_of(LR.launch_args(c)) == (c["inst"][0], c["inst"][1][:4] + (False,))
    for inst in LR.INSTANTIATIONS:
        for gen in ("noisy", "integer"):
            assert any(c["inst"] == inst and c["gen"] == gen for c in LR.ALL_CASES), (inst, gen)
    # the edges the cases are there for
    ids = {c["id"] for c in LR.CASES}
    assert {"c1-M65541-K96-N128-exact-bias-noisy", "c1-M32775-K64-N128-integer", "c1-M1-K64-N128-bias-noisy", "pool-2x15x15-K96-N384-integer",
            "pool-1x6x6-K64-N128-noisy", "ws-3x30x30-K512-N256-integer", "ws-3x2x2-K128-N512-noisy", "c3-3x7x7-v9-integer", "c3-1x2x240-v0-exact-noisy"} <= ids
    assert any(c["op"] == "pool" and (c["M"] + 63) // 64 >= 9 for c in LR.CASES)          # a second group of eight pixel tiles
    nts = {c["N"] // c["inst"][1][2] for c in LR.CASES if c["op"] == "pool" and not c["exact"]}
    assert nts == {1, 2, 3, 4}


@pytest.mark.parametrize("c", [c for c in SMALL if c["gen"] == "noisy"], ids=lambda c: c["id"])
def test_fp32_model_stays_inside_the_bound(c):
    inp, (y, e16, y32, e32) = _ref(c)
    my, my32 = LR.model(inp)
    r16, r32 = LR.ratio(my, y, e16), LR.ratio(my32, y32, e32)
    print("model %s: max |err| / E  y %.3f  y32 %.3f  (|y| max %.3g)" % (c["id"], r16, r32, np.abs(y).max()))
    assert r16 <= 1.0 and r32 <= 1.0
    assert r16 > 0.03                      # a bound the model does not come near would not be a bound on anything


@pytest.mark.parametrize("c", [c for c in SMALL if c["gen"] == "integer"], ids=lambda c: c["id"])
def test_integer_inputs_are_exact(c):
    """What makes the GPU test's bit comparison legitimate: the float64 values are fp32 numbers, the fp32 model - any summation order -
    reproduces them, and its fp16 output is their round-to-nearest-even half."""
    inp, (y, _, y32, _) = _ref(c)
    assert np.array_equal(y32.astype(np.float32).astype(np.float64), y32) and np.abs(y32).max() < 2.0 ** 22 / 4
    assert np.array_equal(4 * y32, np.round(4 * y32)) and len(np.unique(y32)) > 15
    my, my32 = LR.model(inp)
    assert np.array_equal(my32.astype(np.float64), y32)
    assert np.array_equal(my.astype(np.float16).view(np.uint16), y.astype(np.float16).view(np.uint16))
    if c["op"] == "c1":
        assert np.array_equal(y, np.round(y)) and np.array_equal(y.astype(np.float16).astype(np.float64), y)
    if "w_lo" in inp:                       # independent patterns in the two halves
        assert not np.array_equal(inp["w"] != 0, inp["w_lo"] != 0)


@pytest.mark.parametrize("c", [c for c in LR.ALL_CASES if c["op"] in ("pool", "ws") and c["gen"] == "integer"], ids=lambda c: c["id"])
def test_integer_pool_conditions(c):
    inp = LR.make(c)
    a, _ = LR.operand(inp)
    assert a.min() >= 512 and a.max() < 1024 and np.array_equal(4 * a, np.round(4 * a))
    hi = a.astype(np.float16).astype(np.float64)
    lo = a - hi
    assert np.all(np.isin(lo, (-0.25, 0.0, 0.25)))
    assert (lo != 0).mean() >= 0.25
    w = inp["w"]
    assert np.all(np.isin(w, (-1, 0, 1))) and np.all(w.sum(axis=1) == 0) and np.all((w != 0).sum(axis=0) >= 1)      # balanced; every input channel used
    assert ((lo != 0).astype(np.float64) @ (w != 0).astype(np.float64).T).min() >= 1                                # every output sums a lo != 0 operand
    # the dropped row and column of an odd map hold numbers, and the reference does not see them
    if c["H"] % 2:
        other = dict(inp, x=inp["x"].copy())
        other["x"][:, c["H"] - 1] = 7
        other["x"][:, :, c["W"] - 1] = 7
        assert np.array_equal(LR.operand(other)[0], a)


# defect -> the cases it applies to
def _applies(defect, c):
    pooled = c["op"] in ("pool", "ws")
    return {"no_lo": pooled, "drop_tail": c["op"] != "c3" and c["K"] % 64 == 32, "double_tail": c["op"] != "c3" and c["K"] % 64 == 32,
            "no_wrap": c["op"] != "c3" and c["exact"], "pool_neighbour": pooled, "pool_next_frame": pooled and c["B"] > 1,
            "bias_after": c["bias"], "clamp_as_bn": c["clamp"], "frame_border": c["op"] == "c3" and c["B"] > 1,
            "lo_at_hi": c["op"] == "c3" and c["exact"],
            "drop_partial": c["op"] == "c3" and c["H"] > 1}[defect]         # (every tap of the fourth partial sum lies in the row below)


SUBTLE = {"no_lo", "bias_after"}           # of the size of a rounding: at least one `noisy` case has to leave the bound, not every one
EXACT_ANYWAY = {("bias_after", "c1")}       # a second rounding of a small integer changes nothing: the pooled case's quarter-integers see it


def _worst(got, want, bound):
    r = LR.ratio(got, want, bound)
    return r if np.isfinite(r) else np.inf    # an overflow has left the bound


@pytest.mark.parametrize("defect", LR.DEFECTS)
def test_every_defect_leaves_the_bound_or_changes_the_integers(defect):
    cases = [c for c in SMALL if _applies(defect, c) and c["M"] <= 700 and c["K"] <= 512]
    assert any(c["gen"] == "noisy" for c in cases) and any(c["gen"] == "integer" for c in cases), defect
    left = []
    for c in cases:
        inp, (y, e16, y32, e32) = _ref(c)
        with np.errstate(all="ignore"):
            dy, dy32 = LR.model(inp, defect, LR.x_buffer(c, inp))
        if c["gen"] == "noisy":
            r16, r32 = _worst(dy, y, e16), _worst(dy32, y32, e32)
            print("%s on %s: max |err| / E  y %.3g  y32 %.3g" % (defect, c["id"], r16, r32))
            left.append(max(r16, r32 if c["op"] != "c3" else 0.0) > 1.0)
        elif (defect, c["op"]) not in EXACT_ANYWAY:
            same = np.array_equal(dy32.astype(np.float64), y32) and np.array_equal(dy.astype(np.float16).view(np.uint16), y.astype(np.float16).view(np.uint16))
            assert not same, (defect, c["id"])
    assert any(left) if defect in SUBTLE else all(left), (defect, left)
    if defect == "bias_after":
        assert any(c["gen"] == "integer" and c["op"] == "pool" for c in cases)


def test_plants_sit_where_the_kernels_change_owner():
    c = next(c for c in LR.CASES if c["id"] == "ws-3x30x30-K512-N256-noisy")
    rows = set(LR.seam_rows(c).tolist())
    assert {0, 112, 113, 224, 225 + 112, 225 + 113, 31, 32, 113 + 31, 113 + 32} <= rows         # tiles of 113 and 112 rows, 32-row fragments
    c = next(c for c in LR.CASES if c["id"] == "pool-2x15x15-K96-N384-noisy")
    x = np.abs(LR.make(c)["x"].astype(np.float32))
    assert x[:, 14].min() >= 20 and x[:, :, 14].min() >= 20 and x[:, 12:14, :14].min() >= 20 and x[:, :14, 12:14].min() >= 20
    assert x[:, 3, 3, 1:-1].max() < 12
    c = next(c for c in LR.CASES if c["id"] == "c3-3x7x7-v0-noisy")
    x = np.abs(LR.make(c)["x"].astype(np.float32)).reshape(-1, 128)
    assert x[[127, 128, 48, 49, 97, 98, 146]].min() >= 20 and x[8].max() < 12                   # the tile seam inside the third frame, frame borders
    c = next(c for c in LR.CASES if c["id"] == "c1-M300-K96-N256-bias-clamp-noisy")
    x = np.abs(LR.make(c)["x"].astype(np.float32))
    assert x[[0, 31, 32, 63, 64, 299]].min() >= 20 and x[:, [0, 88, 95]].min() >= 20 and x[5, 1:88].max() < 12


@pytest.mark.parametrize("n,k", [(512, 1024), (256, 128), (32, 16), (64, 48)])
def test_host_fragment_packer_against_the_restated_order(n, k):
    """tn_dbg_pack_trans_frags -> pack_trans_frags, the function tn_densenet121_create packs the transitions' weights with: every cell
    holds a different number, so the image is the order."""
    from tennis_amd import _lib
    lib = _lib.load()
    w = np.arange(n * k, dtype=np.uint16).reshape(n, k)        # bit patterns, all different
    out = np.zeros(n * k, np.uint16)
    assert lib.tn_dbg_pack_trans_frags(w.ctypes.data, n, k, out.ctypes.data) == 0
    want = LR.frag_order(w)
    assert np.array_equal(out, want)
    cells = out.reshape(k // 16, n // 32, 64, 8)                # lane l of fragment (g, ct): row 32 ct + (l & 31), k = 16 g + 8 (l >> 5) ...
    for g, ct, l in ((0, 0, 0), (k // 16 - 1, n // 32 - 1, 63), (0, n // 32 - 1, 33)):
        assert np.array_equal(cells[g, ct, l], w[32 * ct + (l & 31), 16 * g + 8 * (l >> 5):16 * g + 8 * (l >> 5) + 8])
    assert lib.tn_dbg_pack_trans_frags(w.ctypes.data, 48, 16, out.ctypes.data) != 0 and b"N % 32" in lib.tn_last_error()
    assert lib.tn_dbg_pack_trans_frags(None, n, k, out.ctypes.data) != 0 and b"null" in lib.tn_last_error()
