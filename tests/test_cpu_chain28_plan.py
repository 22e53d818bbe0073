"""-m "not gpu": the route step for the tile-kernel layers of a 28x28 block (csrc/encoder_plan.h: enc_chain28, chain28_min_batch), asked
through tn_dbg_encoder_plan, which touches no device.

At 224 x 224 the second dense block runs K = 128 ... 288 as one chained strip launch and K = 320 as a strip launch; K = 352 ... 480 are
tile-kernel layers.  Below chain28_min_batch (128 frames) they are five `dense_layer_fused_28x28` launches, from it on one
`dense_block_chained_28x28` launch whose flops and bytes are the five layers' summed in order - the same double arithmetic, so the
comparison is exact.  TN_NO_CHAIN28, TN_NO_CHAIN, TN_CHAIN28_MIN_BATCH, the exact-weights mode and TN_DL_VARIANT each give the five
launches back, and every entry of tests/golden/encoder_routes.json (batches up to 64) reads as it did."""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_routes.json")
SWITCHES = ("TN_NO_FUSE", "TN_NO_CHAIN", "TN_NO_CHAIN28", "TN_CHAIN28_MIN_BATCH", "TN_NO_BLOCK7", "TN_NO_BLOCK14", "TN_BLOCK28", "TN_NO_STRIP",
            "TN_NO_STRIP_CHAIN", "TN_DL_VARIANT", "TN_STRIP_MIN_BATCH")
FUSED, CHAINED = "dense_layer_fused_28x28", "dense_block_chained_28x28"
KS = (352, 384, 416, 448, 480)


@pytest.fixture(scope="module")
def lib():
    from tennis_amd import _lib
    return _lib.load()


def plan(lib, monkeypatch, batch, env=None, flags=0, size=224):
    """{family: (launches, flops, bytes)} and the family order of tn_dbg_encoder_plan under the TN_* environment `env`"""
    from tennis_amd import _lib
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    stats = (_lib.TnKernelStat * 16)()
    n = C.c_int(0)
    rc = lib.tn_dbg_encoder_plan(size, size, flags, batch, 0, stats, 16, C.byref(n))
    assert rc == 0, (rc, lib.tn_last_error())
    rows = [[stats[i].name.decode(), stats[i].launches, stats[i].flops, stats[i].bytes] for i in range(n.value)]
    return {r[0]: tuple(r[1:]) for r in rows}, rows


def five_layers(batch):
    """flops and bytes of the five layers as encoder_plan.h::layer_cost states them, summed in layer order"""
    m = batch * 28 * 28
    flops = bytes_ = 0.0
    for k in KS:
        flops += 2.0 * m * (128.0 * k + 32.0 * 1152)
        bytes_ += float(m) * (k + 32) * 2 + 128.0 * k * 2 + 32.0 * 1152 * 2
    return flops, bytes_


@pytest.mark.parametrize("batch", [127, 128, 256])
def test_threshold_and_cost(lib, monkeypatch, batch):
    fams, rows = plan(lib, monkeypatch, batch)
    off, rows_off = plan(lib, monkeypatch, batch, {"TN_NO_CHAIN28": "1"})
    assert off[FUSED][0] == 5 and CHAINED not in off
    assert (off[FUSED][1], off[FUSED][2]) == five_layers(batch)
    if batch < 128:
        assert rows == rows_off
    else:
        assert FUSED not in fams and fams[CHAINED] == (1,) + five_layers(batch)
        assert fams[CHAINED][1:] == off[FUSED][1:]
        # nothing else moved: the other families, in their order, with the chained launch where the five were
        assert [r if r[0] != FUSED else [CHAINED, 1, r[2], r[3]] for r in rows_off] == rows
    # the strip routes in front of it are what they were
    assert fams["dense_block_strip_28x28"][0] == 1 and fams["dense_layer_strip_28x28"][0] == 1
    assert fams["dense_block_strip_56x56"][0] == 1 and fams["dense_layer_strip_56x56"][0] == 1
    assert fams["dense_block_stream_14x14"][0] == 1 and fams["dense_block_lds_7x7"][0] == 1


@pytest.mark.parametrize("env,flags", [({"TN_NO_CHAIN28": "1"}, 0), ({"TN_NO_CHAIN": "1"}, 0), ({"TN_CHAIN28_MIN_BATCH": "257"}, 0),
                                       ({"TN_DL_VARIANT": "8"}, 0), ({"TN_DL_VARIANT": "128"}, 0), ({}, "exact")],
                         ids=["no_chain28", "no_chain", "min_batch_257", "variant8", "variant128", "exact"])
def test_every_switch_gives_the_five_launches_back(lib, monkeypatch, env, flags):
    from tennis_amd import _lib
    fams, _ = plan(lib, monkeypatch, 256, env, _lib.ENC_EXACT_WEIGHTS if flags == "exact" else 0)
    assert CHAINED not in fams
    # (exact weights and a tuning variant keep the whole block on the tile kernel: twelve launches; the switches leave the strip routes)
    assert fams[FUSED][0] == (12 if flags == "exact" or "TN_DL_VARIANT" in env else 5)


def test_threshold_moves_with_its_switch_and_not_with_the_strip_one(lib, monkeypatch):
    assert CHAINED in plan(lib, monkeypatch, 64, {"TN_CHAIN28_MIN_BATCH": "64"})[0]
    assert CHAINED not in plan(lib, monkeypatch, 63, {"TN_CHAIN28_MIN_BATCH": "64"})[0]
    for b in (2, 63, 64, 127):
        assert CHAINED not in plan(lib, monkeypatch, b, {"TN_STRIP_MIN_BATCH": "1"})[0], b
    # without the strip kernels the whole block is tile-kernel layers, K = 128 ... 480: one launch of twelve
    fams, _ = plan(lib, monkeypatch, 128, {"TN_NO_STRIP": "1"})
    assert fams[CHAINED][0] == 1 and FUSED not in fams
    # other maps: a 448 x 448 input has a 28 x 28 block whose layers pass the tile kernel's K = 512; it stays per layer
    fams, _ = plan(lib, monkeypatch, 128, size=448)
    assert CHAINED not in fams


def test_every_golden_entry_is_unchanged(lib, monkeypatch):
    with open(FIXTURE) as f:
        entries = json.load(f)
    assert len(entries) >= 30
    for e in entries:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        _, rows = plan(lib, monkeypatch, e["batch"], e["env"], e["flags"], e["size"])
        assert rows == e["families"], e
        assert not any(r[0] == CHAINED for r in rows)
    # the entries the threshold was placed for: 224 x 224 at 2, 63 and 64 frames keep five per-layer launches
    for b in (2, 63, 64):
        assert plan(lib, monkeypatch, b)[0][FUSED][0] >= 5
