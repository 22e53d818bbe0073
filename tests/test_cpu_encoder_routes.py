"""The routing plan of the fp16 DenseNet-121 encoder (csrc/encoder_plan.h: what tn_densenet121_create packs by and what
encoder_run_range launches by) asked through tn_dbg_encoder_plan, which touches no device, against tests/golden/encoder_routes.json:
the families, launches, flops and bytes that DenseNet121Features.profile() reported on the GPU for every size, batch, TN_* environment
and create flag of the table (scripts/record_encoder_routes.py recorded it before the plan existed; tests/test_gpu_encoder_routes.py
holds the launches to it).  No GPU needed."""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_routes.json")
SWITCHES = ("TN_NO_FUSE", "TN_NO_CHAIN", "TN_NO_BLOCK7", "TN_NO_BLOCK14", "TN_BLOCK28", "TN_NO_STRIP", "TN_NO_STRIP_CHAIN",
            "TN_DL_VARIANT", "TN_STRIP_MIN_BATCH")
# the eight routes of a dense block by the family their launches are profiled under (geometry suffix apart), in precedence order
ROUTES = ("dense_block_stream_14x14", "dense_block_stream_28x28", "dense_block_lds_7x7", "dense_block_chained_", "dense_block_strip_",
          "dense_layer_strip_", "dense_layer_fused_", "conv1x1_bnrelu")
STEM = ("stem_conv_bn_relu_maxpool", "stem_conv7x7_bn_relu", "maxpool3x3s2")
LAYERWISE = STEM + ("conv1x1_bnrelu", "conv3x3_bnrelu", "transition_conv1x1_avgpool", "head_bnrelu_avgpool7")


def entries():
    with open(FIXTURE) as f:
        return json.load(f)


def entry_id(e):
    env = "+".join(f"{k}={v}" for k, v in sorted(e["env"].items())) or "default"
    return f"{e['size']}-b{e['batch']}-{env}-flags{e['flags']}"


@pytest.fixture(scope="module")
def lib():
    from tennis_amd import _lib
    return _lib.load()


def plan(lib, monkeypatch, size, batch, env, flags=0, calibrate=0):
    """[[name, launches, flops, bytes], ...] of tn_dbg_encoder_plan under the TN_* environment `env`"""
    from tennis_amd import _lib
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    stats = (_lib.TnKernelStat * 16)()
    n = C.c_int(0)
    rc = lib.tn_dbg_encoder_plan(size, size, flags, batch, calibrate, stats, 16, C.byref(n))
    assert rc == 0, (rc, lib.tn_last_error())
    assert all(stats[i].ms == 0 for i in range(n.value))
    return [[stats[i].name.decode(), stats[i].launches, stats[i].flops, stats[i].bytes] for i in range(n.value)]


def routes_reached(rows):
    return {r for e in rows for fam in e["families"] for r in ROUTES if fam[0].startswith(r)}


@pytest.mark.parametrize("entry", entries(), ids=entry_id)
def test_plan_equals_the_recorded_launches(lib, monkeypatch, entry):
    """names, launches, flops and bytes: exactly (the same double arithmetic in the same order)"""
    assert plan(lib, monkeypatch, entry["size"], entry["batch"], entry["env"], entry["flags"]) == entry["families"]


def test_calibration_pass_is_layerwise_whatever_the_switches(lib, monkeypatch):
    """calibrate = 1: only layer-wise families, and one list for every environment of the table (TN_NO_FUSE, which is not a
    routing switch alone, also splits the stem into its two kernels: those families apart)"""
    for size in (224, 448):
        want = plan(lib, monkeypatch, size, 2, {}, calibrate=1)
        assert {f[0] for f in want} <= set(LAYERWISE) and [f[1] for f in want if f[0].startswith("conv")] == [58, 58]
        for env in [e["env"] for e in entries()]:
            got = plan(lib, monkeypatch, size, 2, env, calibrate=1)
            assert {f[0] for f in got} <= set(LAYERWISE)
            assert [f for f in got if f[0] not in STEM] == [f for f in want if f[0] not in STEM], env
            if "TN_NO_FUSE" not in env:
                assert got == want, env


def test_strip_edge_lies_between_63_and_64_frames_and_moves_with_the_switch(lib, monkeypatch):
    def strips(batch, env):
        return any(f[0].startswith(("dense_layer_strip_", "dense_block_strip_")) for f in plan(lib, monkeypatch, 224, batch, env))
    assert not strips(63, {}) and strips(64, {})
    assert not strips(9, {"TN_STRIP_MIN_BATCH": "10"}) and strips(10, {"TN_STRIP_MIN_BATCH": "10"})
    assert strips(1, {"TN_STRIP_MIN_BATCH": "1"}) and not strips(64, {"TN_STRIP_MIN_BATCH": "65"})
    # 512 x 512: 5 workgroups per 128 x 128 frame, 3 per 64 x 64 frame
    fams = {b: [f[0] for f in plan(lib, monkeypatch, 512, b, {})] for b in (12, 13, 21, 22)}
    assert "dense_layer_strip_128x128" not in fams[12] and "dense_layer_strip_128x128" in fams[13]
    assert "dense_layer_strip_64x64" not in fams[21] and "dense_layer_strip_64x64" in fams[22]


def test_every_route_is_reached():
    assert routes_reached(entries()) == set(ROUTES)


def test_a_route_losing_its_only_entries_is_noticed():
    """what test_every_route_is_reached rests on: without the entries that reach any one route the set reached is no longer the full one"""
    rows = entries()
    for r in ROUTES:
        kept = [e for e in rows if not any(f[0].startswith(r) for f in e["families"])]
        assert len(kept) < len(rows) and r not in routes_reached(kept) and routes_reached(kept) != set(ROUTES)


def test_hook_refuses_what_create_refuses(lib):
    from tennis_amd import _lib
    stats = (_lib.TnKernelStat * 16)()
    n = C.c_int(0)
    out = (stats, 16, C.byref(n))
    assert lib.tn_dbg_encoder_plan(224, 224, 0, 2, 0, *out) == 0
    for h, w in ((223, 224), (224, 223), (1025, 224), (224, 1025), (0, 0)):
        assert lib.tn_dbg_encoder_plan(h, w, 0, 2, 0, *out) != 0, (h, w)
    assert lib.tn_dbg_encoder_plan(224, 1024, 0, 2, 0, *out) != 0          # too wide for the conv3x3 LDS tile
    assert lib.tn_dbg_encoder_plan(224, 224, 2, 2, 0, *out) != 0           # unknown flag
    assert lib.tn_dbg_encoder_plan(224, 224, 16, 2, 0, *out) != 0
    assert lib.tn_dbg_encoder_plan(224, 224, _lib.ENC_FP32, 2, 0, *out) != 0       # not planned
    assert lib.tn_dbg_encoder_plan(224, 224, _lib.ENC_FP32X3, 2, 0, *out) != 0
    assert lib.tn_dbg_encoder_plan(224, 224, 0, 0, 0, *out) != 0
    assert lib.tn_dbg_encoder_plan(224, 224, 0, 2, 0, None, 16, C.byref(n)) != 0
    assert lib.tn_dbg_encoder_plan(224, 224, 0, 2, 0, stats, 16, None) != 0


def test_exact_mode_refuses_the_switches_create_refuses(lib, monkeypatch):
    from tennis_amd import _lib
    stats = (_lib.TnKernelStat * 16)()
    n = C.c_int(0)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TN_NO_FUSE", "1")
    assert lib.tn_dbg_encoder_plan(224, 224, _lib.ENC_EXACT_WEIGHTS, 2, 0, stats, 16, C.byref(n)) != 0
    monkeypatch.delenv("TN_NO_FUSE")
    monkeypatch.setenv("TN_DL_VARIANT", "8")
    assert lib.tn_dbg_encoder_plan(224, 224, _lib.ENC_EXACT_WEIGHTS, 2, 0, stats, 16, C.byref(n)) != 0
    assert lib.tn_dbg_encoder_plan(224, 224, 0, 2, 0, stats, 16, C.byref(n)) == 0
