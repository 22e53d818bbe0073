"""-m "not gpu": where a forward folds the head (BatchNorm + ReLU + 7x7 average) into the last transition and the 7x7 block kernel
(csrc/encoder_plan.h::enc_head_fused), asked through tn_dbg_head_fused, which touches no device.

The route exists where both producers of the last block's map are the one-workgroup-per-frame kernels that hold a frame's un-rounded
values in registers: the warp-specialised transition's 64 x 512 tile on a 14 x 14 map (csrc/trans_ws.hip) and the LDS-resident 7x7
block (csrc/dense_block7.hip), with one 7 x 7 pooling window.  It does not depend on the batch.  Calibration (layer-wise kernels),
tn_densenet121_forward_class_maps (the maps are made from the fp32 side copy) and the instrumented pass keep the side copy and the
head launch, so what tn_dbg_encoder_plan reports - the head family included - is what it was: the golden table's rows."""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_routes.json")
SWITCHES = ("TN_NO_FUSE", "TN_NO_CHAIN", "TN_NO_CHAIN28", "TN_CHAIN28_MIN_BATCH", "TN_NO_BLOCK7", "TN_NO_BLOCK14", "TN_BLOCK28", "TN_NO_STRIP",
            "TN_NO_STRIP_CHAIN", "TN_DL_VARIANT", "TN_STRIP_MIN_BATCH", "TN_NO_STRIP_PAIR", "TN_STRIP_PAIR_MIN_BATCH", "TN_NO_HEAD_FUSE",
            "TN_NO_TRANS_WS")


@pytest.fixture(scope="module")
def lib():
    from tennis_amd import _lib
    return _lib.load()


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def fused(lib, monkeypatch, size=224, flags=0, batch=256, calibrate=0, class_maps=0, env=None, width=None):
    _env(monkeypatch, env)
    out = C.c_int(-1)
    rc = lib.tn_dbg_head_fused(size, width or size, flags, batch, calibrate, class_maps, C.byref(out))
    assert rc == 0, (rc, lib.tn_last_error())
    assert out.value in (0, 1)
    return out.value


@pytest.mark.parametrize("batch", [1, 3, 8, 31, 32, 64, 128, 255, 256, 257, 512])
def test_the_default_route_at_224_whatever_the_batch(lib, monkeypatch, batch):
    assert fused(lib, monkeypatch, batch=batch) == 1


@pytest.mark.parametrize("size,want", [(224, 1), (225, 1), (236, 1), (237, 0), (256, 0), (448, 0), (512, 0), (960, 0)])
def test_sizes(lib, monkeypatch, size, want):
    """the last map is 7 x 7 behind a 14 x 14 one up to 236 pixels a side (237: a 15 x 15 map in front of it, which the
    warp-specialised transition does not take); 448: 14 x 14 (the streamed kernel's block); 512: 16 x 16, a 2 x 2 window"""
    assert fused(lib, monkeypatch, size=size) == want
    assert fused(lib, monkeypatch, size=224, width=size) == want


@pytest.mark.parametrize("env", [{"TN_NO_HEAD_FUSE": "1"}, {"TN_NO_BLOCK7": "1"}, {"TN_NO_FUSE": "1"}, {"TN_DL_VARIANT": "8"}, {"TN_NO_TRANS_WS": "1"}],
                         ids=lambda e: next(iter(e)))
def test_switches_that_take_a_producer_away(lib, monkeypatch, env):
    assert fused(lib, monkeypatch, env=env) == 0
    assert fused(lib, monkeypatch) == 1


@pytest.mark.parametrize("env", [{"TN_NO_STRIP_PAIR": "1"}, {"TN_NO_STRIP": "1"}, {"TN_NO_CHAIN": "1"}, {"TN_NO_BLOCK14": "1"}, {"TN_STRIP_MIN_BATCH": "32"},
                                 {"TN_BLOCK28": "1"}], ids=lambda e: next(iter(e)))
def test_switches_of_the_other_blocks_leave_it(lib, monkeypatch, env):
    assert fused(lib, monkeypatch, env=env) == 1


def test_modes_and_passes(lib, monkeypatch):
    from tennis_amd import _lib
    assert fused(lib, monkeypatch, flags=_lib.ENC_EXACT_WEIGHTS) == 0
    assert fused(lib, monkeypatch, flags=_lib.ENC_FP32) == 0
    assert fused(lib, monkeypatch, flags=_lib.ENC_FP32X3) == 0
    assert fused(lib, monkeypatch, flags=_lib.ENC_FP32 | _lib.ENC_EXACT_WEIGHTS) == 0
    assert fused(lib, monkeypatch, calibrate=1) == 0
    assert fused(lib, monkeypatch, class_maps=1) == 0
    assert fused(lib, monkeypatch, calibrate=1, class_maps=1) == 0
    assert fused(lib, monkeypatch) == 1


def test_refusals(lib, monkeypatch):
    _env(monkeypatch, None)
    out = C.c_int(-1)
    assert lib.tn_dbg_head_fused(224, 224, 0, 8, 0, 0, None) != 0
    assert lib.tn_dbg_head_fused(223, 224, 0, 8, 0, 0, C.byref(out)) != 0
    assert lib.tn_dbg_head_fused(224, 224, 0, 0, 0, 0, C.byref(out)) != 0
    assert lib.tn_dbg_head_fused(224, 224, 1 << 20, 8, 0, 0, C.byref(out)) != 0
    assert out.value == -1


def test_the_plan_reports_what_the_golden_table_holds(lib, monkeypatch):
    """the instrumented pass and tn_dbg_encoder_plan keep the head family: one launch per forward, the same flops and bytes"""
    from tennis_amd import _lib
    with open(FIXTURE) as f:
        entries = json.load(f)
    assert len(entries) >= 30
    on = 0
    for e in entries:
        _env(monkeypatch, e["env"])
        stats = (_lib.TnKernelStat * 16)()
        n = C.c_int(0)
        rc = lib.tn_dbg_encoder_plan(e["size"], e["size"], e["flags"], e["batch"], e.get("calibrate", 0), stats, 16, C.byref(n))
        assert rc == 0, (rc, lib.tn_last_error(), e)
        rows = [[stats[i].name.decode(), stats[i].launches, stats[i].flops, stats[i].bytes] for i in range(n.value)]
        assert rows == e["families"], e
        assert rows[-1][0] == "head_bnrelu_avgpool7" and rows[-1][1] == 1, e
        on += fused(lib, monkeypatch, size=e["size"], flags=e["flags"], batch=e["batch"], env=e["env"])
    assert 0 < on < len(entries)
