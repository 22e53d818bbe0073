"""-m "not gpu": which steps of the routing plan take the paired launch geometry of the 28x28 strip kernels (csrc/encoder_plan.h:
enc_strip_pair, EncStep::paired), asked through tn_dbg_encoder_plan_shared, which touches no device.

The paired launch (csrc/dense_strip_pair_w28.hip: two frames per workgroup, B / 2 workgroups) is for a call whose kernels share the
chip with a neighbouring stream's call - the pipelined whole-batch form of encoder_run and nothing else; tn_dbg_encoder_plan answers
for every other caller (the un-split call, the instrumented pass, the half batches) and tn_dbg_encoder_plan_shared for that one.  It is
a flag on a step, not a route: at 224 x 224 the chained strip launch (K = 128 ... 288) and the K = 320 strip launch of the second
block carry it from strip_pair_min_batch (256) frames on when the batch is even, and the families, launches, flops and bytes of
the plan are tn_dbg_encoder_plan's whatever the flag says."""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_routes.json")
SWITCHES = ("TN_NO_FUSE", "TN_NO_CHAIN", "TN_NO_CHAIN28", "TN_CHAIN28_MIN_BATCH", "TN_NO_BLOCK7", "TN_NO_BLOCK14", "TN_BLOCK28", "TN_NO_STRIP",
            "TN_NO_STRIP_CHAIN", "TN_DL_VARIANT", "TN_STRIP_MIN_BATCH", "TN_NO_STRIP_PAIR", "TN_STRIP_PAIR_MIN_BATCH")


@pytest.fixture(scope="module")
def lib():
    from tennis_amd import _lib
    return _lib.load()


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def shared(lib, monkeypatch, batch, env=None, flags=0, size=224):
    """(rows, paired) of tn_dbg_encoder_plan_shared under the TN_* environment `env`"""
    from tennis_amd import _lib
    _env(monkeypatch, env)
    stats = (_lib.TnKernelStat * 16)()
    n, paired = C.c_int(0), C.c_int(-1)
    rc = lib.tn_dbg_encoder_plan_shared(size, size, flags, batch, stats, 16, C.byref(n), C.byref(paired))
    assert rc == 0, (rc, lib.tn_last_error())
    return [[stats[i].name.decode(), stats[i].launches, stats[i].flops, stats[i].bytes] for i in range(n.value)], paired.value


def alone(lib, monkeypatch, batch, env=None, flags=0, size=224):
    from tennis_amd import _lib
    _env(monkeypatch, env)
    stats = (_lib.TnKernelStat * 16)()
    n = C.c_int(0)
    rc = lib.tn_dbg_encoder_plan(size, size, flags, batch, 0, stats, 16, C.byref(n))
    assert rc == 0, (rc, lib.tn_last_error())
    return [[stats[i].name.decode(), stats[i].launches, stats[i].flops, stats[i].bytes] for i in range(n.value)]


@pytest.mark.parametrize("batch,want", [(254, 0), (255, 0), (256, 2), (258, 2), (257, 0), (512, 2)])
def test_threshold_and_parity_of_the_batch(lib, monkeypatch, batch, want):
    """from 256 frames on, an even batch: one paired step for the chain (K = 128 ... 288) and one for K = 320"""
    rows, paired = shared(lib, monkeypatch, batch)
    assert paired == want
    fams = {r[0]: r[1] for r in rows}
    assert fams["dense_block_strip_28x28"] == 1 and fams["dense_layer_strip_28x28"] == 1


def test_an_odd_batch_is_refused_whatever_the_threshold(lib, monkeypatch):
    assert shared(lib, monkeypatch, 255, {"TN_STRIP_PAIR_MIN_BATCH": "2"})[1] == 0
    assert shared(lib, monkeypatch, 3, {"TN_STRIP_PAIR_MIN_BATCH": "2", "TN_STRIP_MIN_BATCH": "1"})[1] == 0
    assert shared(lib, monkeypatch, 254, {"TN_STRIP_PAIR_MIN_BATCH": "2"})[1] == 2
    # the threshold moves with its own switch only; below strip_min_batch there is no strip step to pair
    assert shared(lib, monkeypatch, 64, {"TN_STRIP_PAIR_MIN_BATCH": "64"})[1] == 2
    assert shared(lib, monkeypatch, 62, {"TN_STRIP_PAIR_MIN_BATCH": "64"})[1] == 0
    assert shared(lib, monkeypatch, 32, {"TN_STRIP_PAIR_MIN_BATCH": "2"})[1] == 0
    assert shared(lib, monkeypatch, 32, {"TN_STRIP_PAIR_MIN_BATCH": "2", "TN_STRIP_MIN_BATCH": "32"})[1] == 2


@pytest.mark.parametrize("env,flags,size,want", [
    ({"TN_NO_STRIP_PAIR": "1"}, 0, 224, 0),
    ({"TN_NO_STRIP": "1"}, 0, 224, 0),                 # no strip step at all
    ({"TN_NO_STRIP_CHAIN": "1"}, 0, 224, 7),           # seven per-layer strip steps at 28x28, K = 128 ... 320, each paired
    ({"TN_DL_VARIANT": "8"}, 0, 224, 0),               # a tuning variant keeps the block on the tile kernels
    ({}, "exact", 224, 0),                             # exact weights: no strip route
    ({}, 0, 512, 0),                                   # 128x128 / 64x64 / 32x32 / 16x16 maps: no 28x28 block
    ({}, 0, 448, 3),                                   # the 28x28 block of a 448x448 input starts at K = 256: per-layer strip steps K = 256, 288, 320
], ids=["no_strip_pair", "no_strip", "no_strip_chain", "variant8", "exact", "512", "448"])
def test_every_switch_gives_the_count_its_rule_implies(lib, monkeypatch, env, flags, size, want):
    from tennis_amd import _lib
    f = _lib.ENC_EXACT_WEIGHTS if flags == "exact" else 0
    rows, paired = shared(lib, monkeypatch, 256, env, f, size)
    assert paired == want
    # the flag changes nothing a profile reports
    assert rows == alone(lib, monkeypatch, 256, env, f, size)


def test_families_launches_flops_and_bytes_are_the_unshared_plan_s(lib, monkeypatch):
    with open(FIXTURE) as f:
        entries = json.load(f)
    assert len(entries) >= 30
    for e in entries:
        rows, paired = shared(lib, monkeypatch, e["batch"], e["env"], e["flags"], e["size"])
        assert rows == e["families"], e
        assert rows == alone(lib, monkeypatch, e["batch"], e["env"], e["flags"], e["size"]), e
        assert paired == 0, e          # (batches up to 64: below the threshold)
    for batch in (254, 256, 257, 512):
        assert shared(lib, monkeypatch, batch)[0] == alone(lib, monkeypatch, batch)
    # the same table with the threshold out of the way: the even batches of the table with a 28x28 strip step carry the flag, and
    # the rows stay what they were
    seen = 0
    for e in entries:
        env = dict(e["env"], TN_STRIP_PAIR_MIN_BATCH="2")
        rows, paired = shared(lib, monkeypatch, e["batch"], env, e["flags"], e["size"])
        assert rows == e["families"], e
        n28 = sum(r[1] for r in rows if r[0] in ("dense_block_strip_28x28", "dense_layer_strip_28x28"))
        assert paired == (n28 if e["batch"] % 2 == 0 else 0), e
        seen += paired
    assert seen > 0
