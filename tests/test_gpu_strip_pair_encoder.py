"""-m gpu: the encoder with the paired 28x28 strip launches (default) against TN_NO_STRIP_PAIR=1, each in a fresh child process.

A pipelined whole-batch call runs beside the neighbouring stream's call; there, from strip_pair_min_batch frames on, the chained
strip launch of the 28x28 block (K = 128 ... 288) and its K = 320 launch take two frames per workgroup
(csrc/dense_strip_pair_w28.hip, csrc/encoder_plan.h::enc_strip_pair).  Same arithmetic in the same order per output: features and
the 28x28 concat buffer (read_tap "stage2") must be bit-identical between the two processes.  Which launch ran is not visible in a
profile - the instrumented pass never shares the chip, so it never takes the route - but in tn_dbg_strip_pair_launches: four
pipelined 64-frame calls are 8 paired launches in the first process and 0 in the second.  On the same handle a non-pipelined call
(two half batches) and an instrumented pass follow: the counter must not move, and their features are the pipelined call's on the
same frames.

Small on purpose: max_batch 64 with TN_STRIP_MIN_BATCH=32 and TN_STRIP_PAIR_MIN_BATCH=64 reaches every branch the flagship
batch of 256 does (32 workgroups per paired launch).  The switches are read when the encoder is created; each variant runs this
file as a script."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, CALLS, TAP_FRAMES = 64, 4, 16


def _weights():
    """Seeded DenseNet-121 parameters; one BatchNorm scale in eight negative"""
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(7)
    rng = np.random.default_rng(13)
    for k in sorted(p):
        if k.endswith("_gamma"):
            g = p[k].copy()
            g[rng.random(g.shape[0]) < 0.125] *= -1.0
            p[k] = g
    return p


def _child(out_path):
    import torch
    sys.path.insert(0, ROOT)
    from tennis_amd import _lib
    from tennis_amd.engine import DenseNet121Features

    def launches():
        n = C.c_int64(-1)
        _lib.check(_lib.load().tn_dbg_strip_pair_launches(C.byref(n)), "tn_dbg_strip_pair_launches")
        return n.value

    enc = DenseNet121Features(_weights(), 224, max_batch=B)
    g = torch.Generator(device="cuda")
    res = {"launches_start": launches()}
    enc.set_pipelined(True)
    xs, outs = [], []
    for i in range(CALLS):
        g.manual_seed(7000 + i)
        xs.append(torch.randn((B, 224, 224, 3), generator=g, device="cuda").half())
        outs.append(enc(xs[-1], out=torch.empty((B, enc.feature_dim), dtype=torch.float32, device="cuda")))
        if i >= 1:
            enc.join(1)
    enc.join(0)
    torch.cuda.synchronize()
    res["feat_pipelined"] = torch.stack(outs).cpu().numpy()
    res["stage2"] = enc.read_tap("stage2", TAP_FRAMES).astype(np.float16)          # (the buffer holds fp16 numbers: lossless)
    res["launches_pipelined"] = launches()
    enc.set_pipelined(False)
    res["feat_plain"] = enc(xs[-1]).cpu().numpy()                                  # two half batches of 32
    torch.cuda.synchronize()
    res["launches_plain"] = launches()
    stats, out = enc.profile(xs[-1])                                               # the instrumented pass: one un-split batch
    res["feat_profile"] = out.cpu().numpy()
    res["launches_profile"] = launches()
    res["strip28_launches"] = sum(s["launches"] for s in stats if s["name"] in ("dense_block_strip_28x28", "dense_layer_strip_28x28"))
    np.savez(out_path, **res)


def _run_child(out_path, no_pair):
    env = dict(os.environ)
    for k in ("TN_NO_STRIP_PAIR", "TN_NO_STRIP", "TN_NO_STRIP_CHAIN", "TN_NO_INTERLEAVE", "TN_NO_SPLIT", "TN_SPLIT", "TN_DL_VARIANT"):
        env.pop(k, None)
    env.update(TN_STRIP_MIN_BATCH="32", TN_STRIP_PAIR_MIN_BATCH="64")
    if no_pair:
        env["TN_NO_STRIP_PAIR"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, cwd=ROOT, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child (TN_NO_STRIP_PAIR={int(no_pair)}) failed with {r.returncode}:\n{r.stdout[-4000:]}"
    return dict(np.load(out_path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip_pair")
    paired = _run_child(str(d / "paired.npz"), False)
    plain = _run_child(str(d / "plain.npz"), True)
    return paired, plain


def test_features_and_the_28x28_buffer_are_bit_identical(runs):
    paired, plain = runs
    for key in ("feat_pipelined", "stage2", "feat_plain", "feat_profile"):
        a, b = paired[key], plain[key]
        assert a.shape == b.shape and np.isfinite(a.astype(np.float32)).all(), key
        ndiff = int((a.view(np.uint16 if a.dtype == np.float16 else np.uint32) != b.view(np.uint16 if b.dtype == np.float16 else np.uint32)).sum())
        assert ndiff == 0, f"{key}: {ndiff} of {a.size} values differ"
    a = paired["feat_pipelined"]
    assert a.shape[:2] == (CALLS, B)
    for i in range(1, CALLS):
        assert not np.array_equal(a[i], a[0])               # the calls saw different frames
    assert np.abs(paired["stage2"].astype(np.float32)).max() > 0


def test_the_paired_route_ran_where_it_should_and_nowhere_else(runs):
    paired, plain = runs
    assert int(paired["launches_start"]) == 0 and int(plain["launches_start"]) == 0
    assert int(paired["launches_pipelined"]) == 2 * CALLS    # per call: the chain (K = 128 ... 288) and K = 320
    assert int(plain["launches_pipelined"]) == 0
    # the non-pipelined call and the instrumented pass: the counter does not move
    for run in (paired, plain):
        assert int(run["launches_plain"]) == int(run["launches_pipelined"])
        assert int(run["launches_profile"]) == int(run["launches_pipelined"])
        assert int(run["strip28_launches"]) == 2             # they do run the strip steps, one frame per workgroup


def test_other_forms_of_the_call_give_the_pipelined_features(runs):
    for run in runs:
        last = run["feat_pipelined"][CALLS - 1]
        assert np.array_equal(run["feat_plain"].view(np.uint32), last.view(np.uint32))
        assert np.array_equal(run["feat_profile"].view(np.uint32), last.view(np.uint32))


if __name__ == "__main__":
    _child(sys.argv[1])
