"""-m gpu: the tile-kernel layers of the 28x28 block (K = 352 ... 480) as ONE chained launch vs one launch per layer, in the encoder.

Default: from chain28_min_batch (128) frames per call on, `dense_layer_kernel<28, 14, 512, 32, 2, true>` walks the five layers of a frame
inside one launch, one workgroup per frame; TN_NO_CHAIN28=1 launches the per-layer kernel five times.  The arithmetic of a tile is the
same code, so the bar is bit equality - of the features and of the block's concat buffer (read_tap "stage2").  What the chained form could
get wrong is ordering at the seam between a frame's two row tiles (tests/test_gpu_chain28_kernel.py holds the kernel to it on its own);
such a fault is timing and history dependent, so every batch size runs twice on the same handle with different frames, and the first call
of a size follows calls of other sizes through the same buffers.

Which calls reach the chained launch: un-pipelined, a batch runs as two halves - 256 frames reach the dense layers as 128 (chained),
128 as 64 and 64 as 32 (per layer in both variants); the instrumented pass is never split (128 and 256 frames in one chained launch,
64 frames in five per-layer launches in both variants); the pipelined calls at the end run whole batches of 256.

The switch is read when the encoder is created; each variant runs in a fresh child process (this file, run as a script), so neither
shares a HIP context, an allocator state or a kernel cache with the other."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (256, 64, 128)         # in the order the child runs them
TAP_FRAMES = 8                   # frames of the concat buffer that are compared (the features cover every frame)
FUSED, CHAINED = "dense_layer_fused_28x28", "dense_block_chained_28x28"


def _weights():
    """Seeded DenseNet-121 parameters; one BatchNorm scale in eight negative (the clamp form of BN1 + ReLU then has its bounds the other
    way round, and BN2's scale flips a bottleneck channel's sign)."""
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
    from tennis_amd.engine import DenseNet121Features
    enc = DenseNet121Features(_weights(), 224, max_batch=max(BATCHES))
    g = torch.Generator(device="cuda")
    res = {}
    for rnd in (0, 1):
        for b in BATCHES:
            g.manual_seed(2000 * rnd + b)
            x = torch.randn((b, 224, 224, 3), generator=g, device="cuda").half()
            res[f"feat_b{b}_r{rnd}"] = enc(x).cpu().numpy()
            res[f"stage2_b{b}_r{rnd}"] = enc.read_tap("stage2", TAP_FRAMES).copy()
            # the instrumented pass: the whole batch in one call (128 frames reach the chained launch only here), the families it
            # launched, its features and its concat buffer
            stats, out = enc.profile(x)
            res[f"families_b{b}"] = np.frombuffer(json.dumps({s["name"]: s["launches"] for s in stats}).encode(), dtype=np.uint8)
            res[f"featprof_b{b}_r{rnd}"] = out.cpu().numpy()
            res[f"stage2prof_b{b}_r{rnd}"] = enc.read_tap("stage2", TAP_FRAMES).copy()
    # the flagship form: pipelined calls, whole batches of 256 side by side on two streams in two workspace sets
    enc.set_pipelined(True)
    outs = []
    for i in range(4):
        g.manual_seed(7000 + i)
        x = torch.randn((256, 224, 224, 3), generator=g, device="cuda").half()
        outs.append(enc(x, out=torch.empty((256, enc.feature_dim), dtype=torch.float32, device="cuda")))
        if i >= 1:
            enc.join(1)
    enc.join(0)
    torch.cuda.synchronize()
    enc.set_pipelined(False)
    res["feat_pipelined"] = torch.stack(outs).cpu().numpy()
    np.savez(out_path, **res)


def _run_child(out_path, per_layer):
    env = dict(os.environ)
    for k in ("TN_NO_CHAIN28", "TN_NO_CHAIN", "TN_CHAIN28_MIN_BATCH"):
        env.pop(k, None)
    if per_layer:
        env["TN_NO_CHAIN28"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, cwd=ROOT, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child (TN_NO_CHAIN28={int(per_layer)}) failed with {r.returncode}:\n{r.stdout[-4000:]}"
    return dict(np.load(out_path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain28")
    chained = _run_child(str(d / "chained.npz"), False)
    per_layer = _run_child(str(d / "per_layer.npz"), True)
    return chained, per_layer


def _families(run, b):
    return json.loads(bytes(run[f"families_b{b}"]).decode())


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_chained_tile_layers_match_per_layer_launches(runs, batch):
    chained, per_layer = runs
    for rnd in (0, 1):
        for what in ("feat", "stage2", "featprof", "stage2prof"):
            key = f"{what}_b{batch}_r{rnd}"
            a, b = chained[key], per_layer[key]
            assert np.isfinite(a).all() and a.shape == b.shape, key
            ndiff = int((a != b).sum())
            assert ndiff == 0, f"{key}: {ndiff} of {a.size} values differ, max |d| {float(np.abs(a - b).max())}"
    # the two calls of a size saw different frames (a stale buffer would not)
    assert not np.array_equal(chained[f"feat_b{batch}_r0"], chained[f"feat_b{batch}_r1"])
    assert not np.array_equal(chained[f"stage2prof_b{batch}_r0"], chained[f"stage2prof_b{batch}_r1"])


def test_pipelined_whole_batches_match(runs):
    chained, per_layer = runs
    a, b = chained["feat_pipelined"], per_layer["feat_pipelined"]
    assert np.isfinite(a).all() and a.shape == b.shape and a.shape[:2] == (4, 256)
    ndiff = int((a != b).sum())
    assert ndiff == 0, f"pipelined: {ndiff} of {a.size} values differ, max |d| {float(np.abs(a - b).max())}"
    assert not np.array_equal(a[0], a[1])


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_which_route_ran(runs, batch):
    """From 128 frames on the default encoder reports one chained launch where TN_NO_CHAIN28 reports five per-layer ones; at 64 frames
    both report the five; the strip routes in front of them are the same in both."""
    chained, per_layer = runs
    lc, lp = _families(chained, batch), _families(per_layer, batch)        # family -> launches
    assert CHAINED not in lp and lp[FUSED] == 5
    if batch >= 128:
        assert lc.get(CHAINED) == 1 and FUSED not in lc, lc
        rest = {k: v for k, v in lc.items() if k != CHAINED}
        assert rest == {k: v for k, v in lp.items() if k != FUSED}
    else:
        assert lc == lp
    for run in (lc, lp):
        assert run["dense_block_strip_28x28"] == 1 and run["dense_layer_strip_28x28"] == 1
        assert run["dense_block_strip_56x56"] == 1 and run["dense_layer_strip_56x56"] == 1
        assert run["dense_block_stream_14x14"] == 1 and run["dense_block_lds_7x7"] == 1


if __name__ == "__main__":
    _child(sys.argv[1])
