"""-m gpu: the strip layers of the 56x56 and 28x28 blocks as ONE launch per block vs one launch per layer.

Default: `dense_strip_kernel_chain<W>` walks the block's strip layers (K = 64 ... 192 at 56x56, K = 128 ... 288 at 28x28; K = 224 / K = 320 keep their own launches) inside
one launch, one workgroup per frame; TN_NO_STRIP_CHAIN=1 launches `dense_strip_kernel<W, KS>` once per layer.  The layer bodies
are the same code with the same static schedule, so the bar is bit equality - of the features and of the two concat buffers
(read_tap "stage1" / "stage2").  What the chained form could get wrong is ordering: a layer that reads channels its
predecessor has not finished storing, or a 128-byte line whose other half an earlier layer of the same launch pulled into the
CU's L1.  Such a fault is timing and history dependent, so every batch size runs twice on the same handle with different frames,
and the first call of a size follows calls of other sizes through the same buffers.  (Un-pipelined, a batch of 64 runs as two
halves of 32 = below strip_min_batch: the old route in both variants; 128 and 256 reach the strip kernels as 64 and 128 frames,
and the pipelined calls at the end as 256.)

The switch is read when the encoder is created; each variant runs in a fresh child process (this file, run as a script), so
neither shares a HIP context, an allocator state or a kernel cache with the other.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (256, 64, 128, 8)      # in the order the child runs them; 8 < strip_min_batch (64): the small-batch kernels, both variants
TAP_FRAMES = 8                   # frames of the concat buffers that are compared (the features cover every frame)
CHAIN_FAMILIES = ("dense_block_strip_56x56", "dense_block_strip_28x28")


def _weights():
    """Seeded DenseNet-121 parameters; one BatchNorm scale in eight negative (the clamp form of BN1 + ReLU then has its
    bounds the other way round, and BN2's folded scale flips the sign of a weight row)."""
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(5)
    rng = np.random.default_rng(11)
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
            g.manual_seed(1000 * rnd + b)
            x = torch.randn((b, 224, 224, 3), generator=g, device="cuda").half()
            res[f"feat_b{b}_r{rnd}"] = enc(x).cpu().numpy()
            n = min(b, TAP_FRAMES)
            res[f"stage1_b{b}_r{rnd}"] = enc.read_tap("stage1", n).copy()
            res[f"stage2_b{b}_r{rnd}"] = enc.read_tap("stage2", n).copy()
            # the instrumented pass: which kernel families ran, and its features (both rounds: it is the one call in which 64
            # frames reach the strip kernels in one launch, and the second call on a handle is the one that shows a stale line)
            stats, out = enc.profile(x)
            res[f"families_b{b}"] = np.frombuffer(json.dumps({s["name"]: s["launches"] for s in stats}).encode(), dtype=np.uint8)
            res[f"featprof_b{b}_r{rnd}"] = out.cpu().numpy()
    # the flagship form: pipelined calls, whole batches side by side on two streams in two workspace sets (the only form in which
    # 256 frames reach the dense layers in one launch: un-pipelined, a batch runs as two halves)
    enc.set_pipelined(True)
    xs, outs = [], []
    for i in range(4):
        g.manual_seed(5000 + i)
        xs.append(torch.randn((256, 224, 224, 3), generator=g, device="cuda").half())
        outs.append(enc(xs[-1], out=torch.empty((256, enc.feature_dim), dtype=torch.float32, device="cuda")))
        if i >= 1:
            enc.join(1)
    enc.join(0)
    torch.cuda.synchronize()
    enc.set_pipelined(False)
    res["feat_pipelined"] = torch.stack(outs).cpu().numpy()
    np.savez(out_path, **res)


def _run_child(out_path, no_chain):
    env = dict(os.environ)
    env.pop("TN_NO_STRIP_CHAIN", None)
    if no_chain:
        env["TN_NO_STRIP_CHAIN"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, cwd=ROOT, timeout=900,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child (TN_NO_STRIP_CHAIN={int(no_chain)}) failed with {r.returncode}:\n{r.stdout[-4000:]}"
    return dict(np.load(out_path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip_chain")
    chained = _run_child(str(d / "chained.npz"), False)
    per_layer = _run_child(str(d / "per_layer.npz"), True)
    return chained, per_layer


def _families(run, b):
    return json.loads(bytes(run[f"families_b{b}"]).decode())


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_chained_strip_layers_match_per_layer_launches(runs, batch):
    chained, per_layer = runs
    for rnd in (0, 1):
        for what in ("feat", "stage1", "stage2"):
            key = f"{what}_b{batch}_r{rnd}"
            a, b = chained[key], per_layer[key]
            assert np.isfinite(a).all() and a.shape == b.shape, key
            ndiff = int((a != b).sum())
            assert ndiff == 0, f"{key}: {ndiff} of {a.size} values differ, max |d| {float(np.abs(a - b).max())}"
    # the two calls of a size saw different frames (a stale buffer would not)
    assert not np.array_equal(chained[f"feat_b{batch}_r0"], chained[f"feat_b{batch}_r1"])
    # the instrumented pass (never split into half batches: 64 frames reach the strip kernels in one launch there) too
    for rnd in (0, 1):
        assert np.array_equal(chained[f"featprof_b{batch}_r{rnd}"], per_layer[f"featprof_b{batch}_r{rnd}"]), rnd
    assert not np.array_equal(chained[f"featprof_b{batch}_r0"], chained[f"featprof_b{batch}_r1"])


def test_pipelined_whole_batches_match(runs):
    chained, per_layer = runs
    a, b = chained["feat_pipelined"], per_layer["feat_pipelined"]
    assert np.isfinite(a).all() and a.shape == b.shape and a.shape[:2] == (4, 256)
    ndiff = int((a != b).sum())
    assert ndiff == 0, f"pipelined: {ndiff} of {a.size} values differ, max |d| {float(np.abs(a - b).max())}"
    assert not np.array_equal(a[0], a[1])


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_which_route_ran(runs, batch):
    """The comparison above is between two different routes exactly where it should be: from strip_min_batch frames on the
    default encoder reports the chained families next to the per-layer ones (one strip layer per map keeps its own launch), with
    fewer per-layer launches than under TN_NO_STRIP_CHAIN; there, and below strip_min_batch in both, nothing chained runs."""
    chained, per_layer = runs
    lc, lp = _families(chained, batch), _families(per_layer, batch)        # family -> launches
    fc, fp = sorted(lc), sorted(lp)
    assert not set(fp) & set(CHAIN_FAMILIES), fp
    if batch >= 64:
        assert set(CHAIN_FAMILIES) <= set(fc), fc
        for w, nl_all, nl_chained in ((56, 6, 5), (28, 7, 6)):
            assert lc[f"dense_block_strip_{w}x{w}"] == 1
            assert lp[f"dense_layer_strip_{w}x{w}"] == nl_all and lc[f"dense_layer_strip_{w}x{w}"] == nl_all - nl_chained
    else:
        assert not set(fc) & set(CHAIN_FAMILIES), fc
        assert lc == lp


if __name__ == "__main__":
    _child(sys.argv[1])
