"""-m gpu: the calibration statistics of the calibrated fp16 conversion (tn_densenet121_input_means) against an fp64 oracle.

The one GPU input of ``calibrate.py`` -> ``weights.as_fp16_model(params, input_means=...)`` is the per-channel mean operand of the
119 convolutions behind the stem.  The feature error after the whole conversion hardly moves when those numbers are wrong (a wrong
mean moves a few weights to their other fp16 neighbour), so they are pinned here on their own:
  * the reduction kernel (pool.hip launch_channel_mean, through the tn_dbg_channel_mean hook) against a float64 mean of the same
    fp16 values, at ragged row counts, K not a multiple of 64, ld > K, degenerate clamps and negative scales;
  * input_means end to end against tests/tools/operand_means.py (the reference graph in float64 on the same parameters), in the
    units include/tennis_hip.h defines, on three parameter sets - (a) seeded, (b) (a) with stem channels centred at m_c = 1.0 and
    degenerate / negative-scale clamps planted in a block-1 consumer, (c) trained-looking (tests/tools/trained_like.py) - at
    224x224 (one frame and three), 236x236 (odd maps: a transition's dropped row / column still counts) and 512x512;
  * the encoder's state around the call: input_means after pipelined forwards in either workspace set, read_tap after it, and
    the next pipelined forward.
Measured worst errors go to the session report (the `report` fixture of tests/conftest.py)."""
import numpy as np
import pytest
import torch

from tools import operand_means as OM

pytestmark = pytest.mark.gpu

PRE = "densenet0_"

# Per conv kind, the worst over its convolutions and channels of |library - oracle| / max(1, |oracle|), less the threshold slack of
# block 1's centred clamps (_centred_threshold_slack): an absolute error for means up to 1.  What is left is the fp16 storage of the
# activations, averaged over a frame - except where it is not averaged out (flat regions round the same way in every pixel) and where
# the trained-looking parameters amplify it through 120 layers.  Measured on MI355X (first run, worst of 224 x 1, 224 x 3, 236, 512):
#   sets (a) seeded and (b) degenerate:  dense 1x1 3.0e-4, dense 3x3 2.8e-4, transition 1.6e-4
#   set (c) trained-looking:             dense 1x1 5.3e-3, dense 3x3 5.8e-3, transition 5.4e-3
# The bars are about 3x that; all of them are at least 5x below 0.1, a tenth of the m_c = 1.0 the add-back used to put into the
# degenerate channels of set (b).
BARS = {"seeded": {"dense1x1": 1e-3, "dense3x3": 1e-3, "trans": 5e-4},
        "trained_like": {"dense1x1": 1.6e-2, "dense3x3": 1.8e-2, "trans": 1.6e-2}}
KINDS = ("dense1x1", "dense3x3", "trans")


def _lib():
    from tennis_amd import _lib
    return _lib


# ---- the reduction kernel on its own ---------------------------------------------------------------------------------------------

def _channel_mean_ref(x16, K, a, b, clamp):
    """float64 mean over rows of clamp(x, a, b), or of relu(fp32(fma(x, a, b))) - the kernel's single rounding per element"""
    acc = np.zeros(K)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for r0 in range(0, x16.shape[0], 1 << 16):
        x = x16[r0:r0 + (1 << 16), :K].astype(np.float64)
        if clamp:
            v = np.minimum(np.maximum(x, a64), b64)
        else:
            v = np.maximum((x * a64 + b64).astype(np.float32), np.float32(0)).astype(np.float64)    # x * a exact in double
        acc += v.sum(0)
    return acc / x16.shape[0]


ROWS = (1, 3, 31, 33, 127, 129, 32 * 4 + 1, 32 * 32 + 1, 256 * 56 * 56)


@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("K", [32, 96, 160, 1024])
@pytest.mark.parametrize("rows", ROWS)
def test_channel_mean_kernel_against_fp64(rows, K, clamp):
    if rows > 4096 and K > 96:
        pytest.skip("the full-size map at 32 and 96 channels covers the long reduction")
    import ctypes as C
    L = _lib()
    ctx = L.default_context()
    rng = np.random.default_rng([rows, K, clamp])
    ld = K + 8 + rows % 3                                     # ld > K, and not always a multiple of 8
    x = rng.normal(0.0, 1.5, (rows, ld)).astype(np.float16)
    x[rng.integers(0, rows, 4), rng.integers(0, K, 4)] = np.array([-6e4, -900.0, 3e4, 65504.0], np.float16)
    if clamp:
        thr = rng.normal(0.0, 1.0, K).astype(np.float16).astype(np.float32)
        up = rng.random(K) < 0.5
        a = np.where(up, thr, np.float32(-65504)).astype(np.float32)          # lo
        b = np.where(up, np.float32(65504), thr).astype(np.float32)           # hi
        a[0], b[0] = 0.0, 0.0                                                  # a constant channel: the operand is 0
        a[1], b[1] = -65504.0, 0.3125                                          # open below
        a[2], b[2] = -0.25, 65504.0                                            # open above
        a[3], b[3] = -65504.0, 65504.0                                         # the clamp does nothing
    else:
        a = (rng.uniform(0.1, 2.0, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32)   # scale, negative in about half the channels
        b = rng.normal(0.0, 1.0, K).astype(np.float32)                                      # shift
        a[0], b[0] = -0.75, 0.5                                                # a negative-scale channel
        a[1], b[1] = 0.0, 0.625                                                # scale 0: the constant relu(shift)
        a[2], b[2] = 3e-5, -1.0                                                # tiny scale: ReLU'd to 0 unless x is huge
    xd = torch.from_numpy(x).cuda()
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    scratch = torch.empty(32 * K, dtype=torch.float64, device="cuda")
    outs = []
    for _ in range(2):
        out = torch.full((K,), float("nan"), dtype=torch.float32, device="cuda")
        L.check(ctx.lib.tn_dbg_channel_mean(ctx.handle, L.ptr(xd), ld, K, L.ptr(ad), L.ptr(bd), rows, L.ptr(scratch),
                                            C.c_size_t(scratch.numel() * 8), L.ptr(out), clamp), "tn_dbg_channel_mean")
        outs.append(out.cpu().numpy())
    got = outs[0].astype(np.float64)
    ref = _channel_mean_ref(x, K, a, b, clamp)
    err = np.abs(got - ref)
    assert (err <= 1e-6 * np.abs(ref) + 1e-7).all(), (int(err.argmax()), float(err.max()), got[err.argmax()], ref[err.argmax()])
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))     # the reduction order is fixed
    if clamp:
        assert got[0] == 0.0


def test_channel_mean_hook_refuses_a_short_scratch():
    import ctypes as C
    L = _lib()
    ctx = L.default_context()
    x = torch.zeros((4, 40), dtype=torch.float16, device="cuda")
    s = torch.ones(40, device="cuda")
    scratch = torch.empty(32 * 40, dtype=torch.float64, device="cuda")
    out = torch.empty(40, device="cuda")
    rc = ctx.lib.tn_dbg_channel_mean(ctx.handle, L.ptr(x), 40, 40, L.ptr(s), L.ptr(s), 4, L.ptr(scratch), C.c_size_t(8 * 32 * 40 - 8),
                                     L.ptr(out), 0)
    assert rc != 0 and b"scratch" in ctx.lib.tn_last_error()
    assert ctx.lib.tn_dbg_channel_mean(ctx.handle, L.ptr(x), 39, 40, L.ptr(s), L.ptr(s), 4, L.ptr(scratch), C.c_size_t(8 * 32 * 40),
                                       L.ptr(out), 0) != 0          # ld < K


# ---- input_means end to end ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def param_sets():
    import warnings
    from tools.trained_like import make_trained_like_weights
    from tennis_amd import weights as W
    a = W.make_densenet121_weights(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # (near-dead channels flush a few folded weights: expected here)
        c = W.as_fp16_model(make_trained_like_weights(0))       # plain conversion, as calibrate.frame_means does
    return {"a_seeded": a, "b_degenerate": OM.with_degenerate_channels(a), "c_trained_like": c}


def _frames(size, n):
    from tennis_amd import calib_frames as CF
    return np.ascontiguousarray(np.concatenate([CF.frames(f, 1, size, seed=17) for f in ("scene", "halfblack", "noise")[:n]]))


def _kinds():
    from tennis_amd import weights as W
    convs, _, _ = W.densenet121_layout()
    return {PRE + c["name"] + "_weight": (c["kind"], PRE + c["bn"]) for c in convs if c["kind"] != "stem"}


def _centred_threshold_slack(q):
    """{block-1 1x1 weight name: (cin,) float64}: how far the library's clamp thresholds of stem channels 0 .. 63 may sit from the
    oracle's.  The library stores the pooled stem map centred, x - m_c (m_c: the average running_mean of the channel's seven
    consumers, csrc/encoder.hip), and folds each consumer's BatchNorm on the centred map - its threshold is fp16(c - m_c) + m_c where
    the header's clamp has fp16(c).  A mean of a clamp moves by at most the move of its threshold: up to an fp16 ulp of c, which
    is 2 for a near-dead channel clipped at c ~ 3000 (the trained-looking set has them).  Zero for every other channel, and for a
    degenerate clamp (lo == hi), whose operand is 0 in both."""
    from tennis_amd import weights as W
    f64 = np.float64
    mus = [q[PRE + f"stage1_batchnorm{2 * l}_running_mean"][:64] for l in range(W.BLOCK_CONFIG[0])] + [q[PRE + "batchnorm1_running_mean"][:64]]
    m = np.mean(np.asarray(mus, f64), 0).astype(np.float32)
    m[~np.isfinite(m)] = 0

    def thr(s, t):
        with np.errstate(all="ignore"):
            c = -t.astype(f64) / np.where(s != 0, s, 1).astype(f64)
            return np.clip(c, -65504.0, 65504.0).astype(np.float32).astype(np.float16).astype(f64)

    out = {}
    for l in range(W.BLOCK_CONFIG[0]):
        bn = PRE + f"stage1_batchnorm{2 * l}"
        g, b, mu, v = (q[bn + x][:64] for x in ("_gamma", "_beta", "_running_mean", "_running_var"))
        s = (g / np.sqrt(v + np.float32(W.BN_EPS))).astype(np.float32)
        t = (b - mu * s).astype(np.float32)
        tcen = (t.astype(f64) + s.astype(f64) * m.astype(f64)).astype(np.float32)
        slack = np.zeros(q[bn + "_gamma"].size)
        with np.errstate(all="ignore"):
            d = np.abs((thr(s, tcen) + m.astype(f64)) - thr(s, t))
        lo, hi, _, _ = W.bn_relu_clamp_fold(q, bn)
        slack[:64] = np.where(np.isfinite(d) & (lo[:64] != hi[:64]), d, 0.0)      # (a degenerate clamp is 0: no slack)
        out[PRE + f"stage1_conv{2 * l}_weight"] = slack
    return out


def _worst_by_kind(got, ref, slack):
    """per conv kind: max over its convolutions and channels of (|library - oracle| - slack) / max(1, |oracle|), and where"""
    worst = {k: 0.0 for k in KINDS}
    where = {}
    for name, (kind, _) in _kinds().items():
        r = ref[name]
        e = np.maximum(np.abs(got[name].astype(np.float64) - r) - slack.get(name, 0.0), 0.0) / np.maximum(1.0, np.abs(r))
        if float(e.max()) >= worst[kind]:
            worst[kind], where[kind] = float(e.max()), f"{name}[{int(e.argmax())}] oracle {float(r[e.argmax()]):.4g}"
    return worst, where


@pytest.mark.parametrize("size,batch", [(224, 3), (236, 1), (512, 1)])
@pytest.mark.parametrize("which", ["a_seeded", "b_degenerate", "c_trained_like"])
def test_input_means_against_fp64_oracle(param_sets, which, size, batch, report):
    from tennis_amd import weights as W
    from tennis_amd.engine import DenseNet121Features
    q = param_sets[which]
    frames = _frames(size, batch)
    enc = DenseNet121Features(q, size, max_batch=batch)
    x = torch.from_numpy(frames).cuda()
    got = enc.input_means(x)                  # (engine.input_means asserts the library's numel against the layout's)
    again = enc.input_means(x)
    kinds = _kinds()
    assert list(got) == list(kinds) and sum(v.size for v in got.values()) == 40736
    assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got)     # bit-identical on a repeat
    per_frame = OM.operand_means(q, frames)
    ref = {k: v.mean(0) for k, v in per_frame.items()}
    slack = _centred_threshold_slack(q)
    worst, where = _worst_by_kind(got, ref, slack)
    worst_abs = {kind: max(float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k, (kd, _) in kinds.items() if kd == kind) for kind in KINDS}
    tag = f"calib_stats_{which}_{size}_b{batch}"
    for kind in KINDS:
        report[f"{tag}_{kind}_err"] = worst[kind]
        report[f"{tag}_{kind}_at"] = where.get(kind, "")
        report[f"{tag}_{kind}_maxabs_raw"] = worst_abs[kind]
    # a dense 1x1 channel whose clamp is degenerate (lo == hi: a constant, or always clipped) has the operand 0 by the header's contract
    n_off = 0
    for name, (kind, bn) in kinds.items():
        if kind == "dense1x1":
            lo, hi, _, _ = W.bn_relu_clamp_fold(q, bn)
            off = lo == hi
            n_off += int(off.sum())
            assert (got[name][off] == 0).all(), (name, np.flatnonzero(off & (got[name] != 0))[:8], got[name][off & (got[name] != 0)][:8])
    report[f"{tag}_degenerate_channels"] = n_off
    if which == "b_degenerate":
        assert n_off >= 3
    if batch > 1:
        # the batch's statistic is the mean of the frames' own (the reduction is over batch x pixels; each call rounds once to fp32)
        singles = [enc.input_means(x[i:i + 1]) for i in range(batch)]
        dev = max(float(np.abs(got[k].astype(np.float64) - np.mean([s[k] for s in singles], 0)).max() /
                        max(1.0, float(np.abs(got[k]).max()))) for k in got)
        report[f"{tag}_batch_vs_mean_of_singles"] = dev
        assert dev < 5e-7, dev          # (measured: 1.3e-7)
        w1, where1 = _worst_by_kind(singles[0], {k: v[0] for k, v in per_frame.items()}, slack)
        for kind in KINDS:
            report[f"calib_stats_{which}_{size}_b1_{kind}_err"] = w1[kind]
            worst[kind] = max(worst[kind], w1[kind])
    print(tag, {k: f"{v:.2e}" for k, v in worst.items()}, where)
    for kind, bar in BARS["trained_like" if which == "c_trained_like" else "seeded"].items():
        assert worst[kind] < bar, (kind, worst[kind], where.get(kind))


# ---- state around the call -------------------------------------------------------------------------------------------------------

def test_input_means_between_pipelined_forwards(param_sets, report):
    """A pipelined encoder with max_batch 128 runs whole batches of 128 in two alternating workspace sets.  After each of two
    consecutive forwards (one per set) input_means on 2 frames gives what a fresh encoder gives, bit for bit; read_tap then hands
    out the calibration frames' activations (input_means runs in set 0 - the tap used to follow the last forward into set 1); and
    the next pipelined forward still gives the reference features bit for bit."""
    from tennis_amd.engine import DenseNet121Features
    q = param_sets["a_seeded"]
    taps = ("pool0", "stage1", "trans1")
    cal = torch.from_numpy(_frames(224, 2)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    x = torch.randint(0, 256, (128, 224, 224, 3), generator=g, device="cuda", dtype=torch.uint8)
    fresh = DenseNet121Features(q, 224, max_batch=128)
    ref_means = fresh.input_means(cal)
    ref_taps = {t: fresh.read_tap(t, 2).copy() for t in taps}
    ref_feat = fresh(x).clone()
    del fresh
    enc = DenseNet121Features(q, 224, max_batch=128)
    enc.set_pipelined(True)
    out = torch.empty_like(ref_feat)
    for i in range(3):
        enc(x, out=out)
        enc.join(0)
        assert torch.equal(out, ref_feat), f"pipelined forward {i}: features differ from the reference"
        if i == 2:
            break
        m = enc.input_means(cal)
        bad = [k for k in m if not np.array_equal(m[k].view(np.uint32), ref_means[k].view(np.uint32))]
        assert not bad, f"after forward {i}: input_means differs from a fresh encoder's in {bad[:4]}"
        for t in taps:
            got = enc.read_tap(t, 2)
            assert np.array_equal(got, ref_taps[t]), f"after forward {i} (workspace set {i}): read_tap({t!r}) differs by {np.abs(got - ref_taps[t]).max()}"
    enc.set_pipelined(False)
    report["calib_stats_pipelined_state"] = "ok"
