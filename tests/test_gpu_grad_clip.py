"""-m gpu: opt-in global-norm gradient clipping (``tn_<handle>_set_clip`` / ``_clip_stats``; ``_FlatTrainer.set_clip`` /
``clip_stats``; ``train_gnmt --apply_clip``, ``train --clip_grad_norm``).

1. the two-stage sum of squares through ``tn_dbg_grad_sumsq`` at every edge of its layout, against float64 of the same fp32 values
   at the bound tests/tools/grad_clip_ref.py derives from the kernel's constants;
2. each of the five trainers at the smallest shapes its own step tests use: the norm, a step under the threshold bit-identical to
   an unclipped twin's, two clipped steps on two batches against the float64 replica carried from zero state;
3. the two-part handles: one norm over both buffers, a frozen backbone outside it and untouched;
4. the gradient buffers keep their bits through a clipped step (asserted inside 2 and 3);
5. the ABI's refusals;
6. the two drivers."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from tools import grad_clip_ref as ref

pytestmark = pytest.mark.gpu

K = ref.kernel_constants()
CHUNK, GRID = K["CHUNK"], K["GRID"]
PASS = CHUNK * GRID                                  # floats the grid covers in its first pass
SMALL = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257]
LENGTHS = SMALL + [CHUNK - 1, CHUNK, CHUNK + 1, PASS - 1, PASS, PASS + 1]
BIG = 8 * 1024 * 1024 + 5                            # the backbone's gradient buffer is about 8 M floats
POOL = BIG + 8


def _ctx():
    from tennis_amd import _lib
    return _lib.default_context()


def _sumsq(a, b=None):
    from tennis_amd import _lib
    ctx = _ctx()
    out = C.c_double()
    _lib.check(ctx.lib.tn_dbg_grad_sumsq(ctx.handle, _lib.ptr(a), a.numel() if a is not None else 0, _lib.ptr(b),
                                         b.numel() if b is not None else 0, C.byref(out)), "tn_dbg_grad_sumsq")
    return out.value


@functools.lru_cache(maxsize=None)
def _pools():
    """(normals on the host, the same on the device, ones, zeros): each allocated once, on a 16-byte boundary, sliced per case"""
    host = np.random.default_rng(17).standard_normal(POOL).astype(np.float32)
    dev = torch.from_numpy(host).cuda()
    ones, zeros = torch.ones(POOL, device="cuda"), torch.zeros(POOL, device="cuda")
    assert all(t.data_ptr() % 16 == 0 for t in (dev, ones, zeros))
    return host, dev, ones, zeros


def _spike_positions(n, off):
    """first and last index, both sides of the 16-byte boundary behind the head, of the tail's start, and of chunk boundaries: all
    of them up to three chunks, else the first two, the two around the grid's wrap and the last"""
    head = min(n, (4 - off) % 4)
    body4 = (n - head) // 4
    pos = {0, n - 1, head - 1, head, head + 4 * body4 - 1, head + 4 * body4}
    chunks = -(-4 * body4 // CHUNK)
    ks = range(1, chunks) if chunks <= 3 else [1, 2, GRID - 1, GRID, GRID + 1, chunks - 1]
    for k in ks:
        pos |= {head + k * CHUNK - 1, head + k * CHUNK}
    return sorted(p for p in pos if 0 <= p < n)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_reduction_all_ones_and_single_spikes_are_exact(off):
    """buffers starting 0, 4, 8 and 12 bytes past a 16-byte boundary; sums of ones below 2^24 and a lone 1e3^2 have no rounding"""
    _, _, ones, zeros = _pools()
    for n in LENGTHS:
        assert _sumsq(ones[off:off + n]) == float(n), (n, off)
        z = zeros[off:off + n]
        for p in _spike_positions(n, off):
            z[p] = 1e3
            got = _sumsq(z)
            z[p] = 0.0
            assert got == 1e6, (n, off, p, got)
    assert float(zeros.abs().max()) == 0.0


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_reduction_of_normals_within_the_bound_and_repeatable(report, off):
    host, dev, _, _ = _pools()
    worst = 0.0
    for n in LENGTHS:
        want = float((host[off:off + n].astype(np.float64) ** 2).sum())
        got = _sumsq(dev[off:off + n])
        assert got == _sumsq(dev[off:off + n]), (n, off)                      # the same bits on a second call
        err, bound = abs(got - want) / want, ref.sumsq_rel_bound([n])
        print(f"sumsq normals n={n} off={off}: rel err {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (n, off, err, bound)
        worst = max(worst, err / bound)
    report[f"grad_sumsq_normals_off{off}_worst_err_over_bound"] = worst


def test_reduction_two_segments(report):
    host, dev, ones, _ = _pools()
    worst = 0.0
    for n in SMALL + [CHUNK + 1]:
        a = dev[1:1 + n]
        want_a = float((host[1:1 + n].astype(np.float64) ** 2).sum())
        for b, hb in ((None, None), (dev[POOL - 1:POOL], host[POOL - 1:POOL]), (dev[4099:4099 + 2 * CHUNK + 3], host[4099:4099 + 2 * CHUNK + 3])):
            want = want_a + (float((hb.astype(np.float64) ** 2).sum()) if hb is not None else 0.0)
            got = _sumsq(a, b)
            nb = 0 if b is None else b.numel()
            err, bound = abs(got - want) / want, ref.sumsq_rel_bound([n, nb])
            assert err <= bound and got == _sumsq(a, b), (n, nb, err, bound)
            worst = max(worst, err / bound)
        assert _sumsq(None, a) == _sumsq(a)                                 # an empty first segment
        assert _sumsq(ones[2:2 + n], ones[3:4]) == float(n + 1)
    assert _sumsq(None, None) == 0.0
    report["grad_sumsq_two_segments_worst_err_over_bound"] = worst


def test_reduction_at_the_backbone_size(report):
    host, dev, ones, zeros = _pools()
    assert _sumsq(ones[1:1 + BIG]) == float(BIG)
    z = zeros[1:1 + BIG]
    for p in (0, BIG - 1, 3 + PASS - 1, 3 + PASS):
        z[p] = 1e3
        got = _sumsq(z)
        z[p] = 0.0
        assert got == 1e6, p
    want = float((host[1:1 + BIG].astype(np.float64) ** 2).sum())
    got = _sumsq(dev[1:1 + BIG])
    err, bound = abs(got - want) / want, ref.sumsq_rel_bound([BIG])
    print(f"sumsq normals n={BIG}: rel err {err:.2e} (bound {bound:.2e})")
    report["grad_sumsq_8m_rel_err"] = err
    assert err <= bound and got == _sumsq(dev[1:1 + BIG])


# ---- the trainers ------------------------------------------------------------------------------------------------------------
LR_SGD, MOM, WD, LR_ADAM = 1e-2, 0.9, 1e-4, 1e-3


def _tup(v):
    return v if isinstance(v, tuple) else (v,)


def _flat_norm(tr, rescale):
    return ref.global_norm([g.cpu().numpy() for g in _tup(tr.grads)], rescale)


def _norm_bound(tr):
    """the sum's bound covers the norm: the square root halves a relative error, the rounding to fp32 adds 2^-24"""
    return ref.sumsq_rel_bound([g.numel() for g in _tup(tr.grads)])


def _same_params(a, b):
    return all(torch.equal(x, y) for x, y in zip(_tup(a.params), _tup(b.params)))


def _trainable(tr, skip_prefix=None):
    return [k for k in tr.names if not k.endswith(("running_mean", "running_var")) and not (skip_prefix and k.startswith(skip_prefix))]


def _check_trainer(report, tag, make, fb, kind, batch_size=None):
    """make() -> a fresh trainer on the same parameters; fb(tr, i): forward_backward on batch i (0 or 1); kind 'sgd' | 'adam'"""
    rescale = 1.0 / batch_size if kind == "sgd" else 1.0
    step = (lambda t: t.step(batch_size, LR_SGD, MOM, WD)) if kind == "sgd" else (lambda t: t.step(LR_ADAM))
    probe, plain, clipped = make(), make(), make()
    names = _trainable(probe)
    # the norm, and a step under the threshold
    fb(probe, 0), fb(plain, 0)
    norm64 = _flat_norm(probe, rescale)
    assert norm64 > 0 and abs(ref.global_norm({k: probe.get(k, gradient=True) for k in names}, rescale) - norm64) <= 1e-9 * norm64
    before = [g.clone() for g in _tup(probe.grads)]
    probe.set_clip(2 * norm64)
    step(probe), step(plain)
    norm, scale, count = probe.clip_stats()
    e_norm = abs(norm - norm64) / norm64
    print(f"{tag}: norm {norm:.6e} float64 {norm64:.6e} rel err {e_norm:.2e} (bound {_norm_bound(probe):.2e})")
    report[f"grad_clip_{tag}_norm_rel_err"] = e_norm
    assert e_norm <= _norm_bound(probe)
    assert scale == 1.0 and count == 0
    assert all(torch.equal(a, b) for a, b in zip(before, _tup(probe.grads))), "a clipped step changed the gradient buffer"
    assert _same_params(probe, plain), "a step under the threshold differs from the unclipped step"
    # two clipped steps on two batches against the float64 replica from zero state
    max_norm = norm64 / 4
    p0 = {k: clipped.get(k) for k in names}
    opt = ref.ClippedSGD(p0, LR_SGD, MOM, WD, rescale, max_norm) if kind == "sgd" else ref.ClippedAdam(p0, LR_ADAM, max_norm=max_norm)
    clipped.set_clip(max_norm)
    for i in (0, 1):
        fb(clipped, i)
        grads = {k: clipped.get(k, gradient=True) for k in names}
        before = [g.clone() for g in _tup(clipped.grads)]
        step(clipped)
        assert all(torch.equal(a, b) for a, b in zip(before, _tup(clipped.grads)))
        opt.step(grads)
    fb(plain, 1)
    step(plain)
    norm, scale, count = clipped.clip_stats()
    assert count == 2 and scale < 1.0 and all(s < 1.0 for s in opt.scales)
    assert abs(norm - opt.norms[-1]) <= _norm_bound(clipped) * opt.norms[-1] and abs(scale - opt.scales[-1]) <= 1e-6 * opt.scales[-1]
    worst = 0.0
    for k in names:
        w = opt.w[k]
        err = float(np.abs(clipped.get(k).reshape(w.shape) - w).max() / np.abs(w).max())
        worst = max(worst, err)
        assert err < 1e-5, (k, err)
    print(f"{tag}: worst parameter error after two clipped steps relative to the tensor's maximum: {worst:.2e}")
    report[f"grad_clip_{tag}_param_rel_err"] = worst
    assert not _same_params(clipped, plain), "two clipped steps left the parameters of two unclipped ones"


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_head_trainer(report, cell):
    from tennis_amd import weights as W
    from tennis_amd.engine import TemporalHeadTrainer
    B, T, F, H, classes = 3, 4, 8, 8, 11
    p = W.make_rnn_weights(4, cell, F, H, f"cnnrnn0_{cell}0_")
    p.update(W.make_dense_weights(5, classes, 2 * H, "cnnrnn0_dense0_"))
    rng = np.random.default_rng(4)
    xs = [torch.from_numpy((np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)).cuda() for _ in range(2)]
    ys = [torch.from_numpy(rng.integers(0, classes, B).astype(np.int32)).cuda() for _ in range(2)]
    _check_trainer(report, f"head_{cell}", lambda: TemporalHeadTrainer(p, F, H, classes, max_batch=B, max_steps=T, type=cell),
                   lambda tr, i: tr.forward_backward(xs[i], ys[i]), "sgd", B)


def _gnmt_case(seed, cell):
    from test_gpu_gnmt_train import _case
    cfg = dict(B=3, T=9, F=16, H=8, E=6, V=14, L=6)                       # test_gpu_gnmt_train's smallest
    p, *batch0 = _case(seed, cell=cell, **cfg)
    _, *batch1 = _case(seed + 100, cell=cell, **cfg)
    return cfg, p, [[torch.from_numpy(a).cuda() for a in b] for b in (batch0, batch1)]


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_captioner_trainer(report, cell):
    from tennis_amd.engine import GNMTTrainer
    cfg, p, batches = _gnmt_case(1, cell)
    make = lambda: GNMTTrainer(p, cfg["F"], cfg["H"], cfg["E"], cfg["V"], max_batch=cfg["B"], max_src_len=cfg["T"], max_tgt_len=cfg["L"],
                               cell_type=cell)
    _check_trainer(report, f"gnmt_{cell}", make, lambda tr, i: tr.forward_backward(*batches[i]), "adam")


@functools.lru_cache(maxsize=None)
def _backbone():
    from tennis_amd import weights as W
    return W.make_densenet121_weights(0)


def _frames(n, seed):
    from tennis_amd import weights as W
    return torch.from_numpy(W.normalize_to_nchw_f32(W.synthetic_frames_u8(n, 224, seed))).cuda()


def test_frame_classifier_trainer(report):
    from tennis_amd import weights as W
    from tennis_amd.engine import FrameModelTrainer
    B = 2
    p = dict(_backbone())
    p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
    xs = [_frames(B, s) for s in (5, 6)]
    ys = [torch.from_numpy(np.random.default_rng(s).integers(0, 11, B).astype(np.int32)).cuda() for s in (5, 6)]
    _check_trainer(report, "finetune", lambda: FrameModelTrainer(p, 224, 11, batch=B), lambda tr, i: tr.forward_backward(xs[i], ys[i]),
                   "sgd", B)


def _cnnrnn_setup():
    from tennis_amd import weights as W
    B, T = 2, 3
    p = dict(_backbone())
    p.update(W.make_rnn_weights(2, "gru", 1024, 128, "cnnrnn0_gru0_"))
    p.update(W.make_dense_weights(1, 11, 256, "cnnrnn0_dense0_"))
    xs = [_frames(B * T, s).reshape(B, T, 3, 224, 224) for s in (5, 6)]
    ys = [torch.from_numpy(np.random.default_rng(s).integers(0, 11, B).astype(np.int32)).cuda() for s in (5, 6)]
    return B, T, p, xs, ys


def test_cnnrnn_trainer_one_norm_over_both_parts(report):
    from tennis_amd.engine import CNNRNNTrainer
    B, T, p, xs, ys = _cnnrnn_setup()
    _check_trainer(report, "cnnrnn", lambda: CNNRNNTrainer(p, 224, 11, batch=B, steps=T), lambda tr, i: tr.forward_backward(xs[i], ys[i]),
                   "sgd", B)


def _gnmt_frames_setup():
    from test_gpu_gnmt_frames_train import E, L, SVL, V, _targets
    from tennis_amd import weights as W
    B, T, H = 2, 3, 8
    p = dict(_backbone())
    p.update(W.make_gnmt_weights(5, "gru", 1024, H, E, V))
    p["gnmt_tgt_embed_weight"] = np.random.default_rng(5).normal(0, 0.5, (V, E)).astype(np.float32)
    batches = []
    for s in (5, 6):
        tgt, tvl = _targets(B, s)
        batches.append((_frames(B * T, s).reshape(B, T, 3, 224, 224), torch.tensor(SVL, dtype=torch.int32).cuda(),
                        torch.from_numpy(tgt).cuda(), torch.from_numpy(tvl).cuda()))
    return p, H, E, V, L, batches


def test_gnmt_frames_trainer_one_norm_over_both_parts(report):
    from tennis_amd.engine import GNMTFramesTrainer
    p, H, E, V, L, batches = _gnmt_frames_setup()
    make = lambda: GNMTFramesTrainer(p, H, E, V, size=224, max_batch=2, max_src_len=3, max_tgt_len=L)
    _check_trainer(report, "gnmt_frames", make, lambda tr, i: tr.forward_backward(*batches[i]), "adam")


def _check_frozen(report, tag, tr, fb, step, rescale):
    """frozen backbone: the norm is the head's / captioner's buffer alone (``grads`` leaves the backbone's out), the backbone's
    parameters keep their bits through a clipped step that bites"""
    fb(tr)
    assert len(_tup(tr.grads)) == 1 and len(_tup(tr.params)) == 2
    norm64 = _flat_norm(tr, rescale)
    bb_before, top_before = tr.params[0].clone(), tr.params[1].clone()
    tr.set_clip(norm64 / 4)
    step(tr)
    norm, scale, count = tr.clip_stats()
    e_norm = abs(norm - norm64) / norm64
    report[f"grad_clip_{tag}_frozen_norm_rel_err"] = e_norm
    assert e_norm <= _norm_bound(tr) and count == 1 and abs(scale - 0.25) < 1e-6
    assert torch.equal(bb_before, tr.params[0]) and not torch.equal(top_before, tr.params[1])


def test_cnnrnn_trainer_frozen_backbone_is_outside_the_norm(report):
    from tennis_amd.engine import CNNRNNTrainer
    B, T, p, xs, ys = _cnnrnn_setup()
    tr = CNNRNNTrainer(p, 224, 11, batch=B, steps=T, freeze_backbone=True)
    _check_frozen(report, "cnnrnn", tr, lambda t: t.forward_backward(xs[0], ys[0]), lambda t: t.step(B, LR_SGD, MOM, WD), 1.0 / B)


def test_gnmt_frames_trainer_frozen_backbone_is_outside_the_norm(report):
    from tennis_amd.engine import GNMTFramesTrainer
    p, H, E, V, L, batches = _gnmt_frames_setup()
    tr = GNMTFramesTrainer(p, H, E, V, size=224, max_batch=2, max_src_len=3, max_tgt_len=L, freeze_backbone=True)
    _check_frozen(report, "gnmt_frames", tr, lambda t: t.forward_backward(*batches[0]), lambda t: t.step(LR_ADAM), 1.0)


# ---- the ABI's refusals ------------------------------------------------------------------------------------------------------
def test_abi_refusals_and_switching_off():
    from tennis_amd import _lib
    from tennis_amd.engine import GNMTTrainer
    lib = _lib.load()
    f, i64 = C.c_float(), C.c_int64()
    for h in ("tn_head", "tn_finetune", "tn_cnnrnn_trainer", "tn_gnmt_trainer", "tn_gnmt_frames_trainer"):
        assert getattr(lib, h + "_set_clip")(None, 1.0) != 0 and b"null handle" in lib.tn_last_error()
        assert lib.tn_last_error().decode() == f"invalid argument: {h}_set_clip: null handle"      # (the two-part handles too: their own name)
        assert getattr(lib, h + "_clip_stats")(None, C.byref(f), C.byref(f), C.byref(i64)) != 0 and b"null handle" in lib.tn_last_error()
        assert lib.tn_last_error().decode() == f"invalid argument: {h}_clip_stats: null handle"
    cfg, p, batches = _gnmt_case(1, "gru")
    make = lambda: GNMTTrainer(p, cfg["F"], cfg["H"], cfg["E"], cfg["V"], max_batch=cfg["B"], max_src_len=cfg["T"], max_tgt_len=cfg["L"])
    tr, twin = make(), make()
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        assert lib.tn_gnmt_trainer_set_clip(tr.handle, bad) != 0 and b"max_norm" in lib.tn_last_error()
        with pytest.raises(RuntimeError, match="max_norm"):
            tr.set_clip(bad)
    with pytest.raises(RuntimeError, match="clipping is off"):
        tr.clip_stats()                                                     # off after create
    tr.set_clip(1.0)
    with pytest.raises(RuntimeError, match="no step"):
        tr.clip_stats()                                                     # on, and no step yet
    tr.set_clip(0.0)
    with pytest.raises(RuntimeError, match="clipping is off"):
        tr.clip_stats()
    # set_clip(0) after set_clip(1): the next step is the never-clipped twin's, bit for bit
    for t in (tr, twin):
        t.forward_backward(*batches[0])
        t.step(LR_ADAM)
    assert torch.equal(tr.params, twin.params)
    with pytest.raises(RuntimeError, match="clipping is off"):
        tr.clip_stats()
    # any output pointer may be NULL
    tr.set_clip(1e-3)
    tr.forward_backward(*batches[1])
    tr.step(LR_ADAM)
    assert lib.tn_gnmt_trainer_clip_stats(tr.handle, None, None, C.byref(i64)) == 0 and i64.value == 1
    assert lib.tn_gnmt_trainer_clip_stats(tr.handle, C.byref(f), None, None) == 0 and f.value > 1e-3


# ---- the drivers -------------------------------------------------------------------------------------------------------------
def test_train_gnmt_driver_clip(tmp_path):
    """train_gnmt.train for one epoch: clip=1e9 never bites and leaves the parameters of clip=0.0; a small clip bites every step"""
    from tennis_amd.captions import CaptionSet
    from tennis_amd.models.captioning.gnmt import NMTModel, get_gnmt_encoder_decoder
    from tennis_amd.train_gnmt import train
    from tennis_amd.utils.translation import BeamSearchScorer, BeamSearchTranslator
    tr_set = CaptionSet(split="train", n_points=16, feature_dim=48, mean_frames=10, max_cap_len=50)
    va_set = CaptionSet(split="val", n_points=6, feature_dim=48, mean_frames=10, vocab=tr_set.vocab, inference=True)
    enc, dec = get_gnmt_encoder_decoder(cell_type="gru", hidden_size=24, num_layers=2, num_bi_layers=1)
    model = NMTModel(src_vocab=None, tgt_vocab=tr_set.vocab, encoder=enc, decoder=dec, embed_size=12, prefix="gnmt_", input_size=48)
    model.initialize()
    translator = BeamSearchTranslator(model=model, beam_size=4, scorer=BeamSearchScorer(alpha=1.0, K=5), max_length=20)
    start = {k: np.array(v.data, copy=True) for k, v in model.collect_params().items()}
    finals, hists, logs = {}, {}, {}
    for clip in (0.0, 1e9, 1e-3):
        model.set_params(start)
        logs[clip] = []
        save = tmp_path / f"clip{clip:g}"
        hists[clip] = train(tr_set, va_set, None, model, translator, epochs=1, batch_size=8, lr=2e-2, save_dir=str(save), log=logs[clip].append,
                            clip=clip)
        assert (save / "0000.params").exists()
        finals[clip] = {k: np.array(v.data, copy=True) for k, v in model.collect_params().items()}
    assert "grad_norm" not in hists[0.0][0] and "clipped_steps" not in hists[0.0][0]
    assert not any("grad_norm" in l for l in logs[0.0])
    assert hists[1e9][0]["clipped_steps"] == 0 and np.isfinite(hists[1e9][0]["grad_norm"]) and hists[1e9][0]["grad_norm"] > 0
    assert all(np.array_equal(finals[0.0][k], finals[1e9][k]) for k in start)
    assert (tmp_path / "clip0" / "0000.params").read_bytes() == (tmp_path / "clip1e+09" / "0000.params").read_bytes()
    assert hists[1e-3][0]["clipped_steps"] > 0 and hists[1e-3][0]["grad_norm"] > 1e-3
    assert any("grad_norm=" in l and "clipped_steps=" in l for l in logs[1e-3])
    assert any(not np.array_equal(finals[0.0][k], finals[1e-3][k]) for k in start)


def test_train_driver_dense_windows_clip_grad_norm(tmp_path, capsys):
    """evaluate --save_feats, then train --feats_model --window 4 --temp_pool gru --dense_windows for one epoch: --clip_grad_norm 1e9
    leaves the parameters of a run without the flag, a small one bites and the epoch's line says so"""
    from tennis_amd import evaluate as ev, train as tr
    from tennis_amd.params_io import load_mxnet_params
    root = str(tmp_path / "data")
    common = ["--root", root, "--frames_per_video", "12", "--data_shape", "224", "--model_id", "0001"]
    for split in ("train", "val"):
        assert ev.main(common + ["--split", split, "--save_feats", "--batch_size", "8"]) == 0
    capsys.readouterr()
    finals, outs = [], []
    for model_id, extra in (("0002", []), ("0003", ["--clip_grad_norm", "1e9"]), ("0004", ["--clip_grad_norm", "1e-6"])):
        exp = str(tmp_path / "exp")
        args = ["--root", root, "--frames_per_video", "12", "--data_shape", "224", "--model_id", model_id, "--feats_model", "0001",
                "--window", "4", "--temp_pool", "gru", "--epochs", "1", "--batch_size", "8", "--lr", "0.01", "--exp_root", exp,
                "--dense_windows"] + extra
        assert tr.main(args) == 0
        finals.append(load_mxnet_params(str(tmp_path / "exp" / model_id / "0000.params")))
        outs.append(capsys.readouterr().out)
    counts = [re.findall(r"grad_norm=(\S+) \(last step\), clipped_steps=(\d+) of (\d+)", o) for o in outs]
    assert counts[0] == [] and len(counts[1]) == 1 and len(counts[2]) == 1
    assert int(counts[1][0][1]) == 0 and float(counts[1][0][0]) > 0
    assert int(counts[2][0][1]) == int(counts[2][0][2]) > 0
    assert set(finals[0]) == set(finals[1]) == set(finals[2]) and len(finals[0]) >= 10
    assert all(np.array_equal(np.asarray(finals[0][k]), np.asarray(finals[1][k])) for k in finals[0])
    assert any(not np.array_equal(np.asarray(finals[0][k]), np.asarray(finals[2][k])) for k in finals[0])
