"""Global-norm gradient clipping, the parts that need no GPU: the drivers' flags (both off by default; ``--clip`` alone still
ignored), the entry points in the headers, the ctypes table and the built library, and the float64 helper of the GPU tests
(tests/tools/grad_clip_ref.py) against ``torch.nn.utils.clip_grad_norm_``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tools import grad_clip_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = ("tn_head", "tn_finetune", "tn_cnnrnn_trainer", "tn_gnmt_trainer", "tn_gnmt_frames_trainer")


def test_train_parser_has_clip_grad_norm_default_off():
    from tennis_amd.train import build_parser
    assert build_parser().parse_args([]).clip_grad_norm == 0.0
    assert build_parser().parse_args(["--clip_grad_norm", "2.5"]).clip_grad_norm == 2.5


def test_train_gnmt_parser_has_apply_clip_default_off():
    from tennis_amd.train_gnmt import applied_clip, build_parser
    flags = build_parser().parse_args([])
    assert flags.apply_clip is False and flags.clip == 5.0 and applied_clip(flags) == 0.0
    flags = build_parser().parse_args(["--clip", "3.0"])
    assert flags.clip == 3.0 and applied_clip(flags) == 0.0                    # the reference's flag alone: parsed, ignored
    flags = build_parser().parse_args(["--clip", "3.0", "--apply_clip"])
    assert applied_clip(flags) == 3.0
    assert applied_clip(build_parser().parse_args(["--apply_clip"])) == 5.0


@pytest.mark.parametrize("argv,expected", [([], 0.0), (["--clip", "3.0"], 0.0), (["--clip", "3.0", "--apply_clip"], 3.0)])
def test_train_gnmt_main_hands_clip_to_train_only_under_apply_clip(monkeypatch, tmp_path, argv, expected):
    """main() with build and train replaced: what reaches train(..., clip=) - and that --clip alone changes no other argument"""
    from tennis_amd import train_gnmt as tg

    class _Set:
        def get_captions(self, split=True):
            return [["a"]]

    class _Model:
        src_embed = None

    seen = []
    monkeypatch.setattr(tg, "build", lambda flags: (_Set(), _Set(), _Set(), _Model(), None))
    monkeypatch.setattr(tg, "train", lambda *a, **kw: seen.append(kw) or [])
    for extra in ([], argv):
        assert tg.main(["--root", str(tmp_path), "--model_id", "x"] + extra) == 0
    base, got = seen
    assert base["clip"] == 0.0 and got["clip"] == expected
    assert {k: v for k, v in got.items() if k != "clip"} == {k: v for k, v in base.items() if k != "clip"}


def test_apply_clip_refuses_a_threshold_that_is_not_positive(tmp_path):
    from tennis_amd import train_gnmt as tg
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            tg.main(["--root", str(tmp_path), "--apply_clip", "--clip", bad])


def test_entry_points_are_declared_and_exported():
    from tennis_amd import _lib
    header = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    debug = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    public = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", header))
    hooks = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", debug))
    names = [f"{h}_{f}" for h in HANDLES for f in ("set_clip", "clip_stats")]
    assert all(n in public and n not in hooks for n in names)
    assert "tn_dbg_grad_sumsq" in hooks and "tn_dbg_grad_sumsq" not in public
    assert "clip_global_norm" in header and "train_gnmt.py:97-98" in header       # the call it mirrors, the flag's definition
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names + ["tn_dbg_grad_sumsq"]:
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    c = ref.kernel_constants()
    assert c["CHUNK"] % (4 * c["BLOCK"]) == 0 and c["BLOCK"] % 64 == 0


def test_every_trainer_class_has_the_two_methods():
    from tennis_amd import engine
    for cls in (engine.TemporalHeadTrainer, engine.FrameModelTrainer, engine.CNNRNNTrainer, engine.GNMTTrainer, engine.GNMTFramesTrainer):
        assert cls.set_clip is engine._FlatTrainer.set_clip and cls.clip_stats is engine._FlatTrainer.clip_stats


@pytest.mark.parametrize("seed,max_norm", [(0, 1.0), (1, 5.0), (2, 1e3)])
def test_helper_agrees_with_torch_clip_grad_norm(seed, max_norm):
    """torch adds 1e-6 to the norm, MXNet 1e-8: with a norm >= 10 the two scales agree to 1e-7 relative, far inside the 1e-6 here"""
    rng = np.random.default_rng(seed)
    grads = {"a": rng.normal(0, 3, (17, 5)), "b": rng.normal(0, 3, (129,)), "c": rng.normal(0, 3, (2, 3, 4))}
    norm = ref.global_norm(grads)
    assert norm >= 10.0
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads.values()]
    for p, g in zip(ps, grads.values()):
        p.grad = torch.from_numpy(g.copy())
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    assert abs(total - norm) <= 1e-12 * norm
    scale = ref.clip_scale(norm, max_norm)
    assert (scale == 1.0) == (norm + 1e-8 <= max_norm)
    for p, g in zip(ps, grads.values()):
        want = scale * g
        assert np.abs(p.grad.numpy() - want).max() <= 1e-6 * np.abs(want).max()


def test_helper_scale_edges():
    assert ref.clip_scale(2.0, 4.0) == 1.0 and ref.clip_scale(4.0, 4.0) == 1.0 / (1.0 + 1e-8 / 4.0)
    assert ref.clip_scale(8.0, 2.0) == pytest.approx(0.25, rel=1e-8)
    assert np.isnan(ref.clip_scale(float("nan"), 1.0)) and ref.clip_scale(float("inf"), 1.0) == 0.0
    assert ref.global_norm([np.array([3.0]), np.array([4.0])], rescale=0.5) == 2.5


def test_helper_updates_under_the_threshold_equal_the_unclipped_ones():
    rng = np.random.default_rng(3)
    p = {"w": rng.normal(0, 1, (7, 3)), "b": rng.normal(0, 1, (3,))}
    gs = [{k: rng.normal(0, 1, v.shape) for k, v in p.items()} for _ in range(3)]
    for make in (lambda mn: ref.ClippedSGD(p, 1e-2, 0.9, 1e-4, 0.5, mn), lambda mn: ref.ClippedAdam(p, 1e-3, max_norm=mn)):
        plain, loose, tight = make(None), make(1e9), make(1e-2)
        for g in gs:
            plain.step(g), loose.step(g), tight.step(g)
        assert all(np.array_equal(plain.w[k], loose.w[k]) for k in p) and loose.scales == [1.0] * 3
        assert all(s < 1.0 for s in tight.scales) and not any(np.array_equal(plain.w[k], tight.w[k]) for k in p)
