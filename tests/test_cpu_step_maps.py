"""No GPU: the temporal activation maps' float64 reference (tests/tools/step_maps_ref.py) and its identity, the driver's flag with
its refusals, the file format, the models' refusals, the ABI surface, and the ARG instantiations of the windowed recurrent kernel as
they compile for gfx950 (csrc/rnn_window.hip: code-object metadata of a device-only compile with the Makefile's flags - no scratch,
no spills; nothing else of the listing is read)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tools import step_maps_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tennis_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("tn_window_head_forward_tam", "tn_window_head_forward_rows_tam", "tn_temporal_pool_arg", "tn_temporal_pool_windows_arg",
               "tn_temporal_pool_rows_arg", "tn_dense_step_maps")


@pytest.mark.parametrize("mode", ["gru", "lstm"])
@pytest.mark.parametrize("hidden,window", [(8, 1), (8, 7), (32, 30)])
def test_reference_identity_in_float64(mode, hidden, window):
    """bias + sum_t tam = logit to 1e-12 (relative to |bias| + sum |W pooled|), the steps are first maxima that hold the pooled
    value, and the reverse direction's state at t is the state that has read t .. T-1 (checked on a one-step window and by
    reversing the input)."""
    from tennis_amd import weights as W
    feat, classes, S = 16, 5, 9
    p = W.make_rnn_weights(3, mode, feat, hidden, "r_")
    p.update(W.make_dense_weights(4, classes, 2 * hidden, "d_"))
    x = np.abs(np.random.default_rng(hidden + window).normal(0, 1, (S, window, feat))) * 0.5
    h = SR.head_sequence(x, p, mode, "r_")
    assert h.shape == (S, window, 2 * hidden)
    steps, pooled = SR.first_max(h)
    assert np.array_equal(pooled, h.max(1)) and steps.min() >= 0 and steps.max() < window
    for t in range(window):      # first: no earlier step holds the maximum
        assert not np.any((h[:, t] == pooled) & (steps > t))
    wd, bias = p["d_weight"].astype(np.float64), p["d_bias"].astype(np.float64)
    tam = SR.step_maps(pooled, steps, wd, window)
    assert tam.shape == (S, classes, window)
    logits = pooled @ wd.T + bias
    scale = np.abs(bias) + np.abs(pooled) @ np.abs(wd).T
    assert np.all(np.abs(bias + tam.sum(2) - logits) <= 1e-12 * scale)
    mass, sizes = SR.step_maps_abs(pooled, steps, wd, window)
    assert np.all(sizes.sum(1) == 2 * hidden) and np.all(tam[np.broadcast_to((sizes == 0)[:, None, :], tam.shape)] == 0.0)
    assert np.all(np.abs(tam) <= mass * (1 + 1e-12))
    # entries outside [0, window) contribute nothing
    bad = steps.copy()
    bad[:, ::3], bad[:, 1::3] = -1, window
    kept = SR.step_maps(pooled * ((bad >= 0) & (bad < window)), steps, wd, window)
    assert np.array_equal(SR.step_maps(pooled, bad, wd, window), kept)
    # the backward half of the reversed windows is the forward recurrence with the backward weights: its state order is flipped
    q = {k.replace("r_l0_", "r_X_").replace("r_r0_", "r_l0_").replace("r_X_", "r_r0_"): v for k, v in p.items()}
    hr = SR.head_sequence(x[:, ::-1], q, mode, "r_")
    assert np.allclose(hr[:, ::-1, :hidden], h[:, :, hidden:], rtol=0, atol=1e-14)


def test_save_tams_flag_and_refusals():
    from tennis_amd import evaluate as ev
    assert ev.build_parser().parse_args([]).save_tams is False
    ok = ["--window", "4", "--temp_pool", "gru"]
    assert ev.build_parser().parse_args(["--save_tams"] + ok).save_tams is True
    for bad, why in ((["--window", "1", "--temp_pool", "gru"], "--window 1"), (["--window", "4", "--temp_pool", "mean"], "mean"),
                     (["--window", "4"], "--temp_pool gru"), (ok + ["--save_feats"], "--save_feats"),
                     (ok + ["--corpus_frames", "64"], "--corpus_frames"), (ok + ["--num_gpus", "2"], "--num_gpus 1")):
        with pytest.raises(SystemExit, match=why):
            ev.main(["--save_tams", "--root", "/nonexistent"] + bad)             # refused before anything is opened or built
    for good in (ok, ["--window", "30", "--temp_pool", "lstm", "--feats_model", "0006"], ["--window", "8", "--temp_pool", "max", "--dense_windows"]):
        ev.check_save_tams(ev.build_parser().parse_args(["--save_tams"] + good))
    ev.check_save_tams(ev.build_parser().parse_args(["--window", "1"]))          # without the flag nothing is refused
    with pytest.raises(SystemExit, match="one rank"):
        ev.check_save_tams(ev.build_parser().parse_args(["--save_tams"] + ok), world=2)


def test_load_tams_round_trips_the_savers_file(tmp_path):
    from tennis_amd import evaluate as ev
    rng = np.random.default_rng(5)
    n, window = 6, 4
    cols = dict(tam=rng.normal(0, 1, (n, window)).astype(np.float32), pred=rng.integers(0, 11, n), label=rng.integers(0, 11, n),
                logit=rng.normal(0, 1, n).astype(np.float32), video=["V%03d" % (i // 3) for i in range(n)], frame=list(range(n)),
                frames=rng.integers(0, 9, (n, window)), bias=rng.normal(0, 1, n).astype(np.float32))
    path = str(tmp_path / "exp" / "0042" / "test_tams.npz")
    ev.save_tams(path, **cols)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(ev.TAM_COLUMNS) == ["bias", "frame", "frames", "label", "logit", "pred", "tam", "video"]
        assert z["video"].dtype.kind == "U" and z["tam"].dtype == np.float32 and z["frames"].shape == (n, window)
    got = ev.load_tams(path)
    for k in ("tam", "pred", "label", "logit", "frame", "frames", "bias"):
        assert np.array_equal(got[k], np.asarray(cols[k])), k
    assert list(got["video"]) == cols["video"]
    with pytest.raises(ValueError, match="entries"):
        ev.save_tams(path, **{**cols, "pred": cols["pred"][:3]})
    with pytest.raises(ValueError, match="frames"):
        ev.save_tams(path, **{**cols, "frames": cols["frames"][:, :2]})
    with pytest.raises(ValueError, match=r"\(N, window\)"):
        ev.save_tams(path, **{**cols, "tam": cols["tam"][:, :, None]})
    np.savez(str(tmp_path / "other.npz"), tam=cols["tam"])
    with pytest.raises(ValueError, match="save_tams"):
        ev.load_tams(str(tmp_path / "other.npz"))
    ev.save_cams(str(tmp_path / "cams.npz"), cam=np.zeros((n, 7, 7), np.float32), **{k: cols[k] for k in ("pred", "label", "logit", "video", "frame")})
    with pytest.raises(ValueError, match="save_tams"):
        ev.load_tams(str(tmp_path / "cams.npz"))


def test_models_refuse_what_has_no_maps():
    """raised before the GPU is touched: this test has none"""
    from tennis_amd.models.vision.definitions import CNNRNN, TemporalPooling
    x = np.zeros((2, 4, 16), np.float32)
    idx = np.zeros((2, 4), np.int64)
    mean = TemporalPooling(None, num_classes=11, pool="mean", feats=True)
    for call in (lambda: mean.forward(x, return_tam=True), lambda: mean.forward_windows(x[0], [0], [0], [3], 4, return_tam=True),
                 lambda: mean.forward_table(x[0], idx, return_tam=True)):
        with pytest.raises(ValueError, match="divided by the window"):
            call()
    for m in (CNNRNN(None, num_classes=-1), ):
        for call in (lambda: m.forward(x, return_tam=True), lambda: m.forward_windows(x[0], [0], [0], [3], 4, return_tam=True),
                     lambda: m.forward_table(x[0], idx, return_tam=True)):
            with pytest.raises(ValueError, match="classes"):
                call()


def test_abi_surface():
    from tennis_amd import _lib
    pub = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    declared = _lib.declared_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, pub, re.M), name
        assert name in declared and getattr(lib, name) is not None, name
    assert "models/vision/definitions.py" in pub[pub.index("Temporal activation maps"):pub.index("int tn_dense_step_maps(")]


# ---- the ARG instantiations as they compile for gfx950 ---------------------------------------------------------------------------

def _hflags():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    flags = re.search(r"^HFLAGS := \$\(EXTRA\) (.*)$", mk, re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def _meta(text):
    """{kernel name: {field: int}} from the amdhsa.kernels metadata"""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}
    return out


@pytest.fixture(scope="module")
def window_meta(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rnn_window_isa") / "rnn_window.s")
    p = subprocess.run([HIPCC] + _hflags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "rnn_window.hip"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    text = open(out).read()
    return _meta(text[text.index("amdhsa.kernels:"):])


def test_arg_instantiations_keep_out_of_scratch(window_meta):
    """rnn_window_kernel<G, NB, KR, DPP, MAXT, TAB, ARG>: every ARG instantiation - and every other kernel of the unit - has no private
    segment and no spills, within the registers its launch bound leaves a wave (128 at 1024 threads, 256 at 512).  The set: both
    cells x both rows-per-workgroup x the three forms x both row sources, except the plain LSTM form at 8 rows, which does not fit
    with the steps and which the ARG dispatch runs at 4 rows (docs/kernels.md)."""
    kern = {}
    for n, f in window_meta.items():
        m = re.search(r"rnn_window_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d+)ELb(\d)ELb(\d)E", n)
        if m:
            kern[tuple(int(v) for v in m.groups())] = f
    forms = ((128, 1, 512), (0, 1, 1024), (0, 0, 1024))
    full = {(g, nb) + form + (tab, arg) for g, nbs in ((3, (4, 6)), (4, (4, 8))) for nb in nbs for form in forms for tab in (0, 1)
            for arg in (0, 1)}
    assert set(kern) == full - {(4, 8, 0, 0, 1024, 0, 1), (4, 8, 0, 0, 1024, 1, 1)}, sorted(set(kern) ^ full)
    assert sum(1 for k in kern if k[-1] == 1) == 22
    for k, f in kern.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (k, f)
        assert f["max_flat_workgroup_size"] == k[4] and f["vgpr_count"] <= (128 if k[4] == 1024 else 256), (k, f)
    pools = {n: f for n, f in window_meta.items() if "temporal_pool_windows_kernel" in n}
    assert len(pools) == 4
    for f in pools.values():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, f
