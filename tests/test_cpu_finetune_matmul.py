"""The fp32x3 matrix mode of the backbone training steps (TN_MATMUL_FP32X3) on the host side: the mode's values and entry points in
the C headers, the ctypes table and the built library, ``--matmul`` of train.py / train_gnmt.py, and the trainers' ``matmul=``
check, which runs before a context or the library is touched.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ("tn_finetune_set_matmul", "tn_finetune_matmul_stats", "tn_cnnrnn_trainer_set_matmul", "tn_cnnrnn_trainer_matmul_stats",
                "tn_gnmt_frames_trainer_set_matmul", "tn_gnmt_frames_trainer_matmul_stats")
HOOKS = ("tn_dbg_linear_fp32x3", "tn_dbg_gemm_tn_fp32x3")


def test_mode_values_and_entry_points_in_the_headers():
    header = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    assert re.search(r"^#define TN_MATMUL_F32 0\b", header, re.M)
    assert re.search(r"^#define TN_MATMUL_FP32X3 1\b", header, re.M)
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
    debug = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    for name in HOOKS:
        assert re.search(r"^int %s\(" % name, debug, re.M), name
        assert name not in header                                  # test hooks stay out of the public header


def test_symbols_declared_and_exported():
    from tennis_amd import _lib
    assert _lib.MATMUL_MODES == {"f32": 0, "fp32x3": 1}
    declared = _lib.declared_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS + HOOKS:
        assert name in declared, name
        assert getattr(lib, name) is not None, name


def test_train_parser_takes_matmul():
    from tennis_amd import train
    p = train.build_parser()
    assert p.parse_args([]).matmul == "f32"
    assert p.parse_args(["--matmul", "fp32x3"]).matmul == "fp32x3"
    with pytest.raises(SystemExit):
        p.parse_args(["--matmul", "bf16"])
    # on features there is no backbone in the step
    flags = p.parse_args(["--feats_model", "0006", "--window", "4", "--temp_pool", "gru", "--matmul", "fp32x3"])
    with pytest.raises(SystemExit) as ei:
        train.check_frames_route(flags)
    assert "no backbone" in str(ei.value)
    train.check_frames_route(p.parse_args(["--feats_model", "0006", "--window", "4", "--temp_pool", "gru"]))


def test_train_gnmt_parser_takes_matmul_and_refuses_it_on_features():
    from tennis_amd import train_gnmt
    p = train_gnmt.build_parser()
    assert p.parse_args([]).matmul == "f32"
    assert p.parse_args(["--matmul", "fp32x3"]).matmul == "fp32x3"
    with pytest.raises(SystemExit):
        p.parse_args(["--matmul", "bf16"])
    with pytest.raises(SystemExit) as ei:
        train_gnmt.main(["--feats_model", "X", "--matmul", "fp32x3"])
    assert "--matmul fp32x3" in str(ei.value) and "no backbone" in str(ei.value)


@pytest.mark.parametrize("which", ["FrameModelTrainer", "CNNRNNTrainer", "GNMTFramesTrainer"])
def test_trainers_refuse_an_unknown_matmul_without_a_gpu(which):
    from tennis_amd import engine
    cls = getattr(engine, which)
    args = ({}, 8, 6, 14) if which == "GNMTFramesTrainer" else ({},)
    with pytest.raises(ValueError) as ei:
        cls(*args, matmul="bf16")
    assert "'f32'" in str(ei.value) and "'fp32x3'" in str(ei.value)
