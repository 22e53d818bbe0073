"""The parameter tables of the training handles (csrc/param_table.h: what tn_head_create, tn_gnmt_trainer_create_ex and ft_create
load by and what every *_read_param reads through) asked through tn_dbg_trainer_params, which touches no device: the names are the
keys of the weight makers, the counts their sizes, the flat offsets contiguous from 0 to the handle's numel, and the order the one the
flat parameter / gradient buffers have had since each handle was written - generated here, not read back.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tennis_amd import _lib, weights as W

F_HEAD, H_HEAD, CLASSES = 32, 16, 11
F_CAP, H_CAP, E_CAP, V_CAP = 16, 8, 6, 12
GATES = {"gru": 3, "lstm": 4}
BLOCKS = (6, 12, 24, 16)


def head_order(rnn, dense):
    return ([f"{rnn}{d}0_{k}" for k in ("i2h_weight", "i2h_bias", "h2h_weight", "h2h_bias") for d in "lr"]
            + [dense + "weight", dense + "bias"])


def gnmt_order(pre, layers, bi):
    kinds = ("i2h_weight", "i2h_bias", "h2h_weight", "h2h_bias")
    out = []
    for i in range(layers):
        dirs = ("_l_", "_r_") if i < bi else ("_",)
        out += [f"{pre}enc_rnn{i}{d}{k}" for k in kinds for d in dirs]
    for j in range(layers):
        out += [f"{pre}dec_rnn{j}_{k}" for k in kinds]
    return out + [pre + n for n in ("dec_attention_key_weight", "tgt_proj_weight", "tgt_proj_bias", "tgt_embed_weight")]


def backbone_order(pre, dense):
    """-> (flat names, state names)"""
    flat, state = [], []

    def bn(name):
        flat.extend([name + "_gamma", name + "_beta"])
        state.extend([name + "_running_mean", name + "_running_var"])
    flat.append(pre + "conv0_weight")
    bn(pre + "batchnorm0")
    outer = 1
    for b, layers in enumerate(BLOCKS):
        sp = f"{pre}stage{b + 1}_"
        for l in range(layers):
            bn(f"{sp}batchnorm{2 * l}")
            flat.append(f"{sp}conv{2 * l}_weight")
            bn(f"{sp}batchnorm{2 * l + 1}")
            flat.append(f"{sp}conv{2 * l + 1}_weight")
        if b < 3:
            bn(f"{pre}batchnorm{outer}")
            flat.append(f"{pre}conv{outer}_weight")
            outer += 1
    bn(f"{pre}batchnorm{outer}")
    if dense:
        flat += [dense + "weight", dense + "bias"]
    return flat, state


def check_table(rows, numel, state_numel, params, flat_order, state_order=()):
    """rows [(name, where, offset, count)] against the weight maker's dict and the expected order of both buffers"""
    hooks = [r for r in rows if r[1] == _lib.PARAM_PTR]
    flat = [r for r in rows if r[1] == _lib.PARAM_FLAT]
    state = [r for r in rows if r[1] == _lib.PARAM_STATE]
    assert len(flat) + len(state) + len(hooks) == len(rows)
    assert len({r[0] for r in rows}) == len(rows)                                  # no name twice
    assert {r[0] for r in flat} | {r[0] for r in state} == set(params)
    assert {r[0] for r in state} == {k for k in params if "_running_" in k}
    for name, _, _, count in flat + state:
        assert count == int(np.prod(params[name].shape)), name
    for part, total, order in ((flat, numel, flat_order), (state, state_numel, state_order)):
        assert [r[0] for r in part] == list(order)
        end = 0
        for name, _, off, count in part:                                           # contiguous from 0, nothing overlaps
            assert off == end, name
            end += count
        assert end == total
    return hooks


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_head_table(kind):
    rnn, dense = f"cnnrnn0_{kind}0_", "cnnrnn0_dense0_"
    p = W.make_rnn_weights(1, kind, F_HEAD, H_HEAD, rnn)
    p.update(W.make_dense_weights(2, CLASSES, 2 * H_HEAD, dense))
    rows, n, ns = _lib.trainer_params(_lib.TRAINER_HEAD, (GATES[kind], F_HEAD, H_HEAD, CLASSES), rnn, dense)
    assert check_table(rows, n, ns, p, head_order(rnn, dense)) == [] and ns == 0


@pytest.mark.parametrize("layers, bi", [(2, 1), (3, 1)])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_captioner_table(kind, layers, bi):
    """(3, 1): the third encoder layer has the direction-less enc_rnn2_ names"""
    p = W.make_gnmt_weights(0, kind, F_CAP, H_CAP, E_CAP, V_CAP, layers, bi)
    rows, n, ns = _lib.trainer_params(_lib.TRAINER_GNMT, (GATES[kind], F_CAP, H_CAP, E_CAP, V_CAP, layers, bi), "gnmt_")
    assert check_table(rows, n, ns, p, gnmt_order("gnmt_", layers, bi)) == [] and ns == 0
    if layers == 3:
        assert "gnmt_enc_rnn2_i2h_weight" in {r[0] for r in rows}


@pytest.fixture(scope="module")
def backbone_weights():
    return W.make_densenet121_weights(0, fp16_model=False)


@pytest.mark.parametrize("classes", [0, CLASSES])
def test_backbone_table(backbone_weights, classes):
    """trainable names in the flat buffers, the running statistics in the state buffer in the same walk; the batch-statistic
    hooks are the only rows with a buffer of their own, two per BatchNorm"""
    dense = "framemodel0_dense0_" if classes else None
    p = dict(backbone_weights)
    if classes:
        p.update(W.make_dense_weights(1, classes, 1024, dense))
    rows, n, ns = _lib.trainer_params(_lib.TRAINER_BACKBONE, (classes,), "densenet0_", dense)
    flat, state = backbone_order("densenet0_", dense)
    hooks = check_table(rows, n, ns, p, flat, state)
    assert [r[0] for r in hooks] == [s.replace("_running_", "_batch_") for s in state]
    assert all(off == 0 and count == p[name.replace("_batch_", "_running_")].size for name, _, off, count in hooks)


def test_refusals():
    lib = _lib.load()
    n = C.c_int()
    dims = (C.c_int * 7)(3, 16, 8, 6, 12, 2, 2)
    assert lib.tn_dbg_trainer_params(_lib.TRAINER_GNMT, dims, 7, b"gnmt_", None, None, 0, C.byref(n), None, None) != 0   # bi == layers
    assert lib.tn_dbg_trainer_params(_lib.TRAINER_HEAD, dims, 4, b"a_", None, None, 0, C.byref(n), None, None) != 0       # one prefix
    assert lib.tn_dbg_trainer_params(_lib.TRAINER_BACKBONE, dims, 1, b"d_", None, None, 0, C.byref(n), None, None) != 0   # classes, no prefix
    assert lib.tn_dbg_trainer_params(3, dims, 1, b"d_", None, None, 0, C.byref(n), None, None) != 0
    assert lib.tn_dbg_trainer_params(_lib.TRAINER_HEAD, dims, 4, b"a_", b"b_", None, 0, None, None, None) != 0
    assert lib.tn_dbg_trainer_params(_lib.TRAINER_HEAD, dims, 4, b"x" * 90, b"b_", (_lib.TnParamRow * 10)(), 10, C.byref(n), None, None) != 0
