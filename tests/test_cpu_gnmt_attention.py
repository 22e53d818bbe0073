"""The host side of the captioner's attention outputs (no GPU): the two entry points' declarations, the reference tool
tests/tools/gnmt_attention_ref.py against the oracle it is built on, the "a hypothesis' attention depends only on its token prefix"
argument that tests/test_gpu_gnmt_attention.py rests on, the alignment records and their ``.npz`` file, the driver's flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import gnmt_np as gn
from tools import gnmt_attention_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tn_gnmt_decode_seq_attention", "tn_gnmt_beam_search_attention"]


def test_symbols_declared_and_exported():
    from tennis_amd import _lib
    header = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    declared = _lib.declared_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in declared, name
        assert getattr(lib, name) is not None, name
    assert "gnmt.py:302-303,402-403" in header                                  # the reference call site the entries cite


def _setup(seed, cell, B=3, T=9, F=12, H=8, E=6, V=14, nl=2, nbi=1, proj_scale=1.0, eos_bias=0.0):
    from tennis_amd import weights as W
    p = W.make_gnmt_weights(seed, cell, F, H, E, V, num_layers=nl, num_bi_layers=nbi)
    p["gnmt_tgt_proj_weight"] = (p["gnmt_tgt_proj_weight"] * proj_scale).astype(np.float32)
    p["gnmt_tgt_proj_bias"][3] += eos_bias
    rng = np.random.default_rng(seed)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    svl = rng.integers(2, T + 1, B).astype(np.int32)
    svl[0], svl[1] = T, 1
    mem, states = gn.encoder(src, svl, p, cell, H, num_layers=nl, num_bi_layers=nbi)
    return p, mem, states, svl, rng


@pytest.mark.parametrize("cell,nl,nbi", [("gru", 2, 1), ("lstm", 2, 1), ("gru", 3, 1)])
def test_reference_tool_is_the_oracles_decoder(cell, nl, nbi):
    """the logits it passes through are ``oracle.gnmt_np.decode_seq``'s, bit for bit; its weights are distributions over the valid
    steps and agree with the float32 weights the oracle's own step forms"""
    p, mem, states, svl, rng = _setup(3, cell, nl=nl, nbi=nbi)
    tgt = rng.integers(0, 14, (3, 6)).astype(np.int32)
    want = gn.decode_seq(gn.Decoder(p, 8, num_layers=nl, cell=cell), mem, states, svl, tgt)
    logits, w = ar.teacher_forcing(ar.AttentionDecoder(p, 8, num_layers=nl, cell=cell), mem, states, svl, tgt)
    assert np.array_equal(logits, want)
    assert w.shape == (3, 6, 9) and w.dtype == np.float64
    assert np.abs(w.sum(axis=-1) - 1.0).max() < 1e-12
    for b, n in enumerate(svl):
        assert (w[b, :, n:] == 0.0).all()
    assert (w[1, :, 0] == 1.0).all()                                             # the clip of one valid step
    # ctx = weights . mem: the oracle's float32 context is what the float64 weights give, to float32 rounding
    dec = ar.AttentionDecoder(p, 8, num_layers=nl, cell=cell)
    rnn_states, att = dec.init_state(mem, states, svl)
    _, _, ctx = dec.step(tgt[:, 0], rnn_states, att, np.arange(3))
    assert np.abs(np.einsum("rt,rth->rh", dec.last_weights, mem.astype(np.float64)) - ctx).max() < 1e-5


@pytest.mark.parametrize("cell,kw", [("gru", dict(proj_scale=30.0)), ("lstm", dict(proj_scale=30.0)), ("gru", dict(eos_bias=1.5)),
                                     ("gru", dict())])
def test_a_hypothesis_attention_depends_only_on_its_token_prefix(cell, kw):
    """A small beam search of the oracle, recorded: teacher forcing each returned hypothesis reproduces the oracle's own per-step
    weights along that hypothesis' ancestry.  Both sides are the same float64 formula on float32 first-layer states that come
    out of the same cells on the same inputs, in batches of different composition: 1e-6 covers a BLAS that rounds a row's
    products differently by batch shape (a few float32 ulps of the state, times |keys| ~ 1)."""
    beam, ml = 3, 10
    p, mem, states, svl, _ = _setup(7, cell, **kw)
    dec = ar.AttentionDecoder(p, 8, cell=cell, record=True)
    s, _, v = gn.beam_search(dec, mem, states, svl, 2, 3, beam, 1.0, 5, ml)
    own = ar.ancestry_weights(dec, s, v, beam, ml)
    tf, nrow = ar.hypothesis_alignments(ar.AttentionDecoder(p, 8, cell=cell), mem, states, svl, s, v, ml)
    assert tf.shape == (3, beam, s.shape[2] - 1, 9)
    seen = 0
    for (b, k), w in own.items():
        n = int(nrow[b, k])
        assert w.shape == (n, 9) and n >= 1
        assert np.abs(tf[b, k, :n] - w).max() < 1e-6, (b, k)
        assert (tf[b, k, n:] == 0.0).all()
        seen += n
    assert seen > 3 * beam                                                        # hypotheses of more than one step were walked
    if kw.get("eos_bias"):
        assert s.shape[2] < ml + 2                                                # every beam finished: the early exit
    else:
        assert (v == ml + 2).any() and (nrow[v == ml + 2] == ml).all()            # alive at max_length: the appended <eos> has no row


def test_alignment_records_and_npz_round_trip(tmp_path):
    from tennis_amd import captions as cp
    rng = np.random.default_rng(0)
    att = rng.random((11, 7)).astype(np.float32)                                  # a best beam's (L - 1, T) rows
    i, w = cp.alignment_record(np.int64(4), att, sample_valid_length=6, src_valid_length=np.float32(5.0))
    assert i == 4 and isinstance(i, int) and w.shape == (4, 5) and w.dtype == np.float32       # <bos> w w w w <eos>: four words
    assert np.array_equal(w, att[:4, :5])
    assert cp.alignment_record(0, att, 2, 7.0)[1].shape == (0, 7)                 # <bos> <eos>: no word written out
    assert cp.alignment_record(0, att, 1, 7.0)[1].shape == (0, 7)
    assert cp.alignment_record(0, att, 13, 9.0)[1].shape == (11, 7)               # never beyond the tensor
    records = [(2, att[:3, :4].copy()), (0, att[:0, :6].copy()), (1, att[:5, :7].copy())]
    frames = {0: [("v0", f) for f in range(0, 12, 2)], 1: [("v1", 100 + f) for f in range(7)], 2: [("v0", f) for f in (3, 4, 5, 6)]}
    path = str(tmp_path / "best_test_alignments.npz")
    cp.save_alignments(path, records, frames)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"inst_ids", "words", "steps", "offsets", "weights", "word_offsets", "argmax", "frame_offsets",
                                "frame_videos", "frame_numbers"}
        assert all(z[k].ndim == 1 and z[k].dtype != object for k in z.files)      # flat arrays only
        assert z["inst_ids"].tolist() == [0, 1, 2] and z["words"].tolist() == [0, 5, 3] and z["steps"].tolist() == [6, 7, 4]
        assert z["offsets"].tolist() == [0, 0, 35, 47] and z["word_offsets"].tolist() == [0, 0, 5, 8]
        assert z["frame_offsets"].tolist() == [0, 6, 13, 17] and z["weights"].dtype == np.float32
    back = cp.load_alignments(path)
    assert [b[0] for b in back] == [0, 1, 2]
    for (i, w, am, fr), want in zip(back, (records[1], records[2], records[0])):
        assert w.shape == want[1].shape and np.array_equal(w, want[1]) and am.shape == (w.shape[0],)
        if w.size:
            assert np.array_equal(am, want[1].argmax(axis=1))
        assert fr == frames[i] and len(fr) == w.shape[1]
    cp.save_alignments(path, records)                                             # without frame identities
    assert cp.load_alignments(path)[1][3] is None
    cp.save_alignments(path, [])
    assert cp.load_alignments(path) == []


def test_clip_frame_ids_name_the_steps_as_the_clip_table_does():
    from tennis_amd import captions as cp
    ds = cp.CaptionSet(split="val", n_points=5, feature_dim=8, mean_frames=6, inference=True)
    ids = cp.clip_frame_ids(ds)
    frames, idx, lens = ds.clip_table()
    assert sorted(ids) == list(range(len(ds)))
    for i in range(len(ds)):
        assert ids[i] == ds.clip_frames(i) == [frames[r] for r in idx[i, :lens[i]]]


def test_driver_flag():
    from tennis_amd import evaluate_gnmt, train_gnmt
    p = evaluate_gnmt.build_parser()
    assert p.parse_args([]).save_alignments is False
    assert p.parse_args(["--save_alignments"]).save_alignments is True
    assert p.parse_args(["--save_alignments", "--feats_on_device"]).feats_on_device is True
    with pytest.raises(SystemExit):
        train_gnmt.build_parser().parse_args(["--save_alignments"])              # an evaluation flag


def test_output_attention_stays_an_attribute_and_says_where_the_weights_are():
    from tennis_amd.models.captioning.gnmt import GNMTDecoder
    assert GNMTDecoder(output_attention=True, prefix="dec_")._output_attention is True
    assert "return_attention" in GNMTDecoder.__doc__ and "alignments" in GNMTDecoder.__doc__
