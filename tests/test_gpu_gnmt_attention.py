"""-m gpu: the decoder's attention weights out of ``decode_seq`` and the beam search (``tn_gnmt_decode_seq_attention`` /
``tn_gnmt_beam_search_attention``, ``return_attention=True`` on ``GNMTCaptioner`` and ``BeamSearchTranslator``).

Reference: tests/tools/gnmt_attention_ref.py - the oracle's decoder with the step's distribution recomputed in float64.  The
beam-search alignments are compared with teacher forcing of the DEVICE's own hypotheses (a hypothesis' attention depends only on
its token prefix; tests/test_cpu_gnmt_attention.py pins that), so near ties between beams cannot matter and no beam is left out.
Bar: 1e-4 absolute, the project's bar for every captioner quantity against its oracle.  Rows sum to 1 within 1e-5 (summed in float64;
a handful of float32 ulps per weight does not reach that), positions at or beyond ``valid_length`` are exact zeros."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gnmt_np as gn
from tools import gnmt_attention_ref as ar

pytestmark = pytest.mark.gpu

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


# make_gnmt_weights' attention is nearly uniform: scores of 1e-3, the rows of two beams of a clip 1e-5 apart - below the bar, so a
# wrong ancestor row or a lost slice of the score's contraction would pass.  The beam-search cases (and one teacher-forcing case) scale
# the key weight: the weights then peak at 0.2 - 0.5 and two beams' rows differ by 1e-2 or so (more than ten times the bar, which the beam test asserts).
KEY_SCALE = 1000.0


def _weights(seed, cell, F, H, E, V, nl=2, nbi=1, proj_scale=1.0, eos_bias=0.0, key_scale=1.0):
    from tennis_amd import weights as W
    p = W.make_gnmt_weights(seed, cell, F, H, E, V, num_layers=nl, num_bi_layers=nbi)
    p["gnmt_dec_attention_key_weight"] = (p["gnmt_dec_attention_key_weight"] * key_scale).astype(np.float32)
    p["gnmt_tgt_proj_weight"] = (p["gnmt_tgt_proj_weight"] * proj_scale).astype(np.float32)
    p["gnmt_tgt_proj_bias"][3] += eos_bias
    return p


def _captioner(p, F, H, E, V, B, T, beam=2, max_length=12, cell="gru", nl=2, nbi=1, res=False):
    from tennis_amd.engine import GNMTCaptioner
    return GNMTCaptioner(p, F, H, E, V, beam=beam, max_length=max_length, max_batch=B, max_src_len=T, cell_type=cell, num_layers=nl,
                         num_bi_layers=nbi, use_residual=res)


def _check_rows(w, svl, rows_valid=None):
    """w (..., L, T) device weights of clips with valid lengths svl (leading axis): sums, exact zeros, the one-step clip"""
    w64 = w.astype(np.float64)
    for b, n in enumerate(svl):
        assert (w[b][..., n:] == 0.0).all(), b                                  # exact zeros at and beyond valid_length
        live = w64[b] if rows_valid is None else w64[b][rows_valid[b]]
        assert np.abs(live.sum(axis=-1) - 1.0).max() <= 1e-5, b
        if n == 1:
            assert (live[..., 0] == 1.0).all(), b


# ---- teacher forcing -------------------------------------------------------------------------------------------------------
TF_CASES = {
    "gru": dict(cell="gru", B=4, T=17, F=48, H=32, E=16, V=50, L=8),
    "lstm": dict(cell="lstm", B=4, T=17, F=48, H=32, E=16, V=50, L=8),
    "h24": dict(cell="gru", B=4, T=17, F=48, H=24, E=16, V=50, L=8),                       # hidden no multiple of 64
    "three_layers": dict(cell="gru", B=4, T=17, F=48, H=32, E=16, V=50, L=8, nl=3, nbi=1),
    "four_layers_residual": dict(cell="gru", B=4, T=17, F=48, H=32, E=16, V=50, L=8, nl=4, nbi=2, res=True),
    "t300": dict(cell="gru", B=4, T=300, F=48, H=32, E=16, V=50, L=8),                     # more than one pass per lane
    "t2500": dict(cell="gru", B=1, T=2500, F=16, H=32, E=16, V=50, L=8),                   # the lowered LDS split
    # T 300 again with scores of order 1: clips much shorter than a source of more than 256 steps (104 and 200 valid steps here) are
    # where the score phase's partial rows must fit the LDS the launch was given for T
    "t300_sharp": dict(cell="gru", B=4, T=300, F=48, H=32, E=16, V=50, L=8, key_scale=KEY_SCALE, seed=46),
}


def _tf_inputs(name):
    c = TF_CASES[name]
    seed = c.get("seed", sorted(TF_CASES).index(name) + 41)
    p = _weights(seed, c["cell"], c["F"], c["H"], c["E"], c["V"], c.get("nl", 2), c.get("nbi", 1), key_scale=c.get("key_scale", 1.0))
    rng = np.random.default_rng(seed)
    B, T = c["B"], c["T"]
    src = (np.abs(rng.normal(0, 1, (B, T, c["F"]))) * 0.5).astype(np.float32)
    svl = rng.integers(max(2, T // 3), T + 1, B).astype(np.int32)
    svl[0] = T
    if B > 1:
        svl[1] = 1                                                               # one clip of a single valid step
    tgt = rng.integers(4, c["V"], (B, c["L"])).astype(np.int32)
    return c, p, src, svl, tgt


@pytest.mark.parametrize("name", sorted(TF_CASES))
def test_teacher_forcing_weights_against_the_reference(name, report):
    c, p, src, svl, tgt = _tf_inputs(name)
    kw = dict(cell=c["cell"], nl=c.get("nl", 2), nbi=c.get("nbi", 1), res=c.get("res", False))
    cap = _captioner(p, c["F"], c["H"], c["E"], c["V"], c["B"], c["T"], **kw)
    cap.encode(dev(src), dev(svl))
    plain = cap.decode_seq(dev(tgt))
    logits, att = cap.decode_seq(dev(tgt), return_attention=True)
    assert torch.equal(plain, logits)                                            # off is off: bit-identical logits
    assert torch.equal(plain, cap.decode_seq(dev(tgt)))
    assert att.shape == (c["B"], c["L"], c["T"]) and att.dtype == torch.float32
    w = att.cpu().numpy()
    rmem, rstates = gn.encoder(src, svl, p, c["cell"], c["H"], num_layers=kw["nl"], num_bi_layers=kw["nbi"], use_residual=kw["res"])
    dec = ar.AttentionDecoder(p, c["H"], num_layers=kw["nl"], cell=c["cell"], use_residual=kw["res"])
    rl, rw = ar.teacher_forcing(dec, rmem, rstates, svl, tgt)
    err = float(np.abs(w - rw).max())
    report[f"gnmt_attention_tf_{name}_maxabs_err"] = err
    print(f"teacher forcing {name}: attention max|err| = {err:.3e}")
    assert err <= 1e-4, err
    assert np.abs(logits.cpu().numpy() - rl).max() < 1e-4
    _check_rows(w, svl)


# ---- beam search -----------------------------------------------------------------------------------------------------------
BEAM_CASES = {      # configurations of tests/test_gpu_captioner.py::test_beam_search_matches_oracle, one per path
    "to_max_length": dict(seed=1, B=3, T=11, F=24, H=16, E=12, V=30, beam=4, max_length=12),
    "early_exit": dict(seed=2, B=5, T=23, F=64, H=32, E=20, V=40, beam=4, max_length=40, eos_bias=1.2),
    "mixed": dict(seed=2, B=5, T=23, F=64, H=32, E=20, V=40, beam=4, max_length=40, proj_scale=40.0),
    "lstm": dict(seed=4, B=3, T=13, F=32, H=16, E=12, V=30, beam=4, max_length=14, cell="lstm"),
    "beam1": dict(seed=6, B=3, T=17, F=32, H=16, E=12, V=30, beam=1, max_length=16, proj_scale=30.0),
    "twelve_clips": dict(seed=17, B=12, T=21, F=32, H=32, E=16, V=40, beam=5, max_length=14, proj_scale=30.0),
    "three_layers": dict(seed=10, B=3, T=19, F=40, H=32, E=16, V=40, beam=4, max_length=24, proj_scale=30.0, nl=3, nbi=1),
    "three_layers_long": dict(seed=10, B=3, T=19, F=40, H=32, E=16, V=40, beam=4, max_length=24, nl=3, nbi=1),   # (the one above ends after two steps)
    "t300_beam7": dict(seed=8, B=2, T=300, F=48, H=32, E=16, V=300, beam=7, max_length=20, proj_scale=40.0),
}


def _beam_inputs(name):
    c = BEAM_CASES[name]
    p = _weights(c["seed"], c.get("cell", "gru"), c["F"], c["H"], c["E"], c["V"], c.get("nl", 2), c.get("nbi", 1),
                 c.get("proj_scale", 1.0), c.get("eos_bias", 0.0), KEY_SCALE)
    rng = np.random.default_rng(c["seed"])
    src = (np.abs(rng.normal(0, 1, (c["B"], c["T"], c["F"]))) * 0.5).astype(np.float32)
    svl = rng.integers(max(1, c["T"] // 3), c["T"] + 1, c["B"]).astype(np.int32)
    svl[0] = c["T"]
    return c, p, src, svl


def _check_beam(c, p, src, svl, samples, vlen, att, report=None, tag=None):
    """device alignments att (B, beam, n - 1, T) of the device's hypotheses against teacher forcing of those hypotheses"""
    cell, nl, nbi = c.get("cell", "gru"), c.get("nl", 2), c.get("nbi", 1)
    s, v, w = samples.cpu().numpy(), vlen.cpu().numpy(), att.cpu().numpy()
    B, beam, n = s.shape
    assert w.shape == (B, beam, n - 1, src.shape[1]) and w.dtype == np.float32
    rmem, rstates = gn.encoder(src, svl, p, cell, c["H"], num_layers=nl, num_bi_layers=nbi)
    dec = ar.AttentionDecoder(p, c["H"], num_layers=nl, cell=cell)
    rw, nrow = ar.hypothesis_alignments(dec, rmem, rstates, svl, s, v, c["max_length"])
    emitted = np.arange(n - 1)[None, None, :] < nrow[:, :, None]
    assert (w[~emitted] == 0.0).all()                                 # no decoder step emitted these tokens: exact zeros
    assert (w[np.arange(n - 1)[None, None, :] >= (v - 1)[:, :, None]] == 0.0).all()      # rows at or behind vlen - 1
    err = float(np.abs(w - rw).max())
    # what a wrong ancestor row would cost: the largest distance between the rows two hypotheses of a clip have at the same step
    tell = 0.0
    for k in range(beam):
        for k2 in range(k + 1, beam):
            both = emitted[:, k] & emitted[:, k2]
            if both.any():
                tell = max(tell, float(np.abs(rw[:, k] - rw[:, k2]).max(axis=-1)[both].max()))
    if report is not None:
        report[f"gnmt_attention_beam_{tag}_maxabs_err"] = err
    print(f"beam search {tag}: attention max|err| = {err:.3e}, rows per hypothesis {nrow.min()}..{nrow.max()} of {n - 1}, "
          f"two beams' rows up to {tell:.2e} apart")
    assert err <= 1e-4, err
    _check_rows(w, svl, emitted)
    return nrow, tell


@pytest.mark.parametrize("name", sorted(BEAM_CASES))
def test_beam_search_alignments_against_the_reference(name, report):
    c, p, src, svl = _beam_inputs(name)
    cap = _captioner(p, c["F"], c["H"], c["E"], c["V"], c["B"], c["T"], c["beam"], c["max_length"], c.get("cell", "gru"),
                     c.get("nl", 2), c.get("nbi", 1))
    cap.encode(dev(src), dev(svl))
    samples, scores, vlen, att = cap.beam_search(2, 3, 1.0, 5.0, return_attention=True)
    nrow, tell = _check_beam(c, p, src, svl, samples, vlen, att, report, name)
    if c["beam"] > 1 and name not in ("early_exit", "three_layers"):             # (those two end after one or two steps)
        assert tell > 1e-3, tell                                                 # ten times the bar and more: a wrong row cannot pass
    v, n, ml = vlen.cpu().numpy(), samples.shape[2], c["max_length"]
    # the cases reach the paths their names say
    if name == "to_max_length":
        assert n == ml + 2 and (v == ml + 2).any() and (nrow[v == ml + 2] == ml).all()      # the appended <eos> has no row
    if name == "early_exit":
        assert n < ml + 2 and (nrow == v - 1).all()
    if name == "mixed":
        assert n == ml + 2 and (v < ml + 1).any() and (v == ml + 2).any()                 # finished (-1 carried) and live beams


def test_off_is_off():
    """samples, scores and lengths do not depend on whether the weights were asked for, before or after, on one handle"""
    c, p, src, svl = _beam_inputs("mixed")
    mk = lambda: _captioner(p, c["F"], c["H"], c["E"], c["V"], c["B"], c["T"], c["beam"], c["max_length"])
    never, cap = mk(), mk()
    never.encode(dev(src), dev(svl))
    cap.encode(dev(src), dev(svl))
    want = never.beam_search(2, 3, 1.0, 5.0)
    runs = [cap.beam_search(2, 3, 1.0, 5.0), cap.beam_search(2, 3, 1.0, 5.0, return_attention=True), cap.beam_search(2, 3, 1.0, 5.0)]
    assert len(runs[0]) == 3 and len(runs[1]) == 4 and len(runs[2]) == 3
    for r in runs:
        for a, b in zip(want, r):
            assert a.shape == b.shape and torch.equal(a, b)
    first = mk()                                                                  # asked on the handle's very first search
    first.encode(dev(src), dev(svl))
    on = first.beam_search(2, 3, 1.0, 5.0, return_attention=True)
    assert torch.equal(on[3], runs[1][3])
    for a, b in zip(want, first.beam_search(2, 3, 1.0, 5.0)):
        assert torch.equal(a, b)


def test_encode_rows_route_is_bit_identical():
    c, p, src, svl = _beam_inputs("mixed")
    B, T, F = c["B"], c["T"], c["F"]
    rng = np.random.default_rng(3)
    table = np.full((B * T + 7, F + 5), 9.0, np.float32)                          # rows nobody names, a row stride beyond F
    idx = np.full((B, T), -1, np.int32)
    slots = rng.permutation(B * T + 7)
    k = 0
    for b in range(B):
        for t in range(int(svl[b])):
            idx[b, t] = slots[k]
            table[slots[k], :F] = src[b, t]
            k += 1
    padded = np.where((idx >= 0)[..., None], src, np.float32(0))                   # what the table route sees behind a clip's end
    assert (idx < 0).any()
    a, b_ = (_captioner(p, F, c["H"], c["E"], c["V"], B, T, c["beam"], c["max_length"]) for _ in range(2))
    a.encode(dev(padded), dev(svl))
    b_.encode_rows(dev(table)[:, :F], dev(idx), dev(svl))
    for x, y in zip(a.beam_search(2, 3, 1.0, 5.0, return_attention=True), b_.beam_search(2, 3, 1.0, 5.0, return_attention=True)):
        assert x.shape == y.shape and torch.equal(x, y)
    tgt = dev(rng.integers(4, c["V"], (B, 6)).astype(np.int32))
    for x, y in zip(a.decode_seq(tgt, return_attention=True), b_.decode_seq(tgt, return_attention=True)):
        assert torch.equal(x, y)


def test_translator_passes_the_weights_through():
    from tennis_amd.models.captioning.gnmt import NMTModel, Vocab, get_gnmt_encoder_decoder
    from tennis_amd.utils.translation import BeamSearchScorer, BeamSearchTranslator
    words = "the player serves near far left right a forehand backhand return in out".split()
    vocab = Vocab({w: i + 1 for i, w in enumerate(words)})
    enc, dec = get_gnmt_encoder_decoder(cell_type="gru", hidden_size=32, num_layers=2, num_bi_layers=1)
    model = NMTModel(src_vocab=None, tgt_vocab=vocab, encoder=enc, decoder=dec, embed_size=12, prefix="gnmt_", input_size=48)
    model.initialize()
    tr = BeamSearchTranslator(model=model, beam_size=4, scorer=BeamSearchScorer(alpha=1.0, K=5), max_length=20)
    src = np.abs(np.random.default_rng(0).normal(0, 1, (3, 9, 48))).astype(np.float32)
    svl = np.array([9, 5, 7], np.float32)
    plain = tr.translate(src, svl)
    out = tr.translate(src, svl, return_attention=True)
    assert len(plain) == 3 and len(out) == 4
    for a, b in zip(plain, out):
        assert torch.equal(a, b)
    cap = model._captioner(4, 20, 3, 9)
    cap.encode(dev(src), dev(svl))
    want = cap.beam_search(2, 3, 1.0, 5.0, 20, return_attention=True)
    assert out[3].shape == (3, 4, out[0].shape[2] - 1, 9) and torch.equal(out[3], want[3])
    rows = tr.translate_rows(dev(src.reshape(27, 48)), np.where(np.arange(9)[None] < svl[:, None], np.arange(27).reshape(3, 9), -1),
                             svl, return_attention=True)
    assert len(rows) == 4 and rows[3].shape == out[3].shape


def test_translator_frame_mode_weights_are_over_the_frames():
    """the tiny frame-mode setup of tests/test_gpu_captioner.py::test_frame_mode_source_embedding: with a ``src_embed`` the encoder
    steps are the clip's frames, and the weights equal those of the feature-mode model fed the backbone's features"""
    from tennis_amd import weights as W
    from tennis_amd.model_zoo import get_model
    from tennis_amd.models.captioning.gnmt import NMTModel, Vocab, get_gnmt_encoder_decoder
    from tennis_amd.models.vision.definitions import FrameModel
    from tennis_amd.utils.layers import TimeDistributed
    from tennis_amd.utils.translation import BeamSearchScorer, BeamSearchTranslator
    vocab = Vocab({f"w{i}": 30 - i for i in range(26)})
    cnn_model = FrameModel(get_model("DenseNet121", pretrained=True, seed=0).features, 11)
    mk = lambda se: NMTModel(src_vocab=None, tgt_vocab=vocab, encoder=get_gnmt_encoder_decoder(cell_type="gru", hidden_size=32)[0],
                             decoder=get_gnmt_encoder_decoder(cell_type="gru", hidden_size=32)[1], embed_size=16, prefix="gnmt_",
                             src_embed=se, input_size=1024, seed=5)
    frame_model, feat_model = mk(TimeDistributed(cnn_model.backbone)), mk(None)
    frame_model.initialize(); feat_model.initialize()
    B, T = 2, 5
    frames = torch.from_numpy(W.synthetic_frames_u8(B * T, 224).reshape(B, T, 224, 224, 3)).cuda()
    vl = np.array([5, 3], np.float32)
    feats = cnn_model.backbone(frames.reshape(B * T, 224, 224, 3)).reshape(B, T, 1024)
    out = []
    for m, src in ((frame_model, frames), (feat_model, feats)):
        tr = BeamSearchTranslator(model=m, beam_size=3, scorer=BeamSearchScorer(alpha=1.0, K=5), max_length=10)
        out.append(tr.translate(src, vl, return_attention=True))
    assert len(out[0]) == 4 and out[0][3].shape == (B, 3, out[0][0].shape[2] - 1, T)
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert (out[0][3][1, :, :, 3:] == 0).all() and float(out[0][3][1, 0, 0].sum()) == pytest.approx(1.0, abs=1e-5)


def test_second_batch_on_one_handle_follows_the_call_not_the_capacity(report):
    """a shorter T and a smaller B after the first batch: the history's strides are the call's"""
    c, p, src, svl = _beam_inputs("mixed")
    cap = _captioner(p, c["F"], c["H"], c["E"], c["V"], c["B"], c["T"], c["beam"], c["max_length"])
    cap.encode(dev(src), dev(svl))
    s, _, v, att = cap.beam_search(2, 3, 1.0, 5.0, return_attention=True)
    _check_beam(c, p, src, svl, s, v, att, report, "first_batch")
    src2, svl2 = np.ascontiguousarray(src[1:3, :14]), np.minimum(svl[1:3], 14).astype(np.int32)
    svl2[0] = 14
    cap.encode(dev(src2), dev(svl2))
    s2, _, v2, att2 = cap.beam_search(2, 3, 1.0, 5.0, return_attention=True)
    assert att2.shape[0] == 2 and att2.shape[3] == 14
    _check_beam(c, p, src2, svl2, s2, v2, att2, report, "second_batch")
    tgt = np.random.default_rng(5).integers(4, c["V"], (2, 5)).astype(np.int32)
    w = cap.decode_seq(dev(tgt), return_attention=True)[1].cpu().numpy()
    rmem, rstates = gn.encoder(src2, svl2, p, "gru", c["H"])
    rw = ar.teacher_forcing(ar.AttentionDecoder(p, c["H"]), rmem, rstates, svl2, tgt)[1]
    assert w.shape == (2, 5, 14) and np.abs(w - rw).max() <= 1e-4


def test_abi_errors():
    from tennis_amd import _lib
    c, p, src, svl = _beam_inputs("to_max_length")
    cap = _captioner(p, c["F"], c["H"], c["E"], c["V"], c["B"], c["T"], c["beam"], c["max_length"])
    lib, ptr = cap.lib, _lib.ptr
    R, L, T = c["B"] * c["beam"], c["max_length"] + 2, c["T"]
    samples = torch.empty((R, L), dtype=torch.int32, device="cuda")
    scores = torch.empty(R, dtype=torch.float32, device="cuda")
    vlen = torch.empty(R, dtype=torch.int32, device="cuda")
    att = torch.zeros((R, L - 1, T), dtype=torch.float32, device="cuda")
    tgt = dev(np.full((c["B"], 4), 5, np.int32))
    logits = torch.empty((c["B"], 4, c["V"]), dtype=torch.float32, device="cuda")
    watt = torch.zeros((c["B"], 4, T), dtype=torch.float32, device="cuda")
    n = C.c_int(0)
    invalid = -1                                                                   # TN_ERR_INVALID (include/tennis_hip.h)
    beam = lambda a: lib.tn_gnmt_beam_search_attention(cap.handle, 2, 3, 1.0, 5.0, c["max_length"], ptr(samples), ptr(scores), ptr(vlen),
                                                       C.byref(n), a)
    tf = lambda a: lib.tn_gnmt_decode_seq_attention(cap.handle, ptr(tgt), 4, 4, ptr(logits), a)
    # before any encode
    assert beam(ptr(att)) == invalid and b"tn_gnmt_encode first" in lib.tn_last_error()
    assert tf(ptr(watt)) == invalid and b"tn_gnmt_encode first" in lib.tn_last_error()
    cap.encode(dev(src), dev(svl))
    # a null attention
    assert beam(None) == invalid and b"tn_gnmt_beam_search_attention: null" in lib.tn_last_error()
    assert tf(None) == invalid and b"tn_gnmt_decode_seq_attention: null" in lib.tn_last_error()
    assert beam(ptr(att)) == 0 and tf(ptr(watt)) == 0
    torch.cuda.synchronize()
    assert float(att.sum()) > 0 and float(watt.sum()) == pytest.approx(c["B"] * 4, abs=1e-3)


def test_evaluate_collects_alignment_records_on_both_routes(tmp_path):
    """``captions.evaluate(alignments=[])`` on the loader route and from a device-resident table: the return value is unchanged, one
    record per instance - the best beam's rows for the words written out, over the clip's valid steps -, and the ``.npz`` names each
    step's frame as ``clip_frames`` does"""
    from tennis_amd import captions as cp
    from tennis_amd.captions import CaptionSet
    from tennis_amd.models.captioning.gnmt import NMTModel, get_gnmt_encoder_decoder
    from tennis_amd.utils.translation import BeamSearchScorer, BeamSearchTranslator
    tr_set = CaptionSet(split="train", n_points=6, feature_dim=24, mean_frames=8)
    va_set = CaptionSet(split="val", n_points=7, feature_dim=24, mean_frames=8, vocab=tr_set.vocab, inference=True)
    enc, dec = get_gnmt_encoder_decoder(cell_type="gru", hidden_size=16)
    model = NMTModel(src_vocab=None, tgt_vocab=tr_set.vocab, encoder=enc, decoder=dec, embed_size=8, prefix="gnmt_", input_size=24)
    model.initialize()
    translator = BeamSearchTranslator(model=model, beam_size=3, scorer=BeamSearchScorer(alpha=1.0, K=5), max_length=10)
    table, rows = cp.upload_clip_table(va_set)
    want = cp.evaluate(cp.bucketed_batches(va_set, 3, 2), model, translator, tr_set)
    rec, rec_rows = [], []
    got = cp.evaluate(cp.bucketed_batches(va_set, 3, 2), model, translator, tr_set, alignments=rec)
    got_rows = cp.evaluate(cp.bucketed_batches(va_set, 3, 2, rows=rows), model, translator, tr_set, table=table, alignments=rec_rows)
    assert got[0] == want[0] and got[1] == want[1] and got_rows[0] == want[0] and got_rows[1] == want[1]
    lens = va_set.get_clip_lens()
    assert sorted(i for i, _ in rec) == list(range(len(va_set))) and [i for i, _ in rec] == [i for i, _ in rec_rows]
    for (i, w), (_, w2) in zip(rec, rec_rows):
        assert w.shape == (len(want[1][i]), lens[i]) and w.dtype == np.float32 and np.array_equal(w, w2)
        if w.size:
            assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
    assert sum(w.shape[0] for _, w in rec) > 0                                    # some words were written out
    path = str(tmp_path / "best_valid_alignments.npz")
    cp.save_alignments(path, rec, cp.clip_frame_ids(va_set))
    back = cp.load_alignments(path)
    by_id = dict(rec)
    for i, w, am, fr in back:
        assert np.array_equal(w, by_id[i]) and fr == [(v, int(f)) for v, f in va_set.clip_frames(i)]
        if w.size:
            assert np.array_equal(am, w.argmax(axis=1))


def test_evaluate_gnmt_save_alignments_on_both_routes(tmp_path):
    """``evaluate_gnmt --save_alignments`` on a small on-disk tree after one training epoch: ``best_{valid,test}_alignments.npz`` beside
    the sentences, one record per point with a row per written word, the same file contents with ``--feats_on_device``, and the
    results the driver returns without the flag"""
    import os
    from tennis_amd import captions as cp, evaluate_gnmt as eg, train_gnmt as tg
    from tools import clip_tree
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    clip_tree.write(root, feature_dim=20)
    common = ["--data_root", root, "--feats_model", "0042", "--root", exp, "--num_hidden", "16", "--emb_size", "8", "--emb_file", "",
              "--tgt_max_len", "12", "--beam_size", "2", "--test_batch_size", "2", "--num_buckets", "2", "--model_id", "m"]
    assert tg.main(common + ["--epochs", "1", "--batch_size", "4", "--dropout", "0.0", "--lr", "0.01"]) == 0
    d = os.path.join(exp, "m")
    plain = eg.main(common)
    assert not [f for f in os.listdir(d) if f.endswith(".npz")]                   # nothing is written unless asked
    got = {}
    for route, extra in (("loader", []), ("table", ["--feats_on_device"])):
        assert eg.main(common + ["--save_alignments"] + extra) == plain
        got[route] = {s: cp.load_alignments(os.path.join(d, f"best_{s}_alignments.npz")) for s in ("valid", "test")}
        for s in ("valid", "test"):
            sents = open(os.path.join(d, f"best_{s}_out.txt")).read().split("\n")[:-1]
            assert [r[0] for r in got[route][s]] == list(range(len(sents)))
            for (i, w, am, fr), line in zip(got[route][s], sents):
                assert w.shape == (len(line.split()), len(fr)) and len(fr) >= 1 and am.shape == (w.shape[0],)
                if w.size:
                    assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
    for s in ("valid", "test"):
        for a, b in zip(got["loader"][s], got["table"][s]):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
