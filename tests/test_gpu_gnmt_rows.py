"""-m gpu: the captioner trained and evaluated from a device-resident feature table (``GNMTTrainer.forward_backward_rows``,
``GNMTCaptioner.encode_rows``, ``BeamSearchTranslator.translate_rows``; ``tn_gnmt_trainer_forward_backward_rows`` /
``tn_gnmt_encode_rows``).  The clips of a batch are ragged: a batch is padded to its longest clip, a pad step is index -1 and stands
for the row of zeros the materialised batch holds there.  The gathered step against the same step on the host-materialised
zero-padded batch - bit for bit, because the gathered kernels keep the dispatch rule, the k-loop and the MFMA order -, against the
float64 oracle (oracle/gnmt_train_torch.py) at the bars of tests/test_gpu_gnmt_train.py, the calls' contract, and the drivers
(``train_gnmt`` / ``evaluate_gnmt --feats_on_device``) against the loader route.

Shapes by launch_linear_f32's rule, ceil(N / 64) * ceil(M / 64) >= 512 with M = B * T and N = dirs * gates * H:
  skinny (32 x 32 tiles): B 3, T 70, lengths [70, 2, 33] - clip 1 holds rows 70 .. 139 of which 72 .. 139 are pad: the M-tile at rows
    96 .. 127 is all pad, the tiles either side are mixed (and so is the last, partial tile: rows 192 .. 209 are clip 2's padding);
    F 50 in a table of row stride 52: scalar staging.
  64 x 64, LSTM, H 256 (N = 2048, 32 tiles): B 16, T 64 (16 M-tiles; every clip is one tile, so none is all pad: mixed tiles with
    lengths 1, 5, 64) and B 8, T 128 (16 M-tiles; clip 1 of 5 frames holds rows 128 .. 255: the tile at rows 192 .. 255 is all pad).
  64 x 64, GRU, H 256 (N = 1536, 24 tiles): B 16, T 88 (22 M-tiles, 528 in all); clip 2 of 5 frames holds rows 176 .. 263, pad from
    181 on: the tile at rows 192 .. 255 is all pad.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import gnmt_train_torch as gt

pytestmark = pytest.mark.gpu

E, V, L = 8, 20, 6
LR = 1e-3
SKINNY = dict(B=3, T=70, F=50, ld=52, H=8, lens=(70, 2, 33), R=301)
CASES = {
    "skinny_gru": dict(SKINNY, cell="gru"),
    "skinny_lstm": dict(SKINNY, cell="lstm"),
    "big_lstm_T64": dict(B=16, T=64, F=64, ld=64, H=256, cell="lstm", lens=(64, 5, 1, 33, 64, 17, 2, 63, 64, 40, 1, 5, 64, 9, 30, 64), R=1501),
    "big_lstm_T128": dict(B=8, T=128, F=64, ld=64, H=256, cell="lstm", lens=(128, 5, 1, 64, 100, 127, 65, 128), R=1501),
    "big_gru_T88": dict(B=16, T=88, F=64, ld=64, H=256, cell="gru", lens=(88, 1, 5, 64, 88, 17, 2, 87, 88, 40, 1, 5, 64, 9, 30, 88), R=1501),
    # three layers, residual connections, no bidirectional layer (layer 0's N = gates * H), dropout 0.2 with one seed on both handles
    "three_layers": dict(SKINNY, cell="gru", nl=3, nbi=0, res=True, drop=0.2),
}
ORACLE = ["skinny_gru", "skinny_lstm", "three_layers", "big_gru_T88"]      # float64 autograd on the CPU: about a second at the most


def _pad_tiles(c):
    """(tile rows, number of M-tiles whose rows are all pad) of the case's layer-0 i2h product"""
    M, N = c["B"] * c["T"], (1 if c.get("nbi", 1) == 0 else 2) * (3 if c["cell"] == "gru" else 4) * c["H"]
    tile = 64 if -(-N // 64) * -(-M // 64) >= 512 else 32
    pad = np.concatenate([np.arange(c["T"]) >= n for n in c["lens"]])
    return tile, sum(bool(pad[m:m + tile].all()) for m in range(0, M, tile))


def test_the_cases_take_the_paths_their_names_say():
    assert _pad_tiles(CASES["skinny_gru"]) == (32, 2) and _pad_tiles(CASES["skinny_lstm"]) == (32, 2)
    assert _pad_tiles(CASES["three_layers"]) == (32, 2)
    assert _pad_tiles(CASES["big_lstm_T64"]) == (64, 0)
    assert _pad_tiles(CASES["big_lstm_T128"])[0] == 64 and _pad_tiles(CASES["big_lstm_T128"])[1] >= 1
    assert _pad_tiles(CASES["big_gru_T88"])[0] == 64 and _pad_tiles(CASES["big_gru_T88"])[1] >= 1
    for c in CASES.values():
        assert {1, 5, c["T"]} <= set(c["lens"]) or c["H"] == 8


def _inputs(name):
    from tennis_amd import weights as W
    c = CASES[name]
    B, T, F, H, R = c["B"], c["T"], c["F"], c["H"], c["R"]
    seed = sorted(CASES).index(name) + 21
    p = W.make_gnmt_weights(seed, c["cell"], F, H, E, V, num_layers=c.get("nl", 2), num_bi_layers=c.get("nbi", 1))
    rng = np.random.default_rng(seed)
    p["gnmt_tgt_embed_weight"] = rng.normal(0, 0.5, (V, E)).astype(np.float32)
    wide = (np.abs(rng.normal(0, 1, (R, c["ld"]))) * 0.5).astype(np.float32)        # the table is its first F columns
    svl = np.array(c["lens"], np.int32)
    idx = np.full((B, T), -1, np.int32)
    for b in range(B):
        idx[b, :svl[b]] = rng.integers(0, R - 40, svl[b])                           # the table's last 40 rows: nobody's
    idx[0, 0], idx[0, 1] = 0, R - 41
    idx[0, 2:6] = idx[0, 6]                                                         # one row at neighbouring steps
    idx[-1, :svl[-1]] = idx[0, :svl[-1]]                                            # a clip's start twice
    assert len(np.unique(idx[idx >= 0])) < (idx >= 0).sum() and idx.max() < R - 40
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0] = 2
    tvl = rng.integers(3, L + 1, B).astype(np.int32)
    tvl[0] = L
    for b in range(B):
        tgt[b, tvl[b] - 1] = 3
        tgt[b, tvl[b]:] = 1
    src = np.where((idx >= 0)[..., None], wide[:, :F][np.maximum(idx, 0)], np.float32(0))       # the host-materialised zero-padded batch
    return c, p, wide, idx, svl, tgt, tvl, np.ascontiguousarray(src, dtype=np.float32)


def _trainer(c, p):
    from tennis_amd.engine import GNMTTrainer
    tr = GNMTTrainer(p, c["F"], c["H"], E, V, max_batch=c["B"], max_src_len=c["T"], max_tgt_len=L, cell_type=c["cell"],
                     num_layers=c.get("nl", 2), num_bi_layers=c.get("nbi", 1), use_residual=c.get("res", False))
    if c.get("drop"):
        tr.set_dropout(c["drop"], seed=5)
    return tr


@functools.lru_cache(maxsize=None)
def _run(name):
    """Both steps, once per case: the materialised one and the gathered one (a device idx), one Adam update of each."""
    c, p, wide, idx, svl, tgt, tvl, src = _inputs(name)
    dev = lambda a: torch.from_numpy(a).cuda()
    table = dev(wide)[:, :c["F"]]                                                   # row stride ld: no copy is made of it
    out = {"c": c, "p": p, "src": src, "svl": svl, "tgt": tgt, "tvl": tvl}
    for route in ("mat", "rows"):
        tr = _trainer(c, p)
        if route == "mat":
            loss, logits = tr.forward_backward(dev(src), dev(svl), dev(tgt), dev(tvl), return_logits=True)
        else:
            loss, logits = tr.forward_backward_rows(table, dev(idx), dev(svl), dev(tgt), dev(tvl), return_logits=True)
        out[route] = (loss.clone(), logits.clone(), tr.grads.clone(), {k: tr.get(k, gradient=True) for k in p})
        if c.get("drop"):
            nl, nbi, B, T, H = c["nl"], c["nbi"], c["B"], c["T"], c["H"]
            out[route + "_masks"] = {"enc": [tr.dropout_mask(i, (B, T, (2 if i < nbi else 1) * H)).cpu().numpy() for i in range(nl)],
                                     "dec": {j: tr.dropout_mask(nl + j, (L - 1, B, H)).cpu().numpy() for j in range(1, nl)}}
        tr.step(LR)
        out[route + "_params"] = (tr.params.clone(), tr.state_dict())
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_gathered_step_equals_the_materialised_step_bit_for_bit(name):
    r = _run(name)
    (l0, lg0, g0, named0), (l1, lg1, g1, named1) = r["mat"], r["rows"]
    assert torch.equal(l0, l1) and torch.equal(lg0, lg1)
    assert torch.equal(g0, g1), "the flat gradient buffer"
    assert set(named0) == set(named1) == set(r["p"])
    for k in named0:
        assert np.array_equal(named0[k], named1[k]), k
    assert np.abs(named1["gnmt_enc_rnn0_l_i2h_weight" if r["c"].get("nbi", 1) else "gnmt_enc_rnn0_i2h_weight"]).max() > 0
    assert torch.equal(r["mat_params"][0], r["rows_params"][0]), "every parameter after one Adam step"
    for k in r["p"]:
        assert np.array_equal(r["mat_params"][1][k], r["rows_params"][1][k]), k
        assert not np.array_equal(r["rows_params"][1][k], r["p"][k]), k


@pytest.mark.parametrize("name", ORACLE)
def test_gathered_step_against_the_float64_oracle(report, name):
    r = _run(name)
    c, p = r["c"], r["p"]
    loss, logits, _, grads = r["rows"]
    kw = dict(cell=c["cell"], num_layers=c.get("nl", 2), num_bi_layers=c.get("nbi", 1), use_residual=c.get("res", False))
    rl, rlog, rg = gt.loss_and_grads(p, r["src"], r["svl"], r["tgt"], r["tvl"], c["H"], masks=r.get("rows_masks"), **kw)
    e_loss, e_logits = abs(float(loss) - rl), float(np.abs(logits.cpu().numpy() - rlog).max())
    errs = {k: float(np.abs(grads[k] - g).max() / max(1e-7, np.abs(g).max())) for k, g in rg.items()}
    q, _, _ = gt.adam_step({k: v.astype(np.float64) for k, v in p.items()}, rg, {}, {}, 1, LR)
    st = r["rows_params"][1]
    perr = {k: float(np.abs(st[k] - q[k]).max() / max(1.0, np.abs(q[k]).max())) for k in q}
    print(f"{name}: loss err {e_loss:.2e} (loss {rl:.4f}) logits err {e_logits:.2e} worst gradient err {max(errs.values()):.2e} "
          f"worst parameter err after Adam {max(perr.values()):.2e}")
    report[f"gnmt_rows_{name}_grad_rel_err"] = max(errs.values())
    assert e_loss < 1e-4 * max(1.0, abs(rl)) and e_logits < 1e-4
    for k, e in errs.items():
        assert e < 2e-3, (k, e)
    for k, e in perr.items():
        assert e < 2e-4, (k, e)


@pytest.mark.parametrize("name", ["skinny_gru", "skinny_lstm", "big_gru_T88", "three_layers"])
def test_encode_rows_decode_and_beam_search_equal_the_materialised_route(name):
    from tennis_amd.engine import GNMTCaptioner
    c, p, wide, idx, svl, tgt, tvl, src = _inputs(name)
    dev = lambda a: torch.from_numpy(a).cuda()
    table = dev(wide)[:, :c["F"]]
    got = {}
    for route in ("mat", "rows", "rows_host_idx"):
        cap = GNMTCaptioner(p, c["F"], c["H"], E, V, beam=3, max_length=8, max_batch=c["B"], max_src_len=c["T"], cell_type=c["cell"],
                            num_layers=c.get("nl", 2), num_bi_layers=c.get("nbi", 1), use_residual=c.get("res", False))
        if route == "mat":
            mem = cap.encode(dev(src), dev(svl))
        else:
            mem = cap.encode_rows(table, dev(idx) if route == "rows" else idx, dev(svl) if route == "rows" else svl.astype(np.float32))
        logits = cap.decode_seq(dev(tgt)[:, :-1])
        got[route] = (mem, logits) + tuple(cap.beam_search(2, 3, 1.0, 5.0))
    assert float(got["mat"][0].abs().max()) > 0
    for route in ("rows", "rows_host_idx"):
        for a, b, what in zip(got["mat"], got[route], ("mem", "decode_seq logits", "beam ids", "beam scores", "beam lengths")):
            assert a.shape == b.shape and torch.equal(a, b), (route, what)


def test_translate_rows_and_evaluate_by_rows_equal_the_loader_route():
    """the model-level surface: ``BeamSearchTranslator.translate_rows`` and ``captions.evaluate(..., table=...)`` on a synthetic split"""
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
    got = cp.evaluate(cp.bucketed_batches(va_set, 3, 2, rows=rows), model, translator, tr_set, table=table)
    assert got[0] == want[0] and got[1] == want[1] and len(got[1]) == len(va_set)
    with pytest.raises(ValueError, match="no feature table"):
        cp.evaluate(cp.bucketed_batches(va_set, 3, 2, rows=rows), model, translator, tr_set)
    src, _, svl, _, _ = next(cp.bucketed_batches(va_set, 3, 2))
    ridx = next(cp.bucketed_batches(va_set, 3, 2, rows=rows))[0]
    for a, b in zip(translator.translate(src, svl), translator.translate_rows(table, ridx, svl)):
        assert torch.equal(a, b)


def test_rows_calls_contract():
    from tennis_amd import _lib
    from tennis_amd.engine import GNMTCaptioner
    c, p, wide, idx, svl, tgt, tvl, src = _inputs("skinny_gru")
    B, T, F, R = c["B"], c["T"], c["F"], c["R"]
    dev = lambda a: torch.from_numpy(a).cuda()
    td, idx_d, svl_d, tgt_d, tvl_d = dev(wide), dev(idx), dev(svl), dev(tgt), dev(tvl)
    table = td[:, :F]
    tr = _trainer(c, p)
    cap = GNMTCaptioner(p, F, c["H"], E, V, beam=2, max_length=6, max_batch=B, max_src_len=T, cell_type="gru")
    # a host idx out of range, or with a pad step inside a valid length, raises before any launch: no gradient has been written
    for bad, where, msg in ((-2, (0, 3), "idx must lie in"), (R, (2, 1), "idx must lie in"), (-1, (2, 32), "before its valid length"),
                            (-1, (1, 0), "before its valid length")):
        wrong = idx.copy()
        wrong[where] = bad
        for host in (wrong, torch.from_numpy(wrong), wrong.astype(np.int64)):
            with pytest.raises(ValueError, match=msg):
                tr.forward_backward_rows(table, host, svl, tgt_d, tvl_d)
            with pytest.raises(ValueError, match=msg):
                cap.encode_rows(table, host, svl)
    with pytest.raises(ValueError, match="integers"):
        tr.forward_backward_rows(table, idx.astype(np.float32), svl, tgt_d, tvl_d)
    with pytest.raises(ValueError, match="batch, steps"):
        tr.forward_backward_rows(table, idx[0], svl, tgt_d, tvl_d)
    # the table: dtype, shape, device
    for wrong in (td.double()[:, :F], td[:, :F - 1], td[0, :F], torch.from_numpy(wide)[:, :F], wide[:, :F]):
        with pytest.raises(ValueError):
            tr.forward_backward_rows(wrong, idx_d, svl_d, tgt_d, tvl_d)
        with pytest.raises(ValueError):
            cap.encode_rows(wrong, idx_d, svl_d)
    assert float(tr.grads.abs().max()) == 0.0
    # the C ABI underneath: nulls, ld < F, n_rows < 1, batch / steps against the handle
    lib, ptr, null = tr.lib, _lib.ptr, C.c_void_p(None)
    loss = torch.empty(1, device="cuda")
    fb = lambda **kw: lib.tn_gnmt_trainer_forward_backward_rows(*[{**dict(
        t=tr.handle, table=ptr(table), n=R, ld=c["ld"], idx=ptr(idx_d), svl=ptr(svl_d), tgt=ptr(tgt_d), ldt=L, tvl=ptr(tvl_d), b=B, s=T, l=L,
        loss=ptr(loss), logits=null), **kw}[k] for k in ("t", "table", "n", "ld", "idx", "svl", "tgt", "ldt", "tvl", "b", "s", "l", "loss", "logits")])
    for kw in (dict(t=null), dict(table=null), dict(idx=null), dict(svl=null), dict(tgt=null), dict(tvl=null), dict(loss=null)):
        assert fb(**kw) == -1 and b"null argument" in lib.tn_last_error(), kw
    for kw in (dict(ld=F - 1), dict(n=0)):
        assert fb(**kw) == -1 and b"input size" in lib.tn_last_error(), kw
    for kw in (dict(b=B + 1), dict(s=T + 1), dict(b=0), dict(s=0), dict(l=L + 2), dict(l=1)):
        assert fb(**kw) == -1 and b"exceed the handle" in lib.tn_last_error(), kw
    enc = lambda **kw: lib.tn_gnmt_encode_rows(*[{**dict(g=cap.handle, table=ptr(table), n=R, ld=c["ld"], idx=ptr(idx_d), vl=ptr(svl_d), b=B,
                                                            s=T, mem=null), **kw}[k] for k in ("g", "table", "n", "ld", "idx", "vl", "b", "s", "mem")])
    for kw in (dict(g=null), dict(table=null), dict(idx=null), dict(vl=null)):
        assert enc(**kw) == -1 and b"null argument" in lib.tn_last_error(), kw
    for kw in (dict(ld=F - 1), dict(n=0)):
        assert enc(**kw) == -1 and b"input size" in lib.tn_last_error(), kw
    for kw in (dict(b=B + 1), dict(s=T + 1), dict(b=0), dict(s=0)):
        assert enc(**kw) == -1 and b"exceed the handle" in lib.tn_last_error(), kw
    assert float(tr.grads.abs().max()) == 0.0
    assert fb() == 0 and enc() == 0 and float(tr.grads.abs().max()) > 0
    # a smaller batch and fewer steps than the maxima, from a host idx
    sub = idx[:2, :40].copy()
    sub[0, 38:] = -1
    l2 = tr.forward_backward_rows(table, sub, np.array([38, 2], np.int32), tgt_d[:2], tvl_d[:2])
    assert bool(torch.isfinite(l2))


def test_device_idx_past_the_table_is_the_clamped_index():
    """The kernels clamp an index >= rows to the last row and read zeros for ANY negative index (linear.hip, train.hip: the clamp
    stands in front of every address).  A device idx is not range-checked on the host: its result is that of the clamped indices."""
    c, p, wide, idx, svl, tgt, tvl, src = _inputs("skinny_gru")
    R = c["R"]
    dev = lambda a: torch.from_numpy(a).cuda()
    table = dev(wide)[:, :c["F"]]
    beyond, clamped = idx.copy(), idx.copy()
    beyond[0, 7], beyond[0, 8], beyond[2, 3] = R, R + 7, np.iinfo(np.int32).max
    beyond[1, 5], beyond[2, 40] = -7, np.iinfo(np.int32).min                  # pad steps behind their clips' ends: any negative value
    clamped[0, 7] = clamped[0, 8] = clamped[2, 3] = R - 1
    res = []
    for ix in (beyond, clamped):
        tr = _trainer(c, p)
        loss, logits = tr.forward_backward_rows(table, dev(ix), dev(svl), dev(tgt), dev(tvl), return_logits=True)
        res.append((loss.clone(), logits.clone(), tr.grads.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_drivers_with_feats_on_device_equal_the_loader_route(tmp_path, monkeypatch, capsys):
    """train_gnmt with and without --feats_on_device on a small on-disk tree (a dozen ragged train points, H 16, two epochs, dropout
    on): byte-identical .params files, identical epoch*_out.txt, equal history; under the flag each .npy is opened once per split.
    evaluate_gnmt with the flag: the same loss, BLEU and sentences."""
    from tennis_amd import evaluate_gnmt as eg, train_gnmt as tg
    from tools import clip_tree
    root, exp = str(tmp_path / "data"), str(tmp_path / "exp")
    clip_tree.write(root, feature_dim=20)
    n_files = sum(len({f for a, b in clips for f in range(a, b)}) for clips in clip_tree.CLIPS.values())     # the frames some point reads
    assert n_files < sum(len(f) for _, _, f in os.walk(os.path.join(root, "features"))), "the tree holds frames outside every point too"
    hists, opened, real_train, real_load = [], [], tg.train, np.load

    def counting_train(*a, **k):
        monkeypatch.setattr(np, "load", lambda path, *x, **y: (opened[-1].append(str(path)), real_load(path, *x, **y))[1])
        opened.append([])
        try:
            hists.append(real_train(*a, **k))
        finally:
            monkeypatch.setattr(np, "load", real_load)
        return hists[-1]

    monkeypatch.setattr(tg, "train", counting_train)
    common = ["--data_root", root, "--feats_model", "0042", "--root", exp, "--num_hidden", "16", "--emb_size", "8", "--emb_file", "",
              "--tgt_max_len", "12", "--beam_size", "2", "--test_batch_size", "2", "--num_buckets", "2"]
    train = ["--epochs", "2", "--batch_size", "4", "--dropout", "0.2", "--lr", "0.01"]
    assert tg.main(common + train + ["--model_id", "loader"]) == 0
    assert tg.main(common + train + ["--model_id", "table", "--feats_on_device"]) == 0
    a, b = os.path.join(exp, "loader"), os.path.join(exp, "table")
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and {"0000.params", "0001.params", "epoch0_valid_out.txt", "epoch1_test_out.txt"} <= set(files)
    for f in files:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert len(hists) == 2 and len(hists[0]) == 2 and hists[0] == hists[1]
    assert len(opened[1]) == len(set(opened[1])) == n_files, "under the flag every .npy is opened once per split (the splits share none)"
    assert len(opened[0]) > 2 * n_files, "the loader route reads a frame's file once per point and pass"
    outs, sents = [], []
    for extra in ([], ["--feats_on_device"]):
        outs.append(eg.main(common + ["--model_id", "table"] + extra))
        sents.append([open(os.path.join(b, f"best_{s}_out.txt")).read() for s in ("valid", "test")])
    assert outs[0] == outs[1] and sents[0] == sents[1] and set(outs[0]) == {"valid", "test"}
    assert all(s.count("\n") == 3 for s in sents[0])
    with pytest.raises(SystemExit, match="--feats_model"):
        tg.main(["--data_root", root, "--feats_on_device", "--model_id", "x", "--root", exp])
