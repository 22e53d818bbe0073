"""-m "not gpu": the oracle against independent CPU implementations and the
reference's own golden vectors; host logic; C-ABI surface."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import densenet_np as dn
from oracle import rnn_np as rn
from oracle import vision_np as vn
from oracle.torch_ref import TorchDenseNet121
from tennis_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_densenet_oracle_matches_torch_cpu():
    p = W.make_densenet121_weights(0)
    x = W.normalize_to_nchw_f32(W.synthetic_frames_u8(1, 224))
    f = dn.densenet121_features(x, p)
    ft = TorchDenseNet121(p)(torch.from_numpy(x)).numpy()
    assert f.shape == (1, 1024)
    assert np.abs(f - ft).max() < 2e-5
    assert 0.1 < f.mean() < 3 and np.isfinite(f).all()      # activations stay O(1) through 120 convs


def test_densenet_feature_width_tracks_input_size():
    # AvgPool2D(7) floor + NCHW flatten: 1024 @224, 4096 @512 (reference train.py:259); check 256 -> 1024 cheaply
    p = W.make_densenet121_weights(0)
    x = np.random.default_rng(0).normal(0, 1, (1, 3, 256, 256)).astype(np.float32)
    assert dn.densenet121_features(x, p).shape == (1, 1024)
    ft = TorchDenseNet121(p)(torch.from_numpy(x)).numpy()
    assert np.abs(dn.densenet121_features(x, p) - ft).max() < 2e-5


def test_densenet_layout_counts():
    convs, final_bn, c = W.densenet121_layout()
    assert len(convs) == 120 and c == 1024 and final_bn == "batchnorm4"
    p = W.make_densenet121_weights(0)
    assert sum(v.size for k, v in p.items() if k.endswith("_weight")) == 6_870_208  # 6.870 M
    macs = 0
    h = 56
    for cv in convs:
        if cv["kind"] == "stem":
            macs += 112 * 112 * 64 * 147
        else:
            k = 9 if cv["kind"] == "dense3x3" else 1
            hw = {1: 56, 2: 28, 3: 14, 4: 7}[cv["stage"]] ** 2
            macs += hw * cv["cin"] * cv["cout"] * k
    assert abs(macs / 1e9 - 2.8331) < 1e-3


@pytest.mark.parametrize("mode", ["gru", "lstm"])
def test_rnn_oracle_matches_torch(mode):
    b, t, f, h = 3, 7, 20, 16
    p = W.make_rnn_weights(5, mode, f, h, "r_")
    x = np.random.default_rng(1).normal(0, 1, (b, t, f)).astype(np.float32)
    ref, _, _ = rn.birnn_layer(x, p, "r_", mode)
    net = (torch.nn.GRU if mode == "gru" else torch.nn.LSTM)(f, h, batch_first=True, bidirectional=True)
    with torch.no_grad():
        for d, suf in (("l", ""), ("r", "_reverse")):
            getattr(net, "weight_ih_l0" + suf).copy_(torch.from_numpy(p[f"r_{d}0_i2h_weight"]))
            getattr(net, "weight_hh_l0" + suf).copy_(torch.from_numpy(p[f"r_{d}0_h2h_weight"]))
            getattr(net, "bias_ih_l0" + suf).copy_(torch.from_numpy(p[f"r_{d}0_i2h_bias"]))
            getattr(net, "bias_hh_l0" + suf).copy_(torch.from_numpy(p[f"r_{d}0_h2h_bias"]))
        out = net(torch.from_numpy(x))[0].numpy()
    assert np.abs(out - ref).max() < 1e-5


def test_rnn_valid_length_semantics():
    """Reverse pass starts at the last valid step; padded steps emit zeros and leave the state alone."""
    b, t, f, h = 3, 6, 5, 4
    p = W.make_rnn_weights(2, "gru", f, h, "r_")
    x = np.random.default_rng(3).normal(0, 1, (b, t, f)).astype(np.float32)
    vl = np.array([6, 3, 1])
    out, (fh, _), (bh, _) = rn.birnn_layer(x, p, "r_", "gru", vl)
    for i in range(b):
        o_i, (fh_i, _), (bh_i, _) = rn.birnn_layer(x[i:i + 1, :vl[i]], p, "r_", "gru")
        assert np.allclose(out[i, :vl[i]], o_i[0], atol=1e-6)
        assert np.all(out[i, vl[i]:] == 0)
        assert np.allclose(fh[i], fh_i[0], atol=1e-6) and np.allclose(bh[i], bh_i[0], atol=1e-6)


def _prf1_inputs(case, classes):
    rng = np.random.RandomState(case["seed"])
    out = []
    for _ in range(case["batches"]):
        logits = rng.randn(case["n"], len(classes)).astype(np.float32)
        labels = rng.randint(0, len(classes), case["n"]).astype(np.float32)
        logits[np.arange(case["n"]), labels.astype(int)] += 1.5
        out.append((labels, logits))
    return out


def test_prf1_against_reference_golden():
    """Both the oracle PRF1 and the product PRF1 (host path) reproduce the vectors the
    reference's own metrics/vision.py::PRF1 produced (tests/golden/make_reference_golden.py)."""
    from tennis_amd.metrics.vision import PRF1
    g = json.load(open(os.path.join(GOLD, "prf1_reference.json")))
    for case in g["cases"]:
        for cls in (vn.PRF1, lambda label_names: PRF1(label_names=label_names)):
            m = cls(g["classes"])
            for labels, logits in _prf1_inputs(case, g["classes"]):
                m.update([labels], [logits])
            got = m.get()
            assert [k for k, _ in got] == [k for k, _ in case["scores"]]
            assert len(got) == 39
            assert np.allclose([v for _, v in got], [v for _, v in case["scores"]], rtol=0, atol=1e-12)
            assert np.array_equal(m.mat, np.array(case["mat"]))


def test_time_distributed_shape_contract():
    """reference definitions.py:166-167: TimeDistributed(Debug()) maps (3,2,3,2,2) -> (3,2,4,1,1)."""
    from tennis_amd.utils.layers import TimeDistributed
    calls = []

    def fake_model(x):
        calls.append(tuple(x.shape))
        return np.zeros((x.shape[0], 4, 1, 1), np.float32)
    td = TimeDistributed(fake_model)
    y = td(np.ones((3, 2, 3, 2, 2), np.float32))
    assert y.shape == (3, 2, 4, 1, 1) and calls == [(6, 3, 2, 2)]
    a, b = td.__class__(lambda x: (np.zeros((x.shape[0], 5)), np.zeros((x.shape[0], 2))))(np.ones((3, 2, 7)))
    assert a.shape == (3, 2, 5) and b.shape == (3, 2, 2)
    assert vn.time_distributed(lambda z: z.sum(-1), np.ones((3, 2, 7))).shape == (3, 2)


def test_dataset_paths_and_windows():
    from tennis_amd.dataset import DataLoader, TennisSet
    assert TennisSet.get_feature_path("data/features/0006", "V006", 1234) == \
        "data/features/0006/V006.mp4/0000001000/0000001234.npy"
    assert TennisSet.get_image_path("data/frames", "V006", 999) == "data/frames/V006.mp4/0000000000/0000000999.jpg"
    d = TennisSet(window=4, data_shape=32, frames_per_video=10)
    assert d.window_frames(d._samples[0]) == [0, 0, 0, 1]          # offsets -2..1 clamped at 0
    assert d.window_frames(d._samples[9]) == [7, 8, 9, 9]          # clamped at max_frame
    x, label, idx = d[3]
    assert x.shape == (4, 3, 32, 32) and x.dtype == np.float32 and idx == 3 and 0 <= label < 11
    d2 = TennisSet(window=5, stride=2, every=2, data_shape=32, frames_per_video=11)
    assert d2.window_frames(["V006", 4, "OTH"]) == [0, 2, 4, 6, 8]  # offsets -2..2, stride 2
    assert d2.window_frames(["V006", 10, "OTH"])[-1] == 8           # max_frame = 11-2 = 9 snapped down to an `every` frame (dataset.py:196-200)
    xb, lb, ib = next(iter(DataLoader(TennisSet(data_shape=32), batch_size=5)))
    assert xb.shape == (5, 3, 32, 32) and lb.shape == (5,) and list(ib) == [0, 1, 2, 3, 4]
    pad = TennisSet(data_shape=32, frames_per_video=10, save_feats=True, split_first=5, video_length=30,
                    videos=("V006",))
    assert len(pad) == 30 and all(s[2] == "OTH" for s in pad._samples[10:])


def test_abi_library_exports_every_declared_symbol():
    from tennis_amd import _lib
    header = open(os.path.join(ROOT, "include", "tennis_hip.h")).read()
    debug = open(os.path.join(ROOT, "include", "tennis_hip_debug.h")).read()
    public = sorted(set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", header)))
    hooks = sorted(set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", debug)))
    # the drop-in header carries the reference's surface only: test / tuning hooks live in tennis_hip_debug.h
    assert not [n for n in public if n.startswith("tn_dbg_") or n in ("tn_densenet121_profile", "tn_densenet121_read_tap", "tn_jpeg_sync_passes")]
    assert len(public) >= 60 and len(hooks) >= 20 and not set(public) & set(hooks)
    declared = sorted(public + hooks)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"
    assert sorted(_lib.declared_symbols()) == declared            # the ctypes table covers the whole header
    assert _lib.load().tn_version() >= 100


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from tennis_amd import _lib
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.Context(0)
    from tennis_amd.model_zoo import get_model
    from tennis_amd.models.vision.definitions import FrameModel
    m = FrameModel(get_model("DenseNet121", pretrained=True).features, 11)
    with pytest.raises((RuntimeError, AssertionError)):
        m(np.zeros((1, 3, 224, 224), np.float32))


def test_block_surface_roundtrip(tmp_path):
    """initialize / collect_params / save_parameters / load_parameters keep Gluon names."""
    from tennis_amd.models.vision.definitions import CNNRNN
    m = CNNRNN(None, num_classes=11, type="lstm", hidden_size=8, prefix="cnnrnn0_")
    m.initialize(); m.hybridize()
    p = W.make_rnn_weights(1, "lstm", 12, 8, "cnnrnn0_lstm0_")
    p.update(W.make_dense_weights(2, 11, 16, "cnnrnn0_dense0_"))
    m.set_params(p)
    f = str(tmp_path / "0003.params")
    m.save_parameters(f)
    m2 = CNNRNN(None, num_classes=11, type="lstm", hidden_size=8, prefix="cnnrnn0_")
    m2.load_parameters(f)
    for k, v in m.collect_params().items():
        assert np.array_equal(v.data, m2.collect_params()[k].data)
    assert "cnnrnn0_lstm0_r0_h2h_weight" in m.collect_params()
    m.collect_params().reset_ctx([0])
    for prm in m.collect_params().values():
        prm.grad_req = "null"                                       # evaluate.py:152-154


def test_caption_set_batching_and_sentences(tmp_path):
    """dataset.py:52-74 caption ids, utils/captioning.py Pad batches + write_sentences (host logic only)."""
    from tennis_amd.captions import CaptionSet, bucketed_batches, pad_batchify, write_sentences
    train = CaptionSet(split="train", n_points=10, feature_dim=8, mean_frames=6, max_cap_len=5)
    v = train.vocab
    assert v.idx_to_token[:4] == ["<unk>", "<pad>", "<bos>", "<eos>"]
    x, cap, tl, cl = train[0]
    assert cap.dtype == np.int32 and cap[0] == v["<bos>"] and cap[-1] == v["<eos>"] and cl == len(cap) <= 7
    assert x.shape == (tl, 8)
    test = CaptionSet(split="test", n_points=9, feature_dim=8, mean_frames=6, vocab=v, inference=True, every=2)
    seen = []
    for src, tgt, svl, tvl, ids in bucketed_batches(test, 4):
        assert src.dtype == np.float32 and tgt.dtype == np.int32 and svl.dtype == np.float32
        for r, i in enumerate(ids):
            s = test[int(i)]
            assert np.array_equal(src[r, :s[2]], s[0]) and not src[r, s[2]:].any()
            assert np.array_equal(tgt[r, :s[3]], s[1]) and not tgt[r, s[3]:].any()
        seen += ids.tolist()
    assert sorted(seen) == list(range(9))
    f = tmp_path / "out.txt"
    write_sentences([["a", "b"], "c d"], str(f))
    assert f.read_text() == "a b\nc d\n"


def test_bucketed_batches_training_sampler():
    """FixedBucketSampler(shuffle=True) stand-in (utils/captioning.py:48-55): every sample exactly once per epoch, the
    order changes from epoch to epoch and is reproducible; data-parallel ranks split the same batch list evenly."""
    from tennis_amd.captions import CaptionSet, bucketed_batches
    ds = CaptionSet(split="train", n_points=23, feature_dim=4, mean_frames=5, max_cap_len=9, inference=True)   # ids travel with the batch
    ids = lambda **kw: [b[-1].astype(int).tolist() for b in bucketed_batches(ds, 4, 3, **kw)]
    plain = ids()
    e0, e0b, e1 = ids(shuffle=True, seed=5, epoch=0), ids(shuffle=True, seed=5, epoch=0), ids(shuffle=True, seed=5, epoch=1)
    for ep in (plain, e0, e1):
        assert sorted(i for b in ep for i in b) == list(range(23))
    assert e0 == e0b and e0 != e1 and e0 != plain
    lens = [l[-1] for l in ds.get_data_lens()]
    width = -(-(max(lens) - min(lens) + 1) // 3)
    for b in e0:                                        # a batch never mixes buckets
        assert len({(lens[i] - min(lens)) // width for i in b}) == 1
    r0, r1 = ids(shuffle=True, seed=5, epoch=0, rank=0, world=2), ids(shuffle=True, seed=5, epoch=0, rank=1, world=2)
    assert len(r0) == len(r1) == -(-len(e0) // 2)
    assert sorted(i for b in e0 for i in b) == sorted(set(i for b in r0 + r1 for i in b))


def _wavg_worker(rank, world, port, q):
    import os
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch
    import torch.distributed as dist
    from tennis_amd.train_gnmt import allreduce_grads
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class T:                                            # the surface allreduce_grads uses: a flat gradient tensor
        grads = torch.tensor([1.0, 2.0]) if rank == 0 else torch.tensor([5.0, -2.0])
    t = T()
    allreduce_grads(t, 30 if rank == 0 else 10)
    q.put((rank, t.grads.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_captioner_ddp_gradients_are_token_weighted():
    """Ranks average per-TOKEN: (30*g0 + 10*g1) / 40, not (g0 + g1) / 2 (reference loss: train_gnmt.py:332-333)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 400) + 17
    procs = [ctx.Process(target=_wavg_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=120) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
    for _, g in res:
        assert np.allclose(g, [(30 * 1 + 10 * 5) / 40, (30 * 2 - 10 * 2) / 40])


def test_gnmt_oracle_properties():
    """Beam 1 == greedy argmax decoding; padding the source does not change the result;
    BOS first / EOS at valid_len-1; teacher-forced log-softmax row equals the step's logp."""
    from oracle import gnmt_np as gn
    from tennis_amd import weights as W
    F, H, E, V = 24, 16, 8, 30
    p = W.make_gnmt_weights(3, "gru", F, H, E, V)
    p["gnmt_tgt_proj_weight"] = (p["gnmt_tgt_proj_weight"] * 20).astype(np.float32)
    rng = np.random.default_rng(3)
    x = np.abs(rng.normal(0, 1, (2, 9, F))).astype(np.float32)
    vl = np.array([9, 6])
    mem, st = gn.encoder(x, vl, p, "gru", H)
    assert not mem[1, 6:].any()
    dec = gn.Decoder(p, H)
    s1, sc1, v1 = gn.beam_search(dec, mem, st, vl, 2, 3, beam=1, max_length=12)
    states, att = dec.init_state(mem, st, vl)
    for b in range(2):
        rs, a, tok, out = [s[b:b + 1] for s in states], att[b:b + 1], np.array([2]), [2]
        for _ in range(12):
            logp, rs, a = dec.step(tok, rs, a, np.array([b]))
            tok = logp.argmax(-1)
            out.append(int(tok[0]))
            if out[-1] == 3:
                break
        else:
            out.append(3)
        assert list(s1[b, 0, :v1[b, 0]]) == out
    mem2, st2 = gn.encoder(x[1:, :6], vl[1:], p, "gru", H)
    s2, _, v2 = gn.beam_search(gn.Decoder(p, H), mem2, st2, vl[1:], 2, 3, beam=4, max_length=12)
    s4, _, v4 = gn.beam_search(dec, mem, st, vl, 2, 3, beam=4, max_length=12)
    assert np.array_equal(v2[0], v4[1]) and np.array_equal(s2[0, 0, :v2[0, 0]], s4[1, 0, :v4[1, 0]])
    assert (s4[:, :, 0] == 2).all()
    for b in range(2):
        for k in range(4):
            assert s4[b, k, v4[b, k] - 1] == 3
    tgt = rng.integers(4, V, (2, 5))
    lg = gn.decode_seq(dec, mem, st, vl, tgt)
    states, att = dec.init_state(mem, st, vl)
    logp, _, _ = dec.step(tgt[:, 0], states, att, np.arange(2))
    assert np.allclose(gn._log_softmax(lg[:, 0]), logp, atol=1e-6)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_gnmt_oracle_matches_independent_torch_restatement(cell):
    """oracle/gnmt_np.py against oracle/gnmt_torch.py (nn.GRUCell / nn.LSTMCell, F.softmax, torch.topk, float64): one
    decode step (log-probabilities, recurrent states, attention context) and three beam-search steps (token ids, beam
    order, scores, finished flags).  reference gnmt.py:369-404, utils/translation.py:51-82."""
    from oracle import gnmt_np as gn, gnmt_torch as gt
    from tennis_amd import weights as W
    F, H, E, V, B, T, beam = 24, 16, 8, 30, 3, 9, 4
    p = W.make_gnmt_weights(7, cell, F, H, E, V)
    p["gnmt_tgt_proj_weight"] = (p["gnmt_tgt_proj_weight"] * 25).astype(np.float32)   # spread the log-probabilities
    rng = np.random.default_rng(11)
    x = np.abs(rng.normal(0, 1, (B, T, F))).astype(np.float32)
    vl = np.array([9, 6, 3])
    mem, st = gn.encoder(x, vl, p, cell, H)
    dec = gn.Decoder(p, H, cell=cell)
    states, att = dec.init_state(mem, st, vl)
    tok = rng.integers(4, V, B)
    att = np.abs(rng.normal(0, 0.3, att.shape)).astype(np.float32)
    logp, ns, ctx = dec.step(tok, states, att, np.arange(B))
    td = gt.TorchDecoder(p, H, E, cell)
    td.init(mem, vl)
    tl, tns, tctx = td.step(tok, [torch.from_numpy(s).double() for s in states], torch.from_numpy(att).double(), torch.arange(B))
    assert np.abs(logp - tl.numpy()).max() < 2e-5 and np.abs(ctx - tctx.numpy()).max() < 2e-6
    assert len(ns) == len(tns) and max(np.abs(a - b.numpy()).max() for a, b in zip(ns, tns)) < 2e-6
    assert np.abs(np.exp(logp).sum(1) - 1).max() < 1e-5
    # masked attention: a padded source step carries no weight (clip 2 has 3 valid steps of 9)
    mem_pad = mem.copy(); mem_pad[2, 3:] = 99.0
    dec2 = gn.Decoder(p, H, cell=cell); dec2.init_state(mem_pad, st, vl)
    assert np.allclose(dec2.step(tok, states, att, np.arange(B))[2][2], ctx[2], atol=1e-6)
    # three beam-search steps: EOS (id 3) is reachable, so finished beams and the "emit -1" path are exercised
    s_np, sc_np, _ = gn.beam_search(dec, mem, st, vl, 2, 3, beam=beam, alpha=1.0, K=5, max_length=3)
    s_t, sc_t, alive_t = gt.beam_search(td, mem, st, vl, 2, 3, beam, 1.0, 5, 3)
    assert np.array_equal(s_np[:, :, :4], s_t)                     # BOS + 3 steps, same beams in the same order
    assert np.abs(sc_np - sc_t).max() < 2e-5
    assert np.array_equal(s_np[:, :, 4] == 3, alive_t)             # gnmt_np appends EOS to the unfinished beams


def test_bleu_pinned_to_reference_golden():
    """tennis_amd.metrics.bleu.compute_bleu vs vectors produced by the reference's own metrics/bleu.py
    (tests/golden/make_reference_golden.py): tokenised and plain-text inputs, both tokenisers, smoothing,
    case folding, BPE joins, compound splitting, an empty hypothesis."""
    import json
    from tennis_amd.metrics.bleu import compute_bleu
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bleu_reference.json")))
    n = 0
    for refs, hyps, cases in ((g["refs"], g["hyps"], g["cases"]), (g["text_refs"], g["text_hyps"], g["text_cases"])):
        for c in cases:
            got = compute_bleu(refs, hyps, **c["kwargs"])
            exp = c["result"]
            assert abs(got[0] - exp[0]) < 1e-12 and np.allclose(got[1], exp[1], atol=1e-12)
            assert abs(got[2] - exp[2]) < 1e-12 and got[3] == exp[3] and got[4] == exp[4]
            n += 1
    assert n == 9


def test_error_feedback_rounding_properties():
    """weights._round_fp16_error_feedback / as_fp16_model(input_means=...): every weight lands on one of its two fp16 neighbours,
    fp16-representable weights do not move, the mean-weighted row error is far below round-to-nearest's, and - on the oracle,
    with the means measured on OTHER frames - the conversion error of a conv + ReLU + average-pool stack drops accordingly."""
    from tennis_amd import weights as W
    rng = np.random.default_rng(0)
    w = rng.normal(0, 0.05, (32, 600)).astype(np.float64)
    m = np.abs(rng.normal(0.4, 0.2, 600))
    r = W._round_fp16_error_feedback(w, m)
    lo = w.astype(np.float16)
    up = np.nextafter(lo, np.where(w > lo.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    assert np.all((r == lo.astype(np.float64)) | (r == up.astype(np.float64)))
    assert np.array_equal(r.astype(np.float16).astype(np.float64), r)
    e_rtn = np.abs(((lo.astype(np.float64) - w) * m).sum(1)); e_ef = np.abs(((r - w) * m).sum(1))
    assert e_ef.mean() < 0.1 * e_rtn.mean() and e_ef.max() < 0.5 * e_rtn.mean(), (e_ef.mean(), e_ef.max(), e_rtn.mean())
    w16 = lo.astype(np.float64)
    assert np.array_equal(W._round_fp16_error_feedback(w16, m), w16)
    # end to end on a toy layer: positive activations, pooled output
    a_cal = np.maximum(rng.normal(0.3, 1.0, (4000, 600)), 0) * m[None, :]
    a_tst = np.maximum(rng.normal(0.3, 1.0, (4000, 600)), 0) * m[None, :]
    r2 = W._round_fp16_error_feedback(w, a_cal.mean(0))
    pool = lambda ww: (a_tst @ ww.T).mean(0)
    err_rtn, err_ef = np.abs(pool(lo.astype(np.float64)) - pool(w)).max(), np.abs(pool(r2) - pool(w)).max()
    assert err_ef < 0.2 * err_rtn, (err_ef, err_rtn)
    # through as_fp16_model: only convs named in input_means change, with the BN2 fold applied before the rounding
    p = W.make_densenet121_weights(3, fp16_model=False)
    name = "densenet0_stage1_conv0_weight"
    q = W.as_fp16_model(p, input_means={name: np.full(p[name].shape[1], 0.5)})
    plain = W.as_fp16_model(p)
    assert all(np.array_equal(q[k], plain[k]) for k in p if k != name) and (q[name] != plain[name]).any()
    s2 = p["densenet0_stage1_batchnorm1_gamma"] / np.sqrt(p["densenet0_stage1_batchnorm1_running_var"] + np.float32(W.BN_EPS))
    m1 = W.bn_relu_clamp_fold(p, "densenet0_stage1_batchnorm0")[2]  # round 5: ... and the scale of the BatchNorm + ReLU in front
    folded = (q[name] * s2.reshape(-1, 1, 1, 1) * m1.reshape(1, -1, 1, 1)).astype(np.float32)
    assert np.abs(folded - folded.astype(np.float16).astype(np.float32)).max() < 1e-6 * np.abs(folded).max() + 1e-9


def test_bn_relu_clamp_fold_properties():
    """csrc/calib_host.hip::bn_relu_clamp_fold (tn_bn_relu_clamp_fold, host code) and its numpy reference
    (weights.bn_relu_clamp_fold): relu(s x + t) = sw clamp(x, lo, hi) + tc with lo / hi fp16 numbers.  Exact on the unclipped side of
    every channel, within 2^-11 |t| on the clipped side; degenerate channels (zero / tiny / huge / non-finite scale: ADVICE r4 - the
    round-4 form saturated its shift there) give the right VALUES, not just finite ones; the library and numpy agree bit for bit."""
    from tennis_amd import weights as W
    rng = np.random.default_rng(5)
    n = 4096
    p = {"bn_gamma": (rng.uniform(0.05, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32), "bn_beta": rng.normal(0, 1.0, n).astype(np.float32),
         "bn_running_mean": rng.normal(0, 1.0, n).astype(np.float32), "bn_running_var": rng.uniform(0.01, 4.0, n).astype(np.float32)}
    # degenerate scales: zero, tiny with a positive / negative shift (gamma 5e-6 beta 1; gamma 1e-7 beta 0.1; gamma 1e-5 beta 2),
    # negative tiny, one that leaves the fp16 range, non-finite
    p["bn_gamma"][:10] = [0.0, 1e-7, 3e4, -1e-6, 5e-6, 1e-7, 1e-5, 1e-6, -1e-6, np.inf]
    p["bn_beta"][:10] = [0.7, 0.1, 0.3, 0.5, 1.0, 0.1, 2.0, -1.0, -1.0, 0.4]
    p["bn_running_mean"][:10] = 0.0
    p["bn_running_var"][:10] = 1.0
    p["bn_running_var"][2] = 1e-3
    lo, hi, sw, tc = W.bn_relu_clamp_fold(p, "bn")
    lib = W.bn_relu_clamp_fold(p, "bn", use_library=True)
    for a_, b_ in zip((lo, hi, sw, tc), lib):
        assert np.array_equal(a_, b_)
    s = (p["bn_gamma"] / np.sqrt(p["bn_running_var"] + np.float32(W.BN_EPS))).astype(np.float32)
    t = (p["bn_beta"] - p["bn_running_mean"] * s).astype(np.float32)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(sw).all() and np.isfinite(tc).all() and (lo <= hi).all()
    assert np.array_equal(lo.astype(np.float16).astype(np.float32), lo) and np.array_equal(hi.astype(np.float16).astype(np.float32), hi)
    # the function itself on fp16 inputs (what the concat buffer holds), every channel, the degenerate ones included
    x = np.concatenate([rng.normal(0, 2, (64, n)), rng.normal(0, 300, (8, n)), np.full((1, n), 2.0)]).astype(np.float16).astype(np.float64)
    sd, td = s.astype(np.float64), t.astype(np.float64)
    sd[9] = 0.0; td[9] = 0.0                               # (a non-finite scale - its shift is NaN - is served as the constant 0)
    want = np.maximum(x * sd + td, 0)
    got = sw.astype(np.float64) * np.clip(x, lo, hi) + tc
    err = np.abs(got - want)
    # clipped side: |s| times the rounding of the threshold (half an fp16 ulp of it: <= 2^-11 |t|, except where the threshold is an
    # fp16 subnormal - a scale of 1e6 - whose ulp is absolute)
    thr_ulp = np.spacing(np.abs(np.where(sd > 0, lo, hi)).astype(np.float16)).astype(np.float64)
    assert (err <= np.abs(sd) * 0.5 * thr_ulp + 1e-6 * np.abs(want) + 1e-30).all(), err.max()
    normal = np.abs(td) > 6.2e-5 * np.abs(sd)
    assert (err[:, normal] <= 2.0 ** -11 * np.abs(td[normal]) + 1e-6 * np.abs(want[:, normal]) + 1e-30).all()
    unclipped = want > 2.0 ** -10 * np.abs(td)              # away from the threshold on the open side: exact up to fp32 constants
    assert (err[unclipped] <= 1e-6 * np.abs(want[unclipped]) + 1e-7).all()
    # ADVICE r4's three cases at x = 2: 1.0, 0.1, 2.0 (round 4 gave 0.506, 0.0079, 1.01)
    assert np.allclose(got[-1, [4, 5, 6]], [1.0, 0.1, 2.0], rtol=0, atol=3e-5), got[-1, 4:7]
    assert got[-1, 7] == 0.0 and got[-1, 8] == 0.0 and got[-1, 0] == np.float32(0.7)
    # as_fp16_model folds the same sw: conv weights behind this BatchNorm are fp16 numbers once sw (and BN2's scale) are multiplied in
    q = {"densenet0_stage1_conv0_weight": rng.normal(0, 0.1, (128, n, 1, 1)).astype(np.float32)}
    q.update({k.replace("bn_", "densenet0_stage1_batchnorm0_"): v for k, v in p.items()})
    q.update({"densenet0_stage1_batchnorm1_gamma": rng.uniform(0.5, 1.5, 128).astype(np.float32), "densenet0_stage1_batchnorm1_beta": np.zeros(128, np.float32),
              "densenet0_stage1_batchnorm1_running_mean": np.zeros(128, np.float32), "densenet0_stage1_batchnorm1_running_var": rng.uniform(0.5, 2, 128).astype(np.float32)})
    # channel 2 (gamma 3e4 / sqrt(1e-3)) takes its weights out of the fp16 range: the conversion refuses the checkpoint, as the
    # library does at create (it used to hand out inf weights with a numpy overflow warning)
    with pytest.raises(ValueError, match="fp16 range"):
        W.as_fp16_model(q)
    q["densenet0_stage1_batchnorm0_gamma"] = q["densenet0_stage1_batchnorm0_gamma"].copy()
    q["densenet0_stage1_batchnorm0_gamma"][2] = 30.0
    sw = W.bn_relu_clamp_fold(q, "densenet0_stage1_batchnorm0")[2]
    conv = W.as_fp16_model(q)["densenet0_stage1_conv0_weight"]
    s2 = (q["densenet0_stage1_batchnorm1_gamma"] / np.sqrt(q["densenet0_stage1_batchnorm1_running_var"] + np.float32(W.BN_EPS))).astype(np.float32)
    folded = (conv * s2.reshape(-1, 1, 1, 1) * sw.reshape(1, -1, 1, 1)).astype(np.float32)
    live = sw != 0
    rel = np.abs(folded - folded.astype(np.float16).astype(np.float32))[:, live] / (np.abs(folded[:, live]) + 1e-30)
    big = (np.abs(folded[:, live]) > 1e-4) & (np.abs(folded[:, live]) < 6e4)     # (fp16 subnormals keep fewer bits; beyond the range the library refuses the layer)
    assert rel[big].max() < 1e-6
    assert np.array_equal(conv[:, ~live], q["densenet0_stage1_conv0_weight"][:, ~live])


def test_mxnet_params_reader_against_hand_built_file():
    """tests/golden/gluon_tiny.params was written byte by byte from the published NDArray-list layout
    (tests/golden/make_params_fixture.py, no params_io involved): the reader returns its arrays, dtypes and names,
    strips the Module ``aux:`` prefix, and ``Block.load_parameters`` maps the Gluon STRUCTURAL names of a
    ``TemporalPooling(model=None, num_classes=3)`` (reference definitions.py:60-61) onto the block's parameters."""
    from tennis_amd import params_io as pio
    from tennis_amd.models.vision.definitions import TemporalPooling
    f = os.path.join(os.path.dirname(__file__), "golden", "gluon_tiny.params")
    assert pio.is_mxnet_params(f)
    d = pio.load_mxnet_params(f)
    assert list(d) == ["classes.weight", "classes.bias", "half_vector", "running_thing"]
    assert d["classes.weight"].dtype == np.float32 and d["classes.weight"].shape == (2, 3)
    assert np.array_equal(d["classes.weight"], np.array([[0.5, -1.25, 2.0], [0.125, 3.5, -0.75]], np.float32))
    assert np.array_equal(d["classes.bias"], np.array([0.25, -0.5], np.float32))
    assert d["half_vector"].dtype == np.float16 and np.array_equal(d["half_vector"], np.array([1.0, -2.0, 0.5], np.float16))
    assert np.array_equal(d["running_thing"], np.array([7.0], np.float32))
    m = TemporalPooling(None, num_classes=2, pool="max", feats=True)
    m.load_parameters(f, ignore_extra=True)
    got = {k[len(m.classes.prefix):]: v.data for k, v in m.collect_params().items()}
    assert np.array_equal(got["weight"], d["classes.weight"]) and np.array_equal(got["bias"], d["classes.bias"])
    with pytest.raises(AssertionError, match="half_vector"):        # Gluon's behaviour for names the block does not have
        TemporalPooling(None, num_classes=2, pool="max", feats=True).load_parameters(f)


def test_captioner_checkpoint_structural_names(tmp_path):
    """tests/golden/gluon_gnmt_tiny.params (hand-built, make_params_fixture.py) holds the names Gluon's
    ``save_parameters`` writes for the reference's captioner block tree (gnmt.py:84-111,212-221 inside gluonnlp's
    NMTModel, train_gnmt.py:221-229).  ``NMTModel.load_parameters`` must place every array on the right engine
    parameter - the attention projection transposed (query-side Dense in the file, key-side matrix in the engine) -
    and ``save_parameters`` must write the same names and arrays back."""
    from tennis_amd import params_io as pio
    from tennis_amd.models.captioning.gnmt import NMTModel, get_gnmt_encoder_decoder, Vocab
    f = os.path.join(os.path.dirname(__file__), "golden", "gluon_gnmt_tiny.params")
    d = pio.load_mxnet_params(f)
    assert len(d) == 4 * 5 + 1 + 3

    def build(**kw):
        enc, dec = get_gnmt_encoder_decoder(cell_type="gru", hidden_size=2, num_layers=2, num_bi_layers=1)
        return NMTModel(src_vocab=None, tgt_vocab=Vocab({"a": 1}), encoder=enc, decoder=dec, embed_size=2,
                        prefix="gnmt_", input_size=3, **kw)
    m = build()
    assert len(m.tgt_vocab) == 5
    m.load_parameters(f)
    got = {k: v.data for k, v in m.collect_params().items()}
    assert all(v is not None for v in got.values()) and len(got) == len(d)
    pairs = {"encoder.rnn_cells.0.l_cell.i2h_weight": "gnmt_enc_rnn0_l_i2h_weight",
             "encoder.rnn_cells.0.r_cell.h2h_bias": "gnmt_enc_rnn0_r_h2h_bias",
             "encoder.rnn_cells.1.h2h_weight": "gnmt_enc_rnn1_h2h_weight",
             "decoder.rnn_cells.0.i2h_weight": "gnmt_dec_rnn0_i2h_weight",
             "decoder.rnn_cells.1.i2h_bias": "gnmt_dec_rnn1_i2h_bias",
             "tgt_embed.0.weight": "gnmt_tgt_embed_weight",
             "tgt_proj.weight": "gnmt_tgt_proj_weight", "tgt_proj.bias": "gnmt_tgt_proj_bias"}
    for sname, pname in pairs.items():
        assert np.array_equal(got[pname], d[sname]), sname
    wq = d["decoder.attention_cell._proj_query.weight"]
    assert wq[0, 1] != wq[1, 0] and np.array_equal(got["gnmt_dec_attention_key_weight"], wq.T)
    # every array of the file landed somewhere, once
    assert sorted(float(v.flat[0]) for v in got.values()) == sorted(float(v.flat[0]) for v in d.values())
    g = str(tmp_path / "0003.params")
    m.save_parameters(g)
    back = pio.load_mxnet_params(g)
    assert set(back) == set(d) and all(np.array_equal(back[k], d[k]) for k in d)
    # a model given its embedding table (train_gnmt.py:211-218) holds the Embedding itself: ``tgt_embed.weight``
    m2 = build(tgt_embed=got["gnmt_tgt_embed_weight"])
    m2.load_parameters(g, allow_missing=True)
    m2.save_parameters(g)
    assert "tgt_embed.weight" in pio.load_mxnet_params(g)
    m3 = build()
    m3.load_parameters(g)                                   # ... and a model that built its own reads that name too
    assert np.array_equal(m3.collect_params()["gnmt_tgt_embed_weight"].data, d["tgt_embed.0.weight"])
    # a file naming the projection on the key side is taken as is
    d2 = dict(d); d2["decoder.attention_cell._proj_key.weight"] = d2.pop("decoder.attention_cell._proj_query.weight")
    pio.save_mxnet_params(g, d2)
    m4 = build(); m4.load_parameters(g)
    assert np.array_equal(m4.collect_params()["gnmt_dec_attention_key_weight"].data, wq)


def test_mxnet_params_container_round_trip(tmp_path):
    """tennis_amd.params_io: NDArray-list container (V2 records) write -> read, dtype flags, 0-d / empty shapes,
    'arg:' / 'aux:' prefixes, and Block.load_parameters picking the format by its magic."""
    import struct
    from tennis_amd import params_io as pio
    from tennis_amd import weights as W
    from tennis_amd.models.vision.definitions import FrameModel
    from tennis_amd.model_zoo import get_model
    rng = np.random.default_rng(0)
    d = {"arg:fc_weight": rng.normal(size=(11, 7)).astype(np.float32), "aux:bn_moving_var": rng.random(5).astype(np.float32),
         "half": rng.normal(size=(2, 3, 4)).astype(np.float16), "ids": np.arange(6, dtype=np.int64).reshape(2, 3),
         "bytes": np.arange(5, dtype=np.uint8)}
    f = str(tmp_path / "x.params")
    pio.save_mxnet_params(f, d)
    assert pio.is_mxnet_params(f)
    back = pio.load_mxnet_params(f)
    assert set(back) == {"fc_weight", "bn_moving_var", "half", "ids", "bytes"}
    for k, v in d.items():
        k = k.split(":")[-1]
        assert back[k].dtype == v.dtype and np.array_equal(back[k], v)
    with open(f, "rb") as fh:                       # the header the format description gives
        assert struct.unpack("<QQQ", fh.read(24)) == (0x112, 0, 5) and struct.unpack("<I", fh.read(4))[0] == 0xF993FAC9
    # a model's parameters through the container
    p = W.make_densenet121_weights(0)
    p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
    g = str(tmp_path / "0006.params")
    pio.save_mxnet_params(g, p)
    fm = FrameModel(get_model("DenseNet121", pretrained=False).features, 11, prefix="framemodel0_")
    fm.load_parameters(g)
    got = {k: v.data for k, v in fm.collect_params().items()}
    assert set(got) == set(p) and all(np.array_equal(got[k], p[k]) for k in p)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_train_oracle_matches_torch_autograd(cell):
    """oracle/train_np.py (bi-GRU | bi-LSTM -> max over T -> Dense -> softmax CE, gradient of the summed loss) against
    torch autograd on the CPU: nn.GRU / nn.LSTM (bidirectional, batch_first) have the same gate order and equations."""
    from oracle import train_np as tn
    from tennis_amd import weights as W
    B, T, F, H, C_ = 3, 5, 12, 8, 11
    pre = f"cnnrnn0_{cell}0_"
    p = W.make_rnn_weights(2, cell, F, H, pre)
    p.update(W.make_dense_weights(3, C_, 2 * H, "cnnrnn0_dense0_"))
    rng = np.random.default_rng(1)
    x = rng.normal(0, 1, (B, T, F)).astype(np.float32)
    y = rng.integers(0, C_, B)
    loss, logits, g = tn.forward_backward(x, y, p, cell=cell)
    gru = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(F, H, batch_first=True, bidirectional=True).double()
    fc = torch.nn.Linear(2 * H, C_).double()
    with torch.no_grad():
        for d, suf in (("l0_", ""), ("r0_", "_reverse")):
            getattr(gru, "weight_ih_l0" + suf).copy_(torch.from_numpy(p[pre + d + "i2h_weight"]))
            getattr(gru, "weight_hh_l0" + suf).copy_(torch.from_numpy(p[pre + d + "h2h_weight"]))
            getattr(gru, "bias_ih_l0" + suf).copy_(torch.from_numpy(p[pre + d + "i2h_bias"]))
            getattr(gru, "bias_hh_l0" + suf).copy_(torch.from_numpy(p[pre + d + "h2h_bias"]))
        fc.weight.copy_(torch.from_numpy(p["cnnrnn0_dense0_weight"])); fc.bias.copy_(torch.from_numpy(p["cnnrnn0_dense0_bias"]))
    out, _ = gru(torch.from_numpy(x).double())
    lg = fc(out.max(dim=1).values)
    ls = torch.nn.functional.cross_entropy(lg, torch.from_numpy(y), reduction="none")
    ls.sum().backward()
    assert np.allclose(loss, ls.detach().numpy(), atol=1e-10) and np.allclose(logits, lg.detach().numpy(), atol=1e-10)
    for d, suf in (("l0_", ""), ("r0_", "_reverse")):
        assert np.allclose(g[pre + d + "i2h_weight"], getattr(gru, "weight_ih_l0" + suf).grad.numpy(), atol=1e-9)
        assert np.allclose(g[pre + d + "h2h_weight"], getattr(gru, "weight_hh_l0" + suf).grad.numpy(), atol=1e-9)
        assert np.allclose(g[pre + d + "i2h_bias"], getattr(gru, "bias_ih_l0" + suf).grad.numpy(), atol=1e-9)
        assert np.allclose(g[pre + d + "h2h_bias"], getattr(gru, "bias_hh_l0" + suf).grad.numpy(), atol=1e-9)
    assert np.allclose(g["cnnrnn0_dense0_weight"], fc.weight.grad.numpy(), atol=1e-9)
    assert np.allclose(g["cnnrnn0_dense0_bias"], fc.bias.grad.numpy(), atol=1e-9)


def test_oracle_reproduces_its_committed_fixtures():
    """tests/golden/oracle_*.npz (SURVEY §8c list: densenet121_224_b2, bigru / bilstm b2 t8 f1024, gnmt_step, beam_trace)
    were produced by tests/golden/make_oracle_fixtures.py from seeded inputs: the oracle must keep reproducing them.
    They pin the restatement to itself, not to MXNet (absent)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_oracle_fixtures", os.path.join(GOLD, "make_oracle_fixtures.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    from oracle import densenet_np as dn, gnmt_np as gn, rnn_np as rn
    for mode in ("gru", "lstm"):
        g = np.load(os.path.join(GOLD, f"oracle_bi{mode}_b2_t8_f1024.npz"))
        p, x, vl = mk.rnn_inputs(mode)
        seq, (fh, _), (bh, _) = rn.birnn_layer(x, p, "rnn_", mode, None)
        assert np.abs(seq - g["seq"]).max() < 1e-6 and np.abs(fh - g["h_fwd"]).max() < 1e-6 and np.abs(bh - g["h_bwd"]).max() < 1e-6
        rag, _, (rbh, _) = rn.birnn_layer(x, p, "rnn_", mode, vl)
        assert np.abs(rag - g["seq_ragged"]).max() < 1e-6 and np.abs(rbh - g["h_bwd_ragged"]).max() < 1e-6
        assert np.all(rag[1, 5:] == 0)                                  # steps past valid_length emit zeros
    c = mk.GN
    p, src, vl = mk.gnmt_inputs()
    mem, states = gn.encoder(src, vl, p, "gru", c["H"])
    dec = gn.Decoder(p, c["H"], cell="gru")
    g = np.load(os.path.join(GOLD, "oracle_gnmt_step.npz"))
    rnn_states, att = dec.init_state(mem, states, vl)
    logp, ns, ctx = dec.step(g["tokens"], rnn_states, att, np.arange(c["B"]))
    assert np.abs(mem - g["mem"]).max() < 1e-6 and np.abs(logp - g["logp"]).max() < 1e-5 and np.abs(ctx - g["ctx"]).max() < 1e-6
    t = np.load(os.path.join(GOLD, "oracle_beam_trace.npz"))
    s, sc, vlen = gn.beam_search(dec, mem, states, vl, 2, 3, c["beam"], 1.0, 5, c["max_length"])
    assert np.array_equal(s, t["samples"]) and np.array_equal(vlen, t["valid_length"]) and np.abs(sc - t["scores"]).max() < 1e-5
    d = np.load(os.path.join(GOLD, "oracle_densenet121_224_b2.npz"))
    p, x = mk.densenet_inputs()
    taps = {}
    feats = dn.densenet121_features(x[:1], p, taps=taps)               # one of the two frames keeps the CPU suite short
    assert np.abs(feats - d["feats"][:1]).max() < 1e-5
    assert np.abs(dn.dense(feats, p, "framemodel0_dense0_") - d["logits"][:1]).max() < 1e-5


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_gnmt_train_oracle_forward_matches_numpy_oracle(cell):
    """oracle/gnmt_train_torch.py (torch, for autograd) computes the same teacher-forced logits and loss as the numpy
    restatement oracle/gnmt_np.py it is written from; MXNet Adam's first step moves every weight by ~lr."""
    from oracle import gnmt_np as gn, gnmt_train_torch as gt
    from tennis_amd import weights as W
    B, T, F, H, E, V, L = 3, 9, 16, 8, 6, 14, 6
    p = W.make_gnmt_weights(1, cell, F, H, E, V)
    rng = np.random.default_rng(0)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    vl = np.array([9, 5, 7], np.int32)
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0] = 2
    tvl = np.array([6, 4, 5], np.int32)
    loss, logits, g = gt.loss_and_grads(p, src, vl, tgt, tvl, H, cell=cell)
    mem, states = gn.encoder(src, vl, p, cell, H)
    ref = gn.decode_seq(gn.Decoder(p, H, cell=cell), mem, states, vl, tgt[:, :-1])
    assert np.abs(logits - ref).max() < 1e-6
    rl = gn.masked_softmax_ce(ref, tgt[:, 1:], tvl - 1)
    assert abs(loss - float(rl.mean() * (L - 1) / np.mean(tvl - 1))) < 1e-5          # train_gnmt.py:332-333
    assert set(g) == set(p) and all(np.isfinite(v).all() for v in g.values())
    q, m, v = gt.adam_step({k: a.astype(np.float64) for k, a in p.items()}, g, {}, {}, 1, 1e-3)
    k = "gnmt_tgt_proj_bias"
    moved = np.abs(q[k] - p[k])
    assert np.all(moved[np.abs(g[k]) > 1e-6] > 0.9e-3) and np.all(moved < 1.01e-3)


@pytest.mark.parametrize("nl,nbi,res,cell", [(3, 1, False, "gru"), (4, 2, True, "gru"), (3, 0, True, "lstm"), (2, 1, True, "lstm")])
def test_gnmt_train_oracle_layer_counts_match_numpy_oracle(nl, nbi, res, cell):
    """the training oracle's general form (num_layers / num_bi_layers / use_residual, gnmt.py:136-160,369-404) against the numpy
    restatement the inference tests use, which was written separately (oracle/gnmt_np.py::encoder / Decoder)."""
    from oracle import gnmt_np as gn, gnmt_train_torch as gt
    from tennis_amd import weights as W
    B, T, F, H, E, V, L = 3, 9, 16, 8, 6, 14, 6
    p = W.make_gnmt_weights(2, cell, F, H, E, V, num_layers=nl, num_bi_layers=nbi)
    rng = np.random.default_rng(1)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    vl = np.array([9, 5, 7], np.int32)
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0] = 2
    tvl = np.array([6, 4, 5], np.int32)
    loss, logits, g = gt.loss_and_grads(p, src, vl, tgt, tvl, H, cell=cell, num_layers=nl, num_bi_layers=nbi, use_residual=res)
    mem, states = gn.encoder(src, vl, p, cell, H, num_layers=nl, num_bi_layers=nbi, use_residual=res)
    ref = gn.decode_seq(gn.Decoder(p, H, cell=cell, num_layers=nl, use_residual=res), mem, states, vl, tgt[:, :-1])
    assert np.abs(logits - ref).max() < 1e-6
    assert set(g) == set(p) and all(np.isfinite(v).all() for v in g.values())
    assert all(np.abs(v).max() > 0 for k, v in g.items() if "enc_rnn0_l_" not in k or nbi > 0)


def test_vector_feedback_rounding_library_vs_numpy():
    """tn_round_fp16_calibrated (csrc/calib_host.hip, host code) against its numpy reference: the same neighbour for every weight,
    every weight ON one of its two neighbours, representable weights untouched, and the property the method is for - the row
    errors against EVERY calibration vector shrink, not only against their mean."""
    from tennis_amd import weights as W
    rng = np.random.default_rng(5)
    w = rng.normal(0, 0.05, (48, 300)).astype(np.float32).astype(np.float64)
    A = np.abs(rng.normal(0.4, 0.3, (20, 300))) * rng.uniform(0.3, 2.0, (20, 1))
    a = W._round_fp16_vector_feedback(w, A, use_library=True)
    b = W._round_fp16_vector_feedback(w, A, use_library=False)
    assert np.array_equal(a, b)
    lo = w.astype(np.float16)
    up = np.nextafter(lo, np.where(w > lo.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    assert np.all((a == lo.astype(np.float64)) | (a == up.astype(np.float64)))
    w16 = lo.astype(np.float64)
    assert np.array_equal(W._round_fp16_vector_feedback(w16, A), w16)
    per_frame = lambda r: np.abs((r - w) @ A.T)                       # (rows, frames)
    e_rtn, e_vec = per_frame(w16), per_frame(a)
    e_mean = per_frame(W._round_fp16_error_feedback(w, A.mean(0)))
    assert e_vec.max() < 0.25 * e_rtn.max() and np.sqrt((e_vec ** 2).mean()) < 0.15 * np.sqrt((e_rtn ** 2).mean())
    assert np.sqrt((e_vec ** 2).mean()) < 0.5 * np.sqrt((e_mean ** 2).mean())      # the mean-only method leaves the per-frame part
    # through as_fp16_model: 2-D input_means select the vector method, conv by conv
    p = W.make_densenet121_weights(3, fp16_model=False)
    name = "densenet0_stage1_conv0_weight"
    q = W.as_fp16_model(p, input_means={name: np.abs(rng.normal(0.5, 0.2, (6, p[name].shape[1])))})
    plain = W.as_fp16_model(p)
    rm = "densenet0_stage1_batchnorm1_running_mean"
    assert all(np.array_equal(q[k], plain[k]) for k in p if k not in (name, rm)) and (q[name] != plain[name]).any()
    # round 5, bias correction: the mean conversion error of the 1x1's output over the calibration rows sits in the running mean
    # of the BatchNorm behind it (the only consumer), in the model's own units: sum_k (w_conv - w)[n, k] E[relu(bn1(x))[k]]
    q2 = W.as_fp16_model(p, input_means={name: np.abs(np.random.default_rng(11).normal(0.5, 0.2, (6, p[name].shape[1])))})
    q2n = W.as_fp16_model(p, input_means={name: np.abs(np.random.default_rng(11).normal(0.5, 0.2, (6, p[name].shape[1])))}, bias_correction=False)
    assert np.array_equal(q2n[rm], p[rm]) and not np.array_equal(q2[rm], p[rm])
    _, _, sw1, tc1 = W.bn_relu_clamp_fold(p, "densenet0_stage1_batchnorm0")
    ybar = sw1.astype(np.float64) * np.abs(np.random.default_rng(11).normal(0.5, 0.2, (6, p[name].shape[1]))).mean(0) + tc1
    want = (q2[name].astype(np.float64) - p[name]).sum((2, 3)) @ ybar
    assert np.allclose(q2[rm].astype(np.float64) - p[rm], want, rtol=1e-3, atol=1e-7)


def test_bias_correction_reaches_exactly_the_consumers_of_a_channel():
    """weights._apply_bias_correction (round 5): the mean conversion error of a convolution's output channels is added to the
    running mean of EVERY BatchNorm that reads those channels and of no other - DenseNet's concat topology (reference call site
    models/vision/definitions.py:30 -> gluoncv DenseNet: a dense layer's 32 new channels are read by every later layer of its block
    and by the block's closing BatchNorm; a transition's outputs by every layer of the next block and its closing BatchNorm; a 1x1
    by the BatchNorm behind it; the stem by batchnorm0)."""
    from tennis_amd import weights as W
    p = W.make_densenet121_weights(2, fp16_model=False)
    pre = "densenet0_"

    def changed(bias):
        out = dict(p)
        W._apply_bias_correction(out, bias, pre)
        ch = {}
        for k in p:
            if k.endswith("_running_mean") and not np.array_equal(out[k], p[k]):
                idx = np.nonzero(out[k] != p[k])[0]
                ch[k[len(pre):-len("_running_mean")]] = (int(idx[0]), int(idx[-1]) + 1, out[k][idx] - p[k][idx])
        return ch
    # the 3x3 of layer 2 in block 2 (K0 = 128): channels [128 + 64, 128 + 96) of the block's buffer
    b = np.linspace(0.01, 0.32, 32)
    ch = changed({pre + "stage2_conv5_weight": b})
    want = {f"stage2_batchnorm{2 * l}" for l in range(3, 12)} | {"batchnorm2"}
    assert set(ch) == want
    for lo, hi, d in ch.values():
        assert (lo, hi) == (192, 224) and np.allclose(d, b, rtol=1e-5)
    # a 1x1: the BatchNorm behind it only
    ch = changed({pre + "stage3_conv10_weight": np.full(128, 0.5)})
    assert set(ch) == {"stage3_batchnorm11"} and ch["stage3_batchnorm11"][:2] == (0, 128)
    # transition 2 (conv2: 512 -> 256): every BN1 of block 3 and the block's closing BatchNorm, channels [0, 256)
    ch = changed({pre + "conv2_weight": np.full(256, -0.25)})
    assert set(ch) == {f"stage3_batchnorm{2 * l}" for l in range(24)} | {"batchnorm3"}
    assert all(v[:2] == (0, 256) for v in ch.values())
    # the last block closes with the head's BatchNorm; the stem feeds batchnorm0 (the stem's own BatchNorm) only
    ch = changed({pre + "stage4_conv31_weight": np.full(32, 1.0)})
    assert set(ch) == {"batchnorm4"} and ch["batchnorm4"][:2] == (512 + 15 * 32, 1024)
    ch = changed({pre + "conv0_weight": np.full(64, 1.0)})
    assert set(ch) == {"batchnorm0"}
    # and through as_fp16_model: no 2-D means, no correction (the plain conversion of rounds 1 - 4 is unchanged)
    q = W.as_fp16_model(p)
    assert all(np.array_equal(q[k], p[k]) for k in p if k.endswith("_running_mean"))


def test_conversion_keeps_the_weights_of_near_dead_channels():
    """Round 6 (scripts/dead_debug.py).  A near-dead BatchNorm channel in front of a 1x1 (gamma 1e-5) folds its weights into fp16's
    subnormals; un-folding the few bits that are left handed the library - which needs w[n][k] exactly for the constant tc[k] w[n][k]
    of the clamp form - weights that were up to 100 % off: 8e-3 on the features for dead channels with a positive beta.  Those
    weights now stay as they are, the others still become fp16 numbers once folded."""
    from tennis_amd import weights as W
    rng = np.random.default_rng(11)
    n = 256
    q = {"densenet0_stage1_conv0_weight": rng.normal(0, 0.1, (128, n, 1, 1)).astype(np.float32)}
    g = rng.uniform(0.5, 1.5, n).astype(np.float32)
    dead = np.zeros(n, bool); dead[::9] = True
    g[dead] *= (10.0 ** rng.uniform(-7, -4, int(dead.sum()))).astype(np.float32)
    q.update({"densenet0_stage1_batchnorm0_gamma": g, "densenet0_stage1_batchnorm0_beta": np.abs(rng.normal(0, 0.3, n)).astype(np.float32),
              "densenet0_stage1_batchnorm0_running_mean": np.zeros(n, np.float32), "densenet0_stage1_batchnorm0_running_var": np.ones(n, np.float32),
              "densenet0_stage1_batchnorm1_gamma": np.ones(128, np.float32), "densenet0_stage1_batchnorm1_beta": np.zeros(128, np.float32),
              "densenet0_stage1_batchnorm1_running_mean": np.zeros(128, np.float32), "densenet0_stage1_batchnorm1_running_var": np.ones(128, np.float32)})
    w = q["densenet0_stage1_conv0_weight"]
    conv = W.as_fp16_model(q)["densenet0_stage1_conv0_weight"]
    assert np.array_equal(conv[:, dead], w[:, dead])                      # untouched: the constant beta * w is what these channels contribute
    live = ~dead
    rel = np.abs(conv[:, live] - w[:, live]) / np.abs(w[:, live])
    assert rel.max() < 2.0 ** -10 and (conv[:, live] != w[:, live]).mean() > 0.9        # rounded once, to a neighbour


def test_operand_means_oracle_units_hold_together():
    """tests/tools/operand_means.py, the fp64 oracle of tn_densenet121_input_means, at 224x224 on one frame: the 119 keys are exactly
    the non-stem convolutions of densenet121_layout() in execution order, their lengths add up to the library's numel (per dense layer
    K + 128, per transition its K), and the two units of a dense layer's 1x1 hold together - sw * mean(clamp(x, lo, hi)) + tc is the
    mean of relu(bn(x)) from the same graph, up to |s| times the fp16 rounding of the ReLU threshold.  On the parameter set with
    planted degenerate channels, whose clamp operand is exactly 0."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tools import operand_means as OM
    pre = "densenet0_"
    p = OM.with_degenerate_channels(W.make_densenet121_weights(0))
    relu = {}
    m = OM.operand_means(p, W.synthetic_frames_u8(1, 224), relu_means=relu)
    convs, _, _ = W.densenet121_layout()
    assert list(m) == [pre + c["name"] + "_weight" for c in convs if c["kind"] != "stem"]
    assert all(m[pre + c["name"] + "_weight"].shape == (1, c["cin"]) for c in convs if c["kind"] != "stem")
    numel, c = 0, W.INIT_FEATURES                     # csrc/encoder.hip tn_densenet121_input_means
    for b, nl in enumerate(W.BLOCK_CONFIG):
        numel += sum(c + W.GROWTH * l + 128 for l in range(nl))
        c += W.GROWTH * nl
        if b < 3:
            numel += c
            c //= 2
    assert sum(v.size for v in m.values()) == numel == 40736
    assert set(relu) == {pre + c["name"] + "_weight" for c in convs if c["kind"] == "dense1x1"}
    n_off = 0
    for c in (c for c in convs if c["kind"] == "dense1x1"):
        k, bn = pre + c["name"] + "_weight", pre + c["bn"]
        lo, hi, sw, tc = W.bn_relu_clamp_fold(p, bn)
        s = (p[bn + "_gamma"] / np.sqrt(p[bn + "_running_var"] + np.float32(W.BN_EPS))).astype(np.float32).astype(np.float64)
        t = (p[bn + "_beta"] - p[bn + "_running_mean"] * s.astype(np.float32)).astype(np.float32).astype(np.float64)
        thr = np.where(s > 0, lo, hi).astype(np.float64)
        off = lo == hi
        slack = np.where(off, 0.0, np.abs(s) * np.abs(thr + t / np.where(s != 0, s, 1.0)))
        got = sw.astype(np.float64) * m[k][0] + tc
        want = relu[k][0]
        assert (np.abs(got - want) <= slack + 1e-6 * (np.abs(want) + np.abs(tc) + np.abs(sw) * np.abs(m[k][0])) + 1e-9).all(), k
        assert (m[k][0][off] == 0).all()
        n_off += int(off.sum())
    assert n_off == 3                                 # the three planted degenerate channels of stage1_conv4's operand
    bn = pre + "stage1_batchnorm4"
    assert list(np.flatnonzero(W.bn_relu_clamp_fold(p, bn)[0] == W.bn_relu_clamp_fold(p, bn)[1])) == [3, 17, 58]
    assert W.bn_relu_clamp_fold(p, bn)[2][40] < 0 and m[pre + "stage1_conv4_weight"][0][40] > 0
