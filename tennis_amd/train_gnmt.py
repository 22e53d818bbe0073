"""Host side of the captioner's training path — counterpart of reference train_gnmt.py::train (:305-470): ``--cell_type gru`` or
``lstm``, ``--num_layers`` / ``--num_bi_layers`` as the reference's flags (:58-61; default 2 / 1), residual connections when the
model was built with them:

    trainer = gluon.Trainer(model.collect_params(), 'adam', {'learning_rate': lr})                      :310
    for epoch: for batch in train loader (FixedBucketSampler over target lengths):                      :318
        out, _ = model(src, tgt[:, :-1], src_valid_length, tgt_valid_length - 1)                        :331
        loss = loss_function(out, tgt[:, 1:], tgt_valid_length - 1).mean() * (L - 1) / mean(valid - 1)  :332-333
        loss.backward(); trainer.step(1)                                                                 :334,337
      evaluate valid / test: loss, BLEU of the beam-search translations, write them out                 :372-447
      keep the parameters with the best validation BLEU; lr *= lr_update_factor once
      epoch + 1 >= 2/3 of the epochs; save the epoch's parameters                                       :450-461

Without ``--feats_model`` the model holds the CNN (``src_embed = TimeDistributed(FrameModel(...).backbone)``, :148-186) and the
same step trains it, or with ``--freeze_backbone`` leaves it alone (:164-166): ``tn_gnmt_frames_trainer_*``.

All arithmetic runs in libtennis_hip (``tn_gnmt_trainer_*`` for the step, ``tn_gnmt_*`` for evaluation); with
``torch.distributed`` initialised (backend nccl = RCCL) every rank trains on its own batches and the flat gradient
buffer is averaged over ranks before the Adam update.  nlg-eval's METEOR / CIDEr stay external, as in the survey.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .captions import bucketed_batches, evaluate, to_device, upload_clip_table, write_sentences
from .engine import GNMTFramesTrainer, GNMTTrainer
from .metrics.bleu import compute_bleu


def allreduce_grads(trainer, n_tokens: int):
    """Data parallelism.  A rank's gradient is that of ITS per-token average loss over ``n_tokens`` target tokens; the
    global per-token average over all ranks' batches is sum_r(n_r * mean_r) / sum_r(n_r), so the gradients are
    weighted by the token counts: all-reduce n_r * g_r and n_r, then divide (reference loss: train_gnmt.py:332-333)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        gs = trainer.grads if isinstance(trainer.grads, tuple) else (trainer.grads,)     # frame mode: (backbone, captioner)
        cnt = torch.tensor([float(n_tokens)], dtype=torch.float32, device=gs[0].device)
        from .train import _grad_comm
        comm = _grad_comm(gs[0].device)
        for g in gs:
            g *= float(n_tokens)
            if comm is not None:                 # tn_allreduce_f32: RCCL behind the C-ABI
                comm.allreduce_(g)
            else:
                dist.all_reduce(g, op=dist.ReduceOp.SUM)
        if comm is not None:
            comm.allreduce_(cnt).wait()
        else:
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
        for g in gs:
            g /= cnt


def train(data_train, data_val, data_test, model, translator, epochs: int, batch_size: int, lr: float = 1e-3,
          lr_update_factor: float = 0.5, dropout: float = 0.0, num_buckets: int = 5, test_batch_size: int = 32,
          start_epoch: int = 0, save_dir: str | None = None, seed: int = 0, log=print, freeze_backbone: bool = False,
          frame_size: int | None = None, matmul: str = "f32", feats_on_device: bool = False, clip: float = 0.0):
    """-> history: one dict per epoch (train loss, valid / test loss and BLEU, learning rate).  A model with a ``src_embed`` trains on
    frames (``GNMTFramesTrainer``: the backbone inside the step, frozen or trainable); its checkpoints carry the backbone under the
    model's structural names (``src_embed.model. ...``).  ``matmul``: the matrix pipe of that backbone's GEMMs ("f32" | "fp32x3").
    ``feats_on_device`` (feature mode): each split's features are read once and uploaded as one table; the train step and the
    per-epoch validation / test passes gather their clips from it inside the kernels (``forward_backward_rows`` / ``encode_rows``)
    instead of reading one ``.npy`` per frame and copying a host-built batch every step.  Same parameters, losses and sentences.
    ``clip`` > 0: ``gluon.utils.clip_global_norm(grads, clip)`` between the backward and the update, as the gluonnlp script the
    reference's trainer came from has it and the reference does not (0, the default: no clipping, the reference's step); each
    epoch's record then carries ``grad_norm`` (the last step's) and ``clipped_steps`` (the epoch's)."""
    enc = model.encoder
    if enc._cell_type not in ("gru", "lstm"):
        raise NotImplementedError("the training step is built for GRU / LSTM cells")
    dec = model.decoder
    if bool(getattr(enc, "_use_residual", False)) != bool(getattr(dec, "_use_residual", False)) or enc._num_layers != dec._num_layers:
        raise ValueError("encoder and decoder must agree on num_layers and use_residual (get_gnmt_encoder_decoder builds them that way, "
                         "gnmt.py:397-416)")
    params = {k: v.data for k, v in model.collect_params().items()}
    max_t = max(l[0] for l in data_train.get_data_lens())
    max_l = max(l[-1] for l in data_train.get_data_lens())
    cell = dict(cell_type=enc._cell_type, num_layers=enc._num_layers, num_bi_layers=enc._num_bi_layers,
                use_residual=bool(getattr(enc, "_use_residual", False)))
    frame_mode = getattr(model, "src_embed", None) is not None
    if feats_on_device and frame_mode:
        raise ValueError("feats_on_device serves feature mode: a model with a src_embed trains on frames, which no feature table holds")
    if frame_mode:
        max_t = max(max_t, max(data_train.get_clip_lens()))
        # the side of the frames the step sees: --data_shape, else the batch transform's crop, else that of per-frame (T, 3, S, S) items
        item = data_train[0][0]
        side = frame_size or getattr(getattr(data_train, "_transform", None), "crop", None)
        if side is None and item.dtype == np.float32 and item.ndim == 4 and item.shape[1] == 3 and item.shape[2] == item.shape[3]:
            side = int(item.shape[-1])
        if side is None:
            raise ValueError("train: frame_size is needed - the items are decoded frames and their transform names no crop size")
        trainer = GNMTFramesTrainer(params, enc._hidden_size, model._embed_size, len(model.tgt_vocab), size=side, max_batch=batch_size,
                                    max_src_len=max_t, max_tgt_len=max_l, max_frames=frame_capacity(data_train, batch_size, num_buckets),
                                    prefix=model.prefix, backbone_prefix=model.src_embed.model.prefix, freeze_backbone=freeze_backbone,
                                    matmul=matmul, **cell)
        log("Backbone matmul: {}".format(trainer.matmul))
    else:
        if matmul != "f32":
            raise ValueError("matmul='fp32x3' switches the backbone's GEMMs; a model without src_embed trains on features and has no backbone")
        trainer = GNMTTrainer(params, model._input_size, enc._hidden_size, model._embed_size, len(model.tgt_vocab),
                              max_batch=batch_size, max_src_len=max_t, max_tgt_len=max_l, prefix=model.prefix, **cell)
    if dropout > 0:
        trainer.set_dropout(dropout, seed)
    if clip:
        trainer.set_clip(clip)
    clipped_before = 0
    val_tgt = data_val.get_captions(split=True) if data_val is not None else None
    test_tgt = data_test.get_captions(split=True) if data_test is not None else None
    best_valid_bleu, history = 0.0, []
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
    import torch.distributed as dist
    ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
    # one table per split, uploaded once; under torch.distributed every rank holds the whole table (the batch split is the loader's)
    tables = {id(ds): upload_clip_table(ds) for ds in (data_train, data_val, data_test) if feats_on_device and ds is not None}
    train_table, train_rows = tables.get(id(data_train), (None, None))
    for epoch_id in range(start_epoch, epochs):
        tot, nb = 0.0, 0
        # FixedBucketSampler(..., shuffle=True) of the training loader (utils/captioning.py:48-55)
        for src, tgt, svl, tvl, *_ in bucketed_batches(data_train, batch_size, num_buckets, shuffle=True, seed=seed,
                                                       epoch=epoch_id, rank=rank, world=world, rows=train_rows):
            if feats_on_device:
                loss = trainer.forward_backward_rows(train_table, src, svl.astype(np.int32), torch.from_numpy(tgt).cuda(),
                                                     torch.from_numpy(tvl.astype(np.int32)).cuda())
            else:
                loss = trainer.forward_backward(to_device(src), torch.from_numpy(svl.astype(np.int32)).cuda(),
                                                torch.from_numpy(tgt).cuda(), torch.from_numpy(tvl.astype(np.int32)).cuda())
            allreduce_grads(trainer, int((tvl.astype(np.int64) - 1).sum()))
            trainer.step(lr)                                                     # trainer.step(1)
            tot += float(loss)
            nb += 1
        rec = {"epoch": epoch_id, "train_loss": tot / max(1, nb), "lr": lr}
        if clip and nb:                                                          # one read per epoch: clip_stats synchronises
            norm, _, clipped = trainer.clip_stats()
            rec["grad_norm"], rec["clipped_steps"] = norm, clipped - clipped_before
            clipped_before = clipped
            log("[Epoch {}] grad_norm={:.4f} (last step), clipped_steps={} of {} (clip={})".format(epoch_id, norm, rec["clipped_steps"],
                                                                                                  nb, clip))
            if not math.isfinite(norm):
                log("[Epoch {}] WARNING: the gradient norm is not finite; the clipped updates carried it into the parameters".format(epoch_id))
        model.set_params(trainer.state_dict())                                   # evaluation runs on the updated weights
        for name, ds, ref in (("valid", data_val, val_tgt), ("test", data_test, test_tgt)):
            if ds is None:
                continue
            ev_table, ev_rows = tables.get(id(ds), (None, None))
            ev_loss, out = evaluate(bucketed_batches(ds, test_batch_size, num_buckets, rows=ev_rows), model, translator, data_train,
                                    table=ev_table)
            bleu = compute_bleu([ref], out)[0]
            rec[f"{name}_loss"], rec[f"{name}_bleu"] = ev_loss, bleu
            log("[Epoch {}] {} Loss={:.4f}, {} ppl={:.4f}, {} bleu={:.2f}".format(epoch_id, name, ev_loss, name,
                                                                                 math.exp(min(ev_loss, 50.0)), name, bleu * 100))
            if save_dir:
                write_sentences(out, os.path.join(save_dir, "epoch{:d}_{}_out.txt".format(epoch_id, name)))
        if save_dir and rec.get("valid_bleu", 0.0) > best_valid_bleu:            # :450-454
            best_valid_bleu = rec["valid_bleu"]
            model.save_parameters(os.path.join(save_dir, "valid_best.params"), structural=frame_mode)
        if epoch_id + 1 >= (epochs * 2) // 3:                                    # :456-459
            lr *= lr_update_factor
            log("Learning rate change to {}".format(lr))
        if save_dir:
            model.save_parameters(os.path.join(save_dir, "{:04d}.params".format(epoch_id)), structural=frame_mode)
        history.append(rec)
    return history


def frame_capacity(data_train, batch_size, num_buckets):
    """The most frames a training batch holds once padded (batch x its longest clip): batches are cut from the buckets in dataset
    order or permuted, so the bound is, per bucket, the ``batch_size`` longest clips' count x the longest clip."""
    tl = [l[-1] for l in data_train.get_data_lens()]
    lo, hi = min(tl), max(tl)
    width = max(1, math.ceil((hi - lo + 1) / num_buckets))
    buckets = {}
    for l, t in zip(tl, data_train.get_clip_lens()):
        buckets.setdefault((l - lo) // width, []).append(t)
    return max(min(batch_size, len(v)) * max(v) for v in buckets.values())


def build_parser():
    import argparse
    p = argparse.ArgumentParser(description="tennis_amd train_gnmt (flags of reference train_gnmt.py:48-118)")
    p.add_argument("--model_id", default="0000")
    p.add_argument("--epochs", type=int, default=40)
    p.add_argument("--num_hidden", type=int, default=128,
                   help="hidden size of every cell: a multiple of 4, at most 680 with --cell_type gru and 512 with lstm (gates * hidden <= 2048)")
    p.add_argument("--emb_size", type=int, default=100)
    p.add_argument("--dropout", type=float, default=0.2)
    p.add_argument("--num_layers", type=int, default=2)
    p.add_argument("--num_bi_layers", type=int, default=1)
    p.add_argument("--cell_type", default="gru")
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--beam_size", type=int, default=4)
    p.add_argument("--lp_alpha", type=float, default=1.0)
    p.add_argument("--lp_k", type=int, default=5)
    p.add_argument("--test_batch_size", type=int, default=32)
    p.add_argument("--num_buckets", type=int, default=5)
    p.add_argument("--tgt_max_len", type=int, default=50)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--lr_update_factor", type=float, default=0.5)
    p.add_argument("--every", type=int, default=1)
    p.add_argument("--feats_model", default=None, help="load CNN features as npy files from this model: <data_root>/features/<feats_model>/, "
                   "what `python -m tennis_amd.evaluate --save_feats --model_id <feats_model>` wrote (train_gnmt.py:116-117)")
    p.add_argument("--emb_file", default="embeddings-ex.txt", help="the word embedding file generated by train_embeddings.py, under "
                   "--data_root (train_gnmt.py:118; '' = a learned embedding of --emb_size)")
    p.add_argument("--data_root", default=None, help="the dataset directory (the reference's 'data': splits/, annotations/, features/, "
                   "the embedding file); without it the captions and features are synthetic")
    p.add_argument("--split_id", default="02")
    # the reference's remaining flags (train_gnmt.py:48-118), accepted so that its documented command lines run unchanged, e.g.
    # `python evaluate_gnmt.py --model_id 0102 --num_hidden 256 --backbone_from_id 0006 --feats_model 0006` (models/README.md:68)
    p.add_argument("--bucket_scheme", default="constant", choices=["constant"], help="bucket widths (only the reference's default is built)")
    p.add_argument("--bucket_ratio", type=float, default=0.0)
    p.add_argument("--optimizer", default="adam", choices=["adam"])
    p.add_argument("--clip", type=float, default=5.0, help="accepted; the reference defines the flag and never applies it (train_gnmt.py:305-470)")
    p.add_argument("--apply_clip", action="store_true",
                   help="apply --clip: gluon.utils.clip_global_norm(grads, clip) before every update, as the gluonnlp script behind the "
                        "reference's trainer does (not a reference flag; without it --clip stays accepted and ignored)")
    p.add_argument("--log_interval", type=int, default=100)
    p.add_argument("--num_gpus", type=int, default=1, help="the reference's captioner is single-GPU (train_gnmt.py:126-127); data parallelism here comes from torch.distributed")
    p.add_argument("--backbone", default="DenseNet121")
    p.add_argument("--backbone_from_id", default=None, help="frame mode only (the CNN inside the model); ignored with --feats_model, as in the reference")
    p.add_argument("--freeze_backbone", action="store_true")
    p.add_argument("--matmul", default="f32", choices=["f32", "fp32x3"],
                   help="frame mode: matrix pipe of the backbone's GEMMs, f32 (exact-f32 MFMA) or fp32x3 (fp32 values as three bf16 terms on "
                        "the bf16 MFMA, same float64 bars; not a reference flag)")
    p.add_argument("--feats_on_device", action="store_true",
                   help="feature mode: read each split's features once into one device-resident table and gather every batch's clips "
                        "from it inside the kernels, instead of one .npy read per frame and one host-to-device copy per batch (not a "
                        "reference flag; same results)")
    p.add_argument("--data_shape", type=int, default=512)
    p.add_argument("--feature_dim", type=int, default=1024, help="width of the pre-extracted frame features (feats_model)")
    p.add_argument("--n_points", type=int, default=64, help="synthetic source: points per split")
    p.add_argument("--root", default="models/captioning/experiments")
    p.add_argument("--no_augment", action="store_true", help="frame mode: the test transform for the train split too (not a reference flag)")
    p.add_argument("--frames", action="store_true", help="synthetic source (no --data_root): frame mode on synthetic frames")
    return p


def load_target_embedding(flags, vocab, log=print):
    """reference train_gnmt.py:210-220: ``TokenEmbedding.from_file(data/<emb_file>)`` + ``vocab.set_embedding`` -> the table the
    target ``nn.Embedding`` is initialised with, or None (no file asked for, or a synthetic run whose directory has none)."""
    from .models.captioning.gnmt import TokenEmbedding
    if not flags.emb_file:
        return None
    path = flags.emb_file if os.path.isabs(flags.emb_file) else os.path.join(flags.data_root or "data", flags.emb_file)
    if not os.path.exists(path):
        if flags.data_root is not None:
            raise FileNotFoundError(f"--emb_file: {path} does not exist (pass --emb_file '' for a learned embedding)")
        return None                            # synthetic source: nothing on disk to read
    vocab.set_embedding(TokenEmbedding.from_file(path))
    tab = vocab.embedding.idx_to_vec
    known = int((np.abs(tab).sum(1) > 0).sum())
    log("Loaded {} x {} target embedding from {} ({} of {} vocabulary tokens found)".format(tab.shape[0], tab.shape[1], path, known, len(vocab)))
    return tab


def build(flags):
    """Datasets, model and translator as reference train_gnmt.py:120-256 assembles them.  Feature mode (``--feats_model``): with
    ``--data_root`` the points, captions and per-frame ``.npy`` features come from disk (``TennisSet(captions=True, ...)``), the
    target embedding from ``--emb_file``; without it everything is synthetic.  Frame mode (``--data_root`` without ``--feats_model``,
    :148-186): the points' frames are the source, ``get_model(--backbone, pretrained=True).features`` inside ``FrameModel(..., 11)`` -
    from ``--backbone_from_id``'s newest parameters when given - is the model's ``src_embed = TimeDistributed(cnn_model.backbone)``,
    the train split gets the train transform of :172-179 (``--no_augment``: the test transform), val / test the test transform."""
    from .dataset import TennisSet
    from .models.captioning.gnmt import NMTModel, get_gnmt_encoder_decoder
    from .utils.translation import BeamSearchScorer, BeamSearchTranslator
    if flags.data_root is None and flags.feats_model is not None and os.path.isdir(os.path.join("data", "splits")):
        flags.data_root = "data"           # the reference's layout relative to the working directory (dataset.py:17: root='data')
    frame_mode = flags.feats_model is None and (flags.data_root is not None or getattr(flags, "frames", False))
    src_embed, tf, tf_train = None, None, None
    if frame_mode:
        src_embed = build_backbone(flags)
        if flags.data_root is not None:             # frames from disk: one GPU launch group per batch (tennis_amd.transforms)
            from . import transforms
            norm = [transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])]
            tf = transforms.Compose([transforms.Resize(flags.data_shape + 32), transforms.CenterCrop(flags.data_shape)] + norm)
            tf_train = tf if flags.no_augment else transforms.Compose(                                       # :172-179
                [transforms.RandomResizedCrop(flags.data_shape), transforms.RandomFlipLeftRight(),
                 transforms.RandomColorJitter(brightness=0.4, contrast=0.4, saturation=0.4), transforms.RandomLighting(0.1)] + norm, seed=1000)
    src = dict(root=flags.data_root, split_id=flags.split_id, feats_model=flags.feats_model) if flags.data_root is not None else dict(root=None)
    syn = {} if flags.data_root is not None else dict(feature_dim=flags.feature_dim)
    if frame_mode and flags.data_root is None:
        syn = dict(frames=True, data_shape=flags.data_shape)
    mk = lambda t: dict(transform=t) if frame_mode and flags.data_root is not None else {}
    data_train = TennisSet(captions=True, split="train", every=flags.every, max_cap_len=flags.tgt_max_len,
                           **src, **syn, **mk(tf_train), **({} if flags.data_root is not None else dict(n_points=flags.n_points)))
    data_val = TennisSet(captions=True, split="val", every=flags.every, vocab=data_train.vocab, inference=True,
                         **src, **syn, **mk(tf), **({} if flags.data_root is not None else dict(n_points=max(4, flags.n_points // 4))))
    data_test = TennisSet(captions=True, split="test", every=flags.every, vocab=data_train.vocab, inference=True,
                          **src, **syn, **mk(tf), **({} if flags.data_root is not None else dict(n_points=max(4, flags.n_points // 4))))
    if frame_mode:
        from . import weights as W
        feature_dim = W.densenet121_layout()[2]        # input_size is the backbone's feature width
    else:
        feature_dim = data_train[0][0].shape[1] if len(data_train) else flags.feature_dim  # the width evaluate --save_feats wrote
    tgt_embed = load_target_embedding(flags, data_train.vocab)
    enc, dec = get_gnmt_encoder_decoder(cell_type=flags.cell_type, hidden_size=flags.num_hidden, dropout=flags.dropout,
                                        num_layers=flags.num_layers, num_bi_layers=flags.num_bi_layers)
    model = NMTModel(src_vocab=None, tgt_vocab=data_train.vocab, encoder=enc, decoder=dec, embed_size=flags.emb_size,
                     prefix="gnmt_", input_size=feature_dim, tgt_embed=tgt_embed, src_embed=src_embed)   # train_gnmt.py:228-229
    model.initialize()
    translator = BeamSearchTranslator(model=model, beam_size=flags.beam_size,
                                      scorer=BeamSearchScorer(alpha=flags.lp_alpha, K=flags.lp_k),
                                      max_length=flags.tgt_max_len + 100)                     # train_gnmt.py:250-252
    return data_train, data_val, data_test, model, translator


def build_backbone(flags):
    """reference train_gnmt.py:149-170: the CNN of the frame-mode model, ``TimeDistributed(cnn_model.backbone)``"""
    from .model_zoo import get_model
    from .models.vision.definitions import FrameModel
    from .utils.layers import TimeDistributed
    cnn_model = FrameModel(get_model(flags.backbone, pretrained=True).features, 11)                          # :150-151
    if flags.backbone_from_id:                                                                               # :153-163
        d = os.path.join("models", "vision", "experiments", flags.backbone_from_id)
        if not os.path.isdir(d):
            raise FileNotFoundError("Experiment folder ({}) does not exist".format(d))                       # :161-162
        files = sorted(f for f in os.listdir(d) if f.endswith(".params"))
        if files:
            cnn_model.initialize()
            cnn_model.classes._materialize(1024)
            cnn_model.load_parameters(os.path.join(d, files[-1]))
            print("Loaded backbone params: {}".format(os.path.join(d, files[-1])))
    return TimeDistributed(cnn_model.backbone)                                                               # :168-170


def require_feature_mode(flags):
    """--feats_on_device is a feature-mode switch; in frame mode it ends the run with a message, like --matmul in feature mode"""
    frame_mode = flags.feats_model is None and (flags.data_root is not None or getattr(flags, "frames", False))
    if flags.feats_on_device and frame_mode:
        raise SystemExit("--feats_on_device keeps pre-extracted features on the GPU; without --feats_model (frame mode) the captioner "
                         "reads frames through its backbone and there is no feature table")


def applied_clip(flags) -> float:
    """What ``train`` gets as ``clip``: --clip only under --apply_clip, else 0 (the reference parses the flag and never uses it)"""
    return float(flags.clip) if flags.apply_clip else 0.0


def main(argv=None):
    flags = build_parser().parse_args(argv)
    if flags.apply_clip and not (math.isfinite(flags.clip) and flags.clip > 0):
        raise SystemExit("--apply_clip needs a finite --clip > 0")
    if flags.matmul != "f32" and (flags.feats_model is not None or (flags.data_root is None and not flags.frames)):
        raise SystemExit("--matmul fp32x3 switches the backbone's GEMMs; with --feats_model (or synthetic features) there is no backbone "
                         "in the step - the captioner trains on stored features")
    require_feature_mode(flags)
    data_train, data_val, data_test, model, translator = build(flags)
    save_dir = os.path.join(flags.root, flags.model_id)
    os.makedirs(save_dir, exist_ok=True)
    from .captions import write_sentences
    write_sentences(data_val.get_captions(split=True), os.path.join(save_dir, "val_gt.txt"))         # train_gnmt.py:205-208
    write_sentences(data_test.get_captions(split=True), os.path.join(save_dir, "test_gt.txt"))
    # resume (train_gnmt.py:232-244): the newest NNNN.params of the model id, valid_best.params aside
    start_epoch = 0
    files = sorted((f for f in os.listdir(save_dir) if f.endswith(".params") and f != "valid_best.params"), reverse=True)
    if files:
        start_epoch = int(files[0].split(".")[0]) + 1
        model.load_parameters(os.path.join(save_dir, files[0]))
        print("Loaded model params: {}".format(os.path.join(save_dir, files[0])))
    hist = train(data_train, data_val, data_test, model, translator, flags.epochs, flags.batch_size, lr=flags.lr,
                 lr_update_factor=flags.lr_update_factor, dropout=flags.dropout, num_buckets=flags.num_buckets,
                 test_batch_size=flags.test_batch_size, start_epoch=start_epoch, save_dir=save_dir,
                 freeze_backbone=flags.freeze_backbone, matmul=flags.matmul, feats_on_device=flags.feats_on_device, clip=applied_clip(flags), frame_size=flags.data_shape if getattr(model, "src_embed", None) is not None else None)
    if not hist:
        print("[Finished] nothing to do: {} epochs are on disk".format(start_epoch))
        return 0
    print("[Finished] best valid bleu={:.2f}".format(100 * max(h.get("valid_bleu", 0.0) for h in hist)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
