"""Host side of the temporal-head training path — counterparts of reference train.py:
``gluon.Trainer(params, 'sgd', {...})`` (:298-299), ``gluon.loss.SoftmaxCrossEntropyLoss`` (:324) and
``train_model`` (:388-499) for ``CNNRNN(model=None, type='gru'|'lstm')`` on pre-extracted features (the frozen-backbone
recipe, e.g. model 0042 of models/README.md:57-59; ``engine.TemporalHeadTrainer``) and for the end-to-end frame classifier
``FrameModel(DenseNet121.features, classes)`` with BatchNorm in training mode (model 0006; ``engine.FrameModelTrainer``) — both
expose ``forward_backward(x, labels) -> (loss, logits)``, ``step(batch_size, lr, momentum, wd)``, ``grads`` and ``state_dict()``.
All arithmetic runs in libtennis_hip (tn_head_* / tn_finetune_*); torch is the
buffer / collective plumbing: with ``torch.distributed`` initialised (backend nccl = RCCL) every rank trains on its
shard of the batch and the flat gradient buffer is all-reduced before the update.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .engine import TemporalHeadTrainer


def allreduce_and_step(trainer, global_batch_size: int, lr: float, momentum: float, wd: float):
    """``trainer.step(batch_size)`` of a data-parallel run: sum the per-rank gradients of the summed losses, then
    Gluon's rescale 1/batch_size with the GLOBAL batch size (reference: one Trainer over all devices,
    ``trainer.step(FLAGS.batch_size)``, train.py:424).  ``trainer.grads`` is one flat buffer or a tuple of them
    (``CNNRNNTrainer``: backbone and head, or the head alone with a frozen backbone): every one is summed."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        grads = trainer.grads
        for g in (grads if isinstance(grads, (tuple, list)) else (grads,)):
            comm = _grad_comm(g.device)
            if comm is not None:
                comm.allreduce_(g).wait()              # tn_allreduce_f32: RCCL behind the C-ABI
            else:
                dist.all_reduce(g, op=dist.ReduceOp.SUM)
    trainer.step(global_batch_size, lr, momentum, wd)


_COMMS = {}


def _grad_comm(device):
    """The process's C-ABI communicator over the default group (GPU runs; None on CPU: the gloo tests)."""
    if device.type != "cuda":
        return None
    if device.index not in _COMMS:
        from . import sharding
        _COMMS[device.index] = sharding.feature_comm(device)
    return _COMMS[device.index]


class Trainer:
    """``gluon.Trainer(model.collect_params(), 'sgd', {'learning_rate', 'momentum', 'wd'})`` for the temporal head."""

    def __init__(self, head: TemporalHeadTrainer, optimizer: str = "sgd", optimizer_params: dict | None = None):
        if optimizer != "sgd":
            raise ValueError("only 'sgd' is built (reference train.py:298)")
        op = dict(optimizer_params or {})
        self.head = head
        self.learning_rate = float(op.get("learning_rate", 0.01))
        self.momentum = float(op.get("momentum", 0.0))
        self.wd = float(op.get("wd", 0.0))

    def set_learning_rate(self, lr: float):
        self.learning_rate = float(lr)

    def step(self, batch_size: int):
        allreduce_and_step(self.head, batch_size, self.learning_rate, self.momentum, self.wd)


def best_epoch_from_scores(scores_path: str):
    """(epoch, score) of the best line of ``scores.txt`` ("epoch<TAB>AVG_NB_f1" per validated epoch, written by
    ``train_model``; read back the way reference evaluate.py:186-195 / train.py:334-342 do: first strict maximum)."""
    best_epoch, best_score = -1, -1.0
    with open(scores_path, "r") as f:
        for line in f:
            parts = line.rstrip().split()
            if len(parts) != 2:
                continue
            if float(parts[1]) > best_score:
                best_epoch, best_score = int(parts[0]), float(parts[1])
    return best_epoch, best_score


def newest_params(save_dir: str):
    """Newest ``NNNN.params`` of an experiment directory or None (reference train.py:287-293, evaluate.py:206-212)."""
    if not os.path.isdir(save_dir):
        return None
    files = sorted((f for f in os.listdir(save_dir) if f.endswith(".params")), reverse=True)
    return os.path.join(save_dir, files[0]) if files else None


def is_main_rank() -> bool:
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


def train_model(head: TemporalHeadTrainer, train_batches, metrics, trainer: Trainer, epochs: int, batch_size: int,
                lr_steps=(10, 20), lr_factor: float = 0.75, start_epoch: int = 0, val_fn=None, save_dir: str | None = None,
                log=print, model=None, score_key: str = "AVG_NB_f1", step_fn=None, clip: float = 0.0):
    """reference train.py:388-499 with the model call, loss and backward fused into ``head.forward_backward``.
    ``train_batches``: callable -> iterable of (features (B,T,F) tensor, labels (B,) tensor) per epoch.
    Per epoch (rank 0 only): the validation ``AVG_NB_f1`` is appended to ``<save_dir>/scores.txt`` (:487-489) and the
    parameters go to ``<save_dir>/NNNN.params`` (:497) — through ``model.save_parameters`` (the MXNet container with
    Gluon's structural names, what the reference's ``load_parameters`` reads) when the mirror ``model`` is given,
    else an ``.npz`` of the trainer's prefixed names under ``NNNN.npz``.  ``step_fn``: what a step calls instead of
    ``head.forward_backward`` (``--dense_windows``: ``head.forward_backward_rows`` on (window rows (B,T), labels) batches).
    ``clip`` > 0 (``--clip_grad_norm``, not in the reference): ``head.set_clip(clip)`` - the global norm of ``rescale_grad * g`` over
    every trainable gradient is held at ``clip`` inside ``step``; each epoch's row then carries ``grad_norm`` (the last step's) and
    ``clipped_steps`` (the epoch's), read once per epoch."""
    step_fn = step_fn or head.forward_backward
    if clip:
        head.set_clip(clip)
    clipped_before = 0
    lr_counter = 0
    lr_steps = list(lr_steps) + [1 << 30]
    history = []
    for epoch in range(0, start_epoch):                                     # a resumed run keeps the schedule it had
        if epoch == lr_steps[lr_counter]:
            trainer.set_learning_rate(trainer.learning_rate * lr_factor)
            lr_counter += 1
    for epoch in range(start_epoch, epochs):
        if epoch == lr_steps[lr_counter]:                                   # :395-397
            trainer.set_learning_rate(trainer.learning_rate * lr_factor)
            lr_counter += 1
        for m in metrics:
            m.reset()
        train_sum_loss, nb = 0.0, 0
        for x, y in train_batches():
            loss, logits = step_fn(x, y)                                    # :415-421
            trainer.step(batch_size)                                        # :424
            train_sum_loss += float(loss.mean())                            # :427
            nb += 1
            for m in metrics:
                m.update([y], [logits])                                     # :430-431
        row = {"epoch": epoch, "lr": trainer.learning_rate, "loss": train_sum_loss / max(1, nb)}
        if clip and nb:
            norm, _, clipped = head.clip_stats()
            row["grad_norm"], row["clipped_steps"] = norm, clipped - clipped_before
            clipped_before = clipped
        if val_fn is not None:
            row["val"] = val_fn(head)
        history.append(row)
        log("[Epoch {}] loss: {:.3f} lr: {:.2E}".format(epoch, row["loss"], trainer.learning_rate))
        if "grad_norm" in row:
            log("[Epoch {}] grad_norm={:.4f} (last step), clipped_steps={} of {} (clip_grad_norm={})".format(
                epoch, row["grad_norm"], row["clipped_steps"], nb, clip))
            if not np.isfinite(row["grad_norm"]):
                log("[Epoch {}] WARNING: the gradient norm is not finite; the clipped updates carried it into the parameters".format(epoch))
        if save_dir and is_main_rank():
            os.makedirs(save_dir, exist_ok=True)
            if isinstance(row.get("val"), dict) and score_key in row["val"]:   # :487-489
                with open(os.path.join(save_dir, "scores.txt"), "a") as f:
                    f.write(str(epoch) + "\t" + str(float(row["val"][score_key])) + "\n")
            if model is not None:                                           # :497
                model.set_params(head.state_dict())
                model.save_parameters(os.path.join(save_dir, "{:04d}.params".format(epoch)))
            else:
                with open(os.path.join(save_dir, "{:04d}.npz".format(epoch)), "wb") as f:
                    np.savez(f, **head.state_dict())
    return history


def check_frames_route(flags):
    """The end-to-end routes on frames (no ``--feats_model``): ``--window 1`` (the frame classifier) or ``--window > 1`` with
    ``--temp_pool gru|lstm`` (CNNRNN).  Anything else exits with the reason."""
    if flags.feats_model is not None:
        if getattr(flags, "matmul", "f32") != "f32":
            raise SystemExit("--matmul fp32x3 switches the backbone's GEMMs; with --feats_model there is no backbone in the step "
                             "(the temporal head trains on stored features)")
        return
    if flags.window < 1:
        raise SystemExit("--window must be at least 1")
    if flags.window > 1 and flags.temp_pool not in ("gru", "lstm"):
        raise SystemExit("--window > 1 on frames trains CNNRNN and needs --temp_pool gru|lstm; mean / max have no parameters "
                         "of their own (the reference's train.py:236 leaves a FrameModel under a 5-D input there)")
    if flags.window == 1 and flags.freeze_backbone:
        raise SystemExit("--window 1 trains the frame classifier end to end; a frozen backbone trains on features "
                         "(--feats_model after evaluate --save_feats) or under a temporal head (--window > 1 --temp_pool gru|lstm)")


def check_dense_windows(flags):
    """``--dense_windows`` trains the temporal head from a device-resident feature table: it needs stored features, a window and a
    head with parameters.  Anything else exits with the reason."""
    if not getattr(flags, "dense_windows", False):
        return
    if flags.feats_model is None:
        raise SystemExit("--dense_windows gathers windows from a table of stored features and needs --feats_model "
                         "(after evaluate --save_feats); on frames the backbone runs in every step")
    if flags.window <= 1:
        raise SystemExit("--dense_windows needs --window > 1: with --window 1 there is no window to gather")
    if flags.temp_pool not in ("gru", "lstm"):
        raise SystemExit("--dense_windows needs --temp_pool gru|lstm: mean / max have no parameters to train")


class DeviceWindows:
    """One split for ``--dense_windows``: its feature table (``TennisSet.window_table`` / ``evaluate.load_feature_table``: every
    ``.npy`` read once), every sample's window rows ``idx`` (N, window) int32 and the labels, each uploaded once."""

    def __init__(self, dataset, feat_dim: int, device, split: str, log=print):
        import time
        from .evaluate import load_feature_table
        frames, idx = dataset.window_table()
        need = len(frames) * feat_dim * 4
        free = int(torch.cuda.mem_get_info(device)[0])
        if need > free:
            raise SystemExit(f"--dense_windows: the {split} split's feature table ({len(frames)} frames x {feat_dim} floats) needs "
                             f"{need} bytes and the device has {free} bytes free; train without --dense_windows, or thin the "
                             "split out with --every")
        t0 = time.perf_counter()
        table = load_feature_table(dataset, frames)
        self.table = torch.from_numpy(table).to(device)
        self.idx = torch.from_numpy(idx).to(device)
        labels = np.array([dataset.classes.index(s[2]) for s in dataset._samples])
        self.labels = torch.from_numpy(labels.astype(np.int32)).to(device)
        self.load_seconds = time.perf_counter() - t0
        log("[dense_windows] {} split: {} samples, table of {} frames ({} bytes) loaded in {:.2f} s".format(
            split, len(dataset), len(frames), need, self.load_seconds))

    def epoch_batches(self, loader, local_bs_of, max_batches: int = -1):
        """The epoch's batches from ``loader._batches()`` - the stream the loader route draws from, so the same seed gives the same
        order - as (window rows (b, window), labels (b,)) device slices.  ``local_bs_of(ids)``: the rows of a batch this rank trains on
        (None: the batch is dropped).  The epoch's sample order goes to the device in one copy; a step then only slices."""
        chosen = []
        for i, ids in enumerate(loader._batches()):
            if max_batches > 0 and i > max_batches:                         # train.py:405
                break
            ids = local_bs_of(ids)
            if ids is not None and len(ids):
                chosen.append(np.asarray(ids, np.int64))
        if not chosen:
            return
        order = torch.from_numpy(np.concatenate(chosen)).to(self.idx.device)
        rows, labels = self.idx[order], self.labels[order]                 # one gather per epoch
        a = 0
        for ids in chosen:
            yield rows[a:a + len(ids)], labels[a:a + len(ids)]
            a += len(ids)


def build_parser():
    import argparse
    p = argparse.ArgumentParser(description="tennis_amd train (flags of reference train.py:30-95)")
    p.add_argument("--backbone", default="DenseNet121")
    p.add_argument("--freeze_backbone", action="store_true")
    p.add_argument("--no_augment", action="store_true", help="test transform for the train split too (not a reference flag)")
    p.add_argument("--model_id", default="0000")
    p.add_argument("--split_id", default="02")
    p.add_argument("--data_shape", type=int, default=224)
    p.add_argument("--every", default="1, 1, 1")
    p.add_argument("--balance", default="True, False, False")
    p.add_argument("--window", type=int, default=1)
    p.add_argument("--padding", type=int, default=1)
    p.add_argument("--stride", type=int, default=1)
    p.add_argument("--batch_size", type=int, default=64,
                   help="end-to-end training on frames drops a ragged last batch (BatchNorm statistics are per batch)")
    p.add_argument("--epochs", type=int, default=20)
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--lr_factor", type=float, default=0.75)
    p.add_argument("--lr_steps", default="10, 20")
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--wd", type=float, default=0.0001)
    p.add_argument("--feats_model", default=None)
    p.add_argument("--dense_windows", action="store_true",
                   help="with --feats_model --window W --temp_pool gru|lstm: every split's features go to the device once as a table "
                        "and the training kernels gather each step's windows from it - no per-step file reads, stacking or "
                        "host-to-device copies; bit-identical parameters (not a reference flag)")
    p.add_argument("--clip_grad_norm", type=float, default=0.0,
                   help="X > 0: hold the global norm of the step's gradient (rescaled by 1 / batch_size, over every trainable "
                        "parameter) at X, gluon.utils.clip_global_norm; 0 = off, the reference's step (not a reference flag)")
    p.add_argument("--matmul", default="f32", choices=["f32", "fp32x3"],
                   help="matrix pipe of the backbone's GEMMs when training on frames: f32 (exact-f32 MFMA) or fp32x3 (fp32 values as "
                        "three bf16 terms on the bf16 MFMA, same float64 bars; not a reference flag)")
    # the rest of the reference's flags (train.py:32-93), accepted so that its command lines parse unchanged
    p.add_argument("--backbone_from_id", default=None, help="start the frame model from the newest .params of this model id (train.py:222-235)")
    p.add_argument("--log_interval", type=int, default=100)
    p.add_argument("--num_gpus", type=int, default=1, help="one process per GPU here: data parallelism comes from torch.distributed (train.allreduce_and_step)")
    p.add_argument("--vis", action="store_true", help="refused: outside the accelerated path (SURVEY 2a)")
    p.add_argument("--flow", default="", help="anything but '' is refused: outside the accelerated path (SURVEY 2a)")
    p.add_argument("--max_batches", type=int, default=-1, help="stop an epoch after this many batches (train.py:92: 'for 0031')")
    p.add_argument("--temp_pool", default=None, help="gru or lstm (trained); mean / max need no training")
    p.add_argument("--root", default="data")
    p.add_argument("--decode", default="device", choices=["device", "host", "auto"], help="where on-disk JPEG frames are decoded (see evaluate.py)")
    p.add_argument("--num_workers", type=int, default=3, help="loader threads (train.py:101-102), see evaluate.py")
    p.add_argument("--frames_per_video", type=int, default=16)
    p.add_argument("--exp_root", default=os.path.join("models", "vision", "experiments"))
    return p


def main(argv=None):
    """reference train.py::main (:98-386) for the three trainable configurations on the hot path:
      * ``--feats_model <id> --window W --temp_pool gru|lstm``: the temporal head on pre-extracted features (backbone frozen);
      * ``--window 1`` without ``--feats_model``: the frame classifier end to end (BatchNorm in training mode);
      * ``--window W > 1 --temp_pool gru|lstm`` without ``--feats_model``: CNNRNN over TimeDistributed frames end to end, or with
        ``--freeze_backbone`` the head alone over a backbone whose BatchNorms still run in training mode (train.py:197-236).
    End-to-end training on frames from disk uses the reference's TRAIN transform for the train split (RandomResizedCrop,
    RandomFlipLeftRight, RandomColorJitter(0.4, 0.4, 0.4), RandomLighting(0.1); train.py:125-139 - round 4: one GPU launch group per
    batch, ``tennis_amd.transforms``), the test transform for validation; ``--no_augment`` keeps the test transform everywhere."""
    from . import transforms
    from .dataset import DataLoader, TennisSet
    from .engine import CNNRNNTrainer, FrameModelTrainer, TemporalHeadTrainer
    from .sharding import init_distributed
    from .evaluate import evaluate_model
    from .metrics.vision import PRF1
    from .model_zoo import get_model
    from .models.vision.definitions import CNNRNN, FrameModel
    from . import weights as W
    flags = build_parser().parse_args(argv)
    if flags.flow or flags.vis:
        raise NotImplementedError("--flow / --vis: optical-flow input and visualisation are outside the accelerated path (SURVEY 2a)")
    check_frames_route(flags)
    check_dense_windows(flags)
    if not (np.isfinite(flags.clip_grad_norm) and flags.clip_grad_norm >= 0):
        raise SystemExit("--clip_grad_norm must be finite and >= 0 (0 = off)")
    if flags.num_workers < 0:                          # the reference's -1 = cpu_count() (train.py:101-102)
        flags.num_workers = 3                                               # (files -> features peaks at three decoder threads: scripts/bench_pipeline.py, profiles/r05_c_*)
    every = [int(s) for s in flags.every.split(",")]
    balance = [s.strip().lower() in ("true", "t") for s in flags.balance.split(",")]
    lr_steps = [int(s) for s in flags.lr_steps.split(",")]
    rank, world, dev = init_distributed()              # one process per GPU under torchrun, (0, 1, cuda:current) otherwise
    if flags.batch_size % world:
        raise SystemExit(f"--batch_size {flags.batch_size} must be a multiple of the {world} ranks")
    local_bs = flags.batch_size // world
    # frames on disk come at their native size: Resize(s + 32) / CenterCrop(s) / ToTensor / Normalize as evaluate.py:93-98
    # (one GPU launch per batch); the synthetic source already produces data_shape frames
    on_disk = flags.feats_model is None and os.path.exists(os.path.join(flags.root, "splits", flags.split_id, "train.txt"))
    tf = transforms.Compose([transforms.Resize(flags.data_shape + 32), transforms.CenterCrop(flags.data_shape),
                             transforms.ToTensor(),
                             transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])]) if on_disk else None
    # train.py:125-139: jitter_param = 0.4, lighting_param = 0.1 (every rank draws from its own seed: the ranks train on different rows)
    tf_train = transforms.Compose([transforms.RandomResizedCrop(flags.data_shape), transforms.RandomFlipLeftRight(),
                                   transforms.RandomColorJitter(brightness=0.4, contrast=0.4, saturation=0.4),
                                   transforms.RandomLighting(0.1), transforms.ToTensor(),
                                   transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])],
                                  seed=1000 + rank) if on_disk and not flags.no_augment else tf
    mk = lambda split, ev, bal: TennisSet(root=flags.root, transform=tf_train if split == "train" else tf, split=split, every=ev, padding=flags.padding,
                                          stride=flags.stride, window=flags.window, model_id=flags.model_id,
                                          split_id=flags.split_id, balance=bal, feats_model=flags.feats_model,
                                          data_shape=flags.data_shape, frames_per_video=flags.frames_per_video,
                                          decode=flags.decode)
    train_set, val_set = mk("train", every[0], balance[0]), mk("val", every[1], balance[1])
    n_cls = len(train_set.classes)
    save_dir = os.path.join(flags.exp_root, flags.model_id)
    if flags.feats_model is not None:
        if flags.window <= 1 or flags.temp_pool not in ("gru", "lstm"):
            raise SystemExit("training on features needs --window > 1 and --temp_pool gru|lstm (definitions.py:94-96)")
        feat_dim = int(np.asarray(train_set[0][0]).shape[-1])
        model = CNNRNN(None, num_classes=n_cls, type=flags.temp_pool, hidden_size=128)
        model.rnn._materialize(feat_dim)
        model.classes._materialize(256)
        last = "keep"
        mk_head = lambda p: TemporalHeadTrainer(p, feat_dim, 128, n_cls, max_batch=local_bs, max_steps=flags.window,
                                                rnn_prefix=model.rnn.prefix, dense_prefix=model.classes.prefix,
                                                type=flags.temp_pool)
    elif flags.window > 1:
        model = FrameModel(get_model(flags.backbone, pretrained=True).features, n_cls)
        model.initialize()
        model.classes._materialize(1024)
        if flags.backbone_from_id:                     # train.py:218-229: the FrameModel checkpoint, loaded before wrapping
            bb = newest_params(os.path.join(flags.exp_root, flags.backbone_from_id))
            if bb is not None:
                model.load_parameters(bb)
                print("Loaded backbone params: {}".format(bb))
        model = CNNRNN(model, num_classes=n_cls, type=flags.temp_pool, hidden_size=128)     # train.py:230
        model.rnn._materialize(1024)
        model.classes._materialize(256)
        last = "discard"
        mk_head = lambda p: CNNRNNTrainer(p, flags.data_shape, n_cls, batch=local_bs, steps=flags.window, type=flags.temp_pool,
                                          prefix=model.td.model.prefix, rnn_prefix=model.rnn.prefix,
                                          dense_prefix=model.classes.prefix, freeze_backbone=flags.freeze_backbone,
                                          matmul=flags.matmul)
    else:
        model = FrameModel(get_model(flags.backbone, pretrained=True).features, n_cls)
        model.initialize()
        model.classes._materialize(1024)
        if flags.backbone_from_id:                     # train.py:222-235 loads it for window > 1 only; a frame model started from
            bb = newest_params(os.path.join(flags.exp_root, flags.backbone_from_id))   # another experiment is the same request
            if bb is not None:
                model.load_parameters(bb)
                print("Loaded backbone params: {}".format(bb))
        last = "discard"
        mk_head = lambda p: FrameModelTrainer(p, flags.data_shape, n_cls, batch=local_bs, prefix=model.backbone.prefix,
                                              dense_prefix=model.classes.prefix, matmul=flags.matmul)
    # resume from the newest NNNN.params of the experiment (train.py:286-295)
    start_epoch = 0
    newest = newest_params(save_dir)
    if newest is not None:
        model.load_parameters(newest)
        start_epoch = int(os.path.basename(newest).split(".")[0]) + 1
        print("Loaded model params: {}".format(newest))
    head = mk_head({k: v.data for k, v in model.collect_params().items()})
    if flags.feats_model is None and is_main_rank():
        print("Backbone matmul: {}".format(head.matmul))
    train_data = DataLoader(train_set, flags.batch_size, shuffle=True, last_batch=last, num_workers=flags.num_workers)
    val_data = DataLoader(val_set, flags.batch_size, shuffle=False, num_workers=flags.num_workers)
    trainer = Trainer(head, "sgd", {"learning_rate": flags.lr, "momentum": flags.momentum, "wd": flags.wd})
    metrics = [PRF1(label_names=train_set.classes)]

    def batches():          # every rank walks the same (seeded) batches and trains on its rows rank::world of each
        for i, (data, labels, _) in enumerate(train_data):
            if flags.max_batches > 0 and i > flags.max_batches:             # train.py:405
                break
            x = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
            y = torch.from_numpy(labels.astype(np.int32))
            if world > 1:
                if x.shape[0] % world:
                    continue        # a ragged last batch cannot be split evenly: dropped in data-parallel runs
                x, y = x[rank::world], y[rank::world]
            yield x.to(dev), y.to(dev)

    def validate(h):                                     # train.py:445-470: the validation metrics of the updated model
        model.set_params(h.state_dict())
        vm = [PRF1(label_names=val_set.classes)]
        evaluate_model(model, val_data, val_set, vm)
        return dict(vm[0].get())

    step_fn = None
    if flags.dense_windows:
        log = print if is_main_rank() else (lambda *a: None)
        train_win = DeviceWindows(train_set, feat_dim, dev, "train", log)
        val_win = DeviceWindows(val_set, feat_dim, dev, "val", log)

        def my_rows(ids):           # the rows rank::world of a batch, as batches() slices them
            if world > 1:
                return None if len(ids) % world else ids[rank::world]
            return ids

        def batches():
            head.set_features(train_win.table)
            yield from train_win.epoch_batches(train_data, my_rows, flags.max_batches)

        def validate(h):            # predict_rows over the val split's table, PRF1 fed as evaluate_model feeds it
            h.set_features(val_win.table)
            vm = [PRF1(label_names=val_set.classes)]
            lab = val_win.labels.to(torch.float32)
            for a in range(0, len(val_set), local_bs):
                vm[0].update([lab[a:a + local_bs]], [h.predict_rows(val_win.idx[a:a + local_bs])])
            return dict(vm[0].get())

        step_fn = head.forward_backward_rows

    hist = train_model(head, batches, metrics, trainer, flags.epochs, flags.batch_size, lr_steps=lr_steps,
                       lr_factor=flags.lr_factor, start_epoch=start_epoch, val_fn=validate, save_dir=save_dir, model=model,
                       step_fn=step_fn, clip=flags.clip_grad_norm)
    if hist and is_main_rank():
        best = max(hist, key=lambda r: r["val"].get("AVG_NB_f1", 0.0))
        print("[Finished] best epoch {} val AVG_NB_f1={:.3f}".format(best["epoch"], best["val"].get("AVG_NB_f1", 0.0)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
